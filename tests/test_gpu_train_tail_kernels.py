"""GPU tests (``-m gpu``) of the tail of the train step through the C ABI, each entry point alone: scnattn_caption_loss_bwd (and
the sm1 / row_lse of scnattn_caption_loss_fwd it is chained behind once), scnattn_clamp_adam, scnattn_gather_rows_tm,
scnattn_scatter_add_rows_tm, scnattn_hidden_to_bm, scnattn_hidden_from_bm, scnattn_copy2d, scnattn_add_bcast_rows,
scnattn_reduce_slabs, scnattn_colsum_masked, scnattn_pool_permute_fwd / _bwd and scnattn_f32_to_bf16, judged per element
against fp64 with the three tiers of tests/train_tail_refs.py (bit-equal, sum, derived).

Buffers are guarded windows (tests/kernel_harness.py GBuf / GBuf16 / GBufI): NaN around every input and in the gaps its
strides leave, the sentinel around and inside every output, which must survive; every leading dimension the ABI takes is wider
than its row.  Every case runs twice and must give the same bits.  The shapes are the smallest at which each kernel can still
go wrong (one element, one below / at / above a 256-thread sweep, a vector boundary, the 1024-cell list of the scatter, the
second lap of a grid-stride loop), not the workload's.

The worst err / bound per kernel and result goes to the run's parity report; profiles/parity_report_train_tail_kernels.txt
keeps a copy."""
import pytest
import torch

import train_tail_refs as R
from kernel_harness import GBuf, GBuf16, GBufI, SENT, _call, _slab_buf, _sum_ok, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = ("train-step tail kernels vs fp64: worst |got - ref| / bound over all cases; three tiers: bit for bit, "
                "(n+8) 2^-24 sum|terms|, and the derived bounds of ce_bwd and clamp_adam (tests/train_tail_refs.py)")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _twice(what, run):
    """run() -> a tuple of host tensors; two runs on fresh buffers must agree in every bit"""
    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(_raw(u), _raw(v)), "%s: two runs differ" % what
    return a


# ---- caption_loss_bwd ---------------------------------------------------------------------------------------------------
_ALIGN = (("aligned", 0, 0), ("scores off", 1, 0), ("dscores off", 0, 1))     # (name, offset of scores, of dscores) in floats


def _loss_bwd(dev, scores, targets, lse, P, sm1, ms, md):
    B, T, V = scores.shape
    lens = torch.tensor(R.CE_LENS, dtype=torch.int32)

    def run():
        sb = GBuf(dev, (B, T, V), vals=scores, mis=ms)
        tb = GBufI(dev, B * R.CE_LDT, vals=targets, wide=True)
        dl = GBufI(dev, B, vals=lens)
        lb = GBuf(dev, (B * T,), vals=lse.reshape(-1))
        gb = GBuf(dev, (1,), vals=torch.tensor([R.GOUT]))
        ds = GBuf(dev, (B, T, V), out=True, mis=md)
        mb = GBuf(dev, (B, P), vals=sm1) if P else None
        da = GBuf(dev, (B, T, P), out=True, mis=1) if P else None
        _call("scnattn_caption_loss_bwd", dev, B, T, V, P, sb.ptr, tb.ptr, R.CE_LDT, dl.ptr, int(lens.sum()), lb.ptr,
              mb.ptr if P else None, R.ALPHA_C, gb.ptr, ds.ptr, da.ptr if P else None)
        return (ds.read("dscores"),) + ((da.read("dalphas"),) if P else ())
    return _twice("caption_loss_bwd", run)


@pytest.mark.parametrize("V", R.CE_VS)
def test_caption_loss_bwd(dev, V):
    """both forms of ce_bwd_kernel (the vector form needs V % 4 == 0 and BOTH maps on the 16-byte grid), NaN in the undecoded
    score rows, every bad label, and d alphas for every t at P = 0 (null) / 5 / 196"""
    for (name, ms, md), P in zip(_ALIGN, R.CE_PS):
        form = "ce_bwd vector" if V % 4 == 0 and not ms and not md else "ce_bwd scalar"
        sm1 = R.gen_alphas(P)[1] if P else None

        def bwd(scores, targets, lse32):
            got = _loss_bwd(dev, scores, targets, lse32, P, sm1, ms, md)
            if P:
                _sum_ok("alpha_reg_bwd", "dalphas", got[1], R.dalphas_ref(sm1, R.CE_T))
            return got[0]
        R.walk_ce(form, V, bwd)


@pytest.mark.parametrize("V", (1023, 1028))
def test_caption_loss_bwd_behind_the_forward_kernel(dev, V):
    """the backward on the forward kernel's own row_lse and sm1: the reference keeps the fp64 log-sum-exp and the bound is
    widened by the measured distance of the stored row_lse from it"""
    B, T, P = R.CE_B, R.CE_T, 5
    scores, targets = R.gen_ce(V)
    alphas, _ = R.gen_alphas(P)
    lens = torch.tensor(R.CE_LENS, dtype=torch.int32)

    def fwd():
        sb, ab = GBuf(dev, (B, T, V), vals=scores), GBuf(dev, (B, T, P), vals=alphas, mis=1)
        tb, dl = GBufI(dev, B * R.CE_LDT, vals=targets, wide=True), GBufI(dev, B, vals=lens)
        outs = [GBuf(dev, s, out=True) for s in ((B * T,), (B * T,), (B, P), (B,), (1,))]
        _call("scnattn_caption_loss_fwd", dev, B, T, V, P, sb.ptr, tb.ptr, R.CE_LDT, dl.ptr, int(lens.sum()), ab.ptr, R.ALPHA_C,
              *[o.ptr for o in outs])
        return tuple(o.read(n) for o, n in zip(outs, ("row_lse", "row_loss", "sm1", "reg_part", "loss")))
    row_lse, _, sm1, _, _ = _twice("caption_loss_fwd", fwd)
    _sum_ok("alpha_reg_fwd", "sm1", sm1, R.alpha_reg_ref(alphas))
    want = R.lse64(scores)
    live = torch.zeros(B, T, dtype=torch.bool)
    for b, t in R.ce_cells():
        live[b, t] = True
    row_lse = row_lse.reshape(B, T)
    assert bool((row_lse[~live] == 0).all())
    dlse = torch.where(live, (row_lse.double() - want).abs(), torch.zeros(B, T, dtype=torch.float64))
    print("row_lse: worst distance from fp64 %.3e" % float(dlse.max()))
    assert float(dlse.max()) <= 16 * R.U * float(want.abs().max())        # a log-sum-exp off by more is not a rounding matter
    got = _loss_bwd(dev, scores, targets, row_lse, P, sm1, 0, 0)
    R.judge_ce_bwd("ce_bwd chained", got[0], scores, targets, want, dlse)
    _sum_ok("alpha_reg_bwd", "dalphas", got[1], R.dalphas_ref(sm1, T))


# ---- clamp_adam ---------------------------------------------------------------------------------------------------------
def _adam_step(dev):
    def step(p, g, m, v, k, clip, gs):
        n = p.numel()

        def run():
            pb, mb, vb = (GBuf(dev, (n,), vals=x, out=True, mis=1) for x in (p, m, v))
            gb = GBuf(dev, (n,), vals=g, mis=1)
            _call("scnattn_clamp_adam", dev, n, pb.ptr, gb.ptr, mb.ptr, vb.ptr, R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS, k,
                  clip, gs)
            return pb.read("p"), mb.read("m"), vb.read("v")
        return _twice("clamp_adam", run)
    return step


@pytest.mark.parametrize("n", R.ADAM_NS)
def test_clamp_adam(dev, n):
    """one element .. the second lap of the grid-stride loop (4096 x 256 + 777); windows one float off alignment"""
    R.walk_adam("clamp_adam", n, _adam_step(dev))


def test_clamp_adam_keeps_a_nan_gradient(dev):
    """torch's clamp_ keeps NaN and Adam then makes that parameter NaN: the fused step must diverge as loudly"""
    p, g, m, v = R.gen_adam(257, 1)
    g[100] = R.NAN
    for gs in R.ADAM_GSCALES:
        p2, m2, v2 = _adam_step(dev)(p, g, m, v, 1, 5.0, gs)
        assert bool(m2[100].isnan()) and bool(v2[100].isnan()) and bool(p2[100].isnan()), \
            "a NaN gradient came out as m %r, v %r, p %r" % (float(m2[100]), float(v2[100]), float(p2[100]))
        assert int(p2.isnan().sum()) == 1 and int(m2.isnan().sum()) == 1 and int(v2.isnan().sum()) == 1
        R.judge_adam("clamp_adam nan", p2, m2, v2, p, g, m, v, R.adam_hyper(1, 5.0, gs))


# ---- embedding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.GATHER_MS)
def test_gather_rows_tm(dev, M):
    """L > T, tokens 0 and V-1, and the pinned clamping of -3 to row 0 and of V+2 to row V-1"""
    B, T, L, V = R.GATHER_B, R.GATHER_T, R.GATHER_L, R.GATHER_V
    caps, table = R.gen_gather(M)
    for mis in (0, 1):
        def run():
            cb, tb = GBufI(dev, B * L, vals=caps, wide=True), GBuf(dev, (V, M), vals=table, mis=mis)
            out = GBuf(dev, (T * B, M), out=True, mis=mis)
            _call("scnattn_gather_rows_tm", dev, B, T, L, M, cb.ptr, tb.ptr, V, out.ptr)
            return (out.read("out_tm"),)
        R.judge_bits("gather_rows_tm", "out", _twice("gather_rows_tm", run)[0], R.gather_ref(caps, table, T))


@pytest.mark.parametrize("count", R.SCAT_COUNTS)
@pytest.mark.parametrize("M", R.SCAT_MS)
def test_scatter_add_rows_tm(dev, M, count):
    """a token in 1025 cells (the ordered scan), in 1024 (the longest sorted list) and in 1023; an absent token keeps its
    bits; tokens out of range are skipped; the rows of inactive cells hold NaN"""
    B, T, L, V = R.SCAT_B, R.SCAT_T, R.SCAT_L, R.SCAT_V
    caps, lens, demb, dtable = R.gen_scatter(M, count)

    def run():
        cb, dl = GBufI(dev, B * L, vals=caps, wide=True), GBufI(dev, B, vals=torch.tensor(lens))
        eb = GBuf(dev, (T * B, M), vals=demb, mis=1)
        tb = GBuf(dev, (V, M), vals=dtable, out=True, mis=1)
        pb = GBufI(dev, V)
        _call("scnattn_scatter_add_rows_tm", dev, B, T, L, M, cb.ptr, dl.ptr, eb.ptr, V, tb.ptr, pb.ptr)
        return tb.read("dtable"), pb.read("present")
    got, present = _twice("scatter_add_rows_tm", run)
    R.judge_scatter("scatter_add scan" if count > 1024 else "scatter_add sorted", got, present, caps, lens, demb, dtable, T)
    assert torch.equal(_raw(got[R.SCAT_ABSENT]), _raw(dtable[R.SCAT_ABSENT]))


# ---- layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.HID_DS)
def test_hidden_to_bm_and_from_bm(dev, D):
    B, T = R.HID_B, R.HID_T
    lens = torch.tensor(R.HID_LENS, dtype=torch.int32)
    for to_bm in (True, False):
        src, mask = R.gen_hidden(D, to_bm)
        for mk in (None, mask):
            for with_rowmask in ((False, True) if to_bm else (False,)):
                def run():
                    dl, sb = GBufI(dev, B, vals=lens), GBuf(dev, (B * T, D), vals=src)
                    mb = None if mk is None else GBuf(dev, (B * T, D), vals=mk)
                    out = GBuf(dev, (B * T, D), out=True)
                    rb = GBuf(dev, (B * T,), out=True) if with_rowmask else None
                    if to_bm:
                        _call("scnattn_hidden_to_bm", dev, B, T, D, dl.ptr, sb.ptr, None if mb is None else mb.ptr, out.ptr,
                              None if rb is None else rb.ptr)
                    else:
                        _call("scnattn_hidden_from_bm", dev, B, T, D, dl.ptr, sb.ptr, None if mb is None else mb.ptr, out.ptr)
                    return (out.read("out"),) + ((rb.read("rowmask"),) if rb is not None else ())
                what = "hidden_to_bm" if to_bm else "hidden_from_bm"
                got = _twice(what, run)
                want, rowmask = R.hidden_ref(src, mk, to_bm)
                R.judge_bits(what, "out", got[0], want)
                if with_rowmask:
                    R.judge_bits(what, "rowmask", got[1], rowmask)


@pytest.mark.parametrize("shape", R.COPY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_copy2d(dev, shape):
    Rr, Cc = shape
    vals = torch.randn(Rr, Cc, generator=torch.Generator().manual_seed(Rr * 1000 + Cc))
    vals[0, 0] = -0.0

    def run():
        src, out = GBuf(dev, shape, (Cc + 3, 1), vals=vals, mis=1), GBuf(dev, shape, (Cc + 5, 1), out=True, mis=1)
        _call("scnattn_copy2d", dev, Rr, Cc, src.ptr, Cc + 3, out.ptr, Cc + 5)
        return (out.read("out"),)
    R.judge_bits("copy2d", "out", _twice("copy2d", run)[0], vals)


@pytest.mark.parametrize("E", R.BCAST_ES)
@pytest.mark.parametrize("P", R.BCAST_PS)
def test_add_bcast_rows(dev, P, E):
    x, v = R.gen_bcast(P, E)

    def run():
        xb, vb = GBuf(dev, (R.BCAST_B, P, E), vals=x, out=True, mis=1), GBuf(dev, (R.BCAST_B, E), vals=v)
        _call("scnattn_add_bcast_rows", dev, R.BCAST_B, P, E, vb.ptr, R.BCAST_SCALE, xb.ptr)
        return (xb.read("x"),)
    _sum_ok("add_bcast_rows", "x", _twice("add_bcast_rows", run)[0], R.bcast_ref(x, v))


@pytest.mark.parametrize("W", R.SLAB_WS)
@pytest.mark.parametrize("n", R.SLAB_NS)
def test_reduce_slabs(dev, n, W):
    vals = R.gen_slabs(n, W)

    def run():
        sb, stride, ld = _slab_buf(dev, vals)
        out = GBuf(dev, (R.SLAB_ROWS, W), out=True, mis=1)
        _call("scnattn_reduce_slabs", dev, R.SLAB_ROWS, W, sb.ptr, n, stride, ld, out.ptr)
        return (out.read("out"),)
    _sum_ok("reduce_slabs", "out", _twice("reduce_slabs", run)[0], R.slabs_ref(vals))


@pytest.mark.parametrize("N", R.COLSUM_NS)
def test_colsum_masked(dev, N):
    """select, not multiply: NaN and inf in the masked-out rows; beta = 0 does not read the old out (NaN)"""
    for Rr in R.COLSUM_RS:
        X, mask, old = R.gen_colsum(Rr, N)
        for beta in R.COLSUM_BETAS:
            def run():
                xb = GBuf(dev, X.shape, (N + 3, 1), vals=X, mis=1)
                mb = GBuf(dev, (mask.numel(),), vals=mask)
                out = GBuf(dev, (N,), vals=old if beta else None, out=True, mis=1)
                _call("scnattn_colsum_masked", dev, Rr, N, xb.ptr, N + 3, mb.ptr, out.ptr, beta)
                return (out.read("out"),)
            _sum_ok("colsum_masked", "out", _twice("colsum_masked", run)[0], R.colsum_ref(X, mask, old, Rr, beta))


# ---- pool_permute -----------------------------------------------------------------------------------------------------------
def _pool_strides(C, Hin, Win, channels_last):
    """(sxb, sxc, sxh, sxw) with gaps after every row, plane and image"""
    if channels_last:
        sxw = C + 3
        sxh = Win * sxw + 2
        return Hin * sxh + 1, 1, sxh, sxw
    sxh = Win + 3
    sxc = Hin * sxh + 5
    return C * sxc + 7, sxc, sxh, 1


@pytest.mark.parametrize("C", R.POOL_CS)
@pytest.mark.parametrize("size", R.POOL_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_pool_permute(dev, size, C):
    """up-sampling, down-sampling, identity, non-square maps and Ho != Wo; the channel loop loops at C = 300"""
    Hin, Win, Ho, Wo = size
    B = R.POOL_B
    x, dy = R.gen_pool2d(C, size)
    for cl in (False, True):
        st = _pool_strides(C, Hin, Win, cl)

        def fwd():
            xb, yb = GBuf(dev, x.shape, st, vals=x), GBuf(dev, (B, Ho, Wo, C), out=True)
            _call("scnattn_pool_permute_fwd", dev, B, C, Hin, Win, Ho, Wo, xb.ptr, *st, yb.ptr)
            return (yb.read("y"),)

        def bwd():
            db, xb = GBuf(dev, dy.shape, vals=dy), GBuf(dev, x.shape, st, out=True)
            _call("scnattn_pool_permute_bwd", dev, B, C, Hin, Win, Ho, Wo, db.ptr, xb.ptr, *st)
            return (xb.read("dx"),)
        R.judge_pool_fwd("pool_permute_fwd", _twice("pool_permute_fwd", fwd)[0], x, Ho, Wo)
        R.judge_pool_bwd("pool_permute_bwd", _twice("pool_permute_bwd", bwd)[0], dy, Hin, Win)


# ---- f32_to_bf16 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.BF16_NS)
def test_f32_to_bf16(dev, n):
    """ties, subnormals, +-inf, -0 and NaN at both ends; the largest buffer takes the grid-stride loop into its second lap"""
    for seed in range(7 if n == 4 else 1):
        x = R.gen_bf16(n, seed)

        def run():
            xb, ob = GBuf(dev, (n,), vals=x), GBuf16(dev, 1, n)
            _call("scnattn_f32_to_bf16", dev, n, xb.ptr, ob.ptr)
            return (ob.read("out").reshape(-1),)
        R.judge_bf16("f32_to_bf16", _twice("f32_to_bf16", run)[0], x)


def test_f32_to_bf16_refusals_leave_the_output_untouched(dev):
    from scnattn import _lib as L
    h = L.lib()
    x = R.gen_bf16(1028)
    ok, off = GBuf(dev, (1028,), vals=x), GBuf(dev, (1028,), vals=x, mis=1)
    out = GBuf16(dev, 1, 1028)
    refused = [
        h.scnattn_f32_to_bf16(None, 1026, ok.ptr, out.ptr),              # n % 4 != 0
        h.scnattn_f32_to_bf16(None, 1024, off.ptr, out.ptr),             # the input 4 bytes off the 16-byte grid
        h.scnattn_f32_to_bf16(None, 1024, ok.ptr, out.ptr + 2),          # the output 2 bytes off the 8-byte grid
        h.scnattn_f32_to_bf16(None, 1024, None, out.ptr),
        h.scnattn_f32_to_bf16(None, 1024, ok.ptr, None),
    ]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert b"invalid argument" in h.scnattn_last_error()
    assert out.untouched()
