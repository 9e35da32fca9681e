"""CPU tests of tests/train_tail_refs.py and of the host side of the entry points it covers.

1. The index-arithmetic fp64 references equal torch's own fp64 ops and autograd to 1e-12: F.cross_entropy on
   pack_padded_sequence data plus the doubly-stochastic term, F.adaptive_avg_pool2d(.., (Ho, Wo)).permute(0, 2, 3, 1),
   nn.Embedding forward and backward, clamp_ followed by torch.optim.Adam over three steps, and the one-line torch forms of the
   layout helpers; the bf16 rounding equals tensor.to(torch.bfloat16) bit for bit.
2. The judges exclude nothing a correct fp32 evaluation produces: torch's CPU fp32 evaluation of the same formulas passes
   every judge on every case of the GPU test.  Worst err / bound over all cases, as the test prints them:
       ce_bwd dscores   0.839 at CE_SLACK 0 (the derived bound alone), 0.419 at CE_SLACK 1 (used)
       clamp_adam p     0.998 at ADAM_SLACK 0 (the derived bound alone), 0.499 at ADAM_SLACK 1 (used)
       clamp_adam m 0.480, v 0.478 (no slack: no device function in them)
       dalphas 0.189, sm1 0.080, scatter_add 0.016, colsum_masked 0.118, reduce_slabs 0.099, add_bcast_rows 0.138,
       pool fwd 0.196, pool bwd 0.228; every bit-equal result 0
   Each slack is the smallest whole number of further copies of the derived bound that puts this evaluation at or below 0.5
   (train_tail_refs.py's docstring says why a constant on one term cannot).
3. Each planted defect fails the judge it was planted for.
4. Host logic: the eight new symbols are in the ctypes table and in the header, the library's version stays 109, and each
   entry refuses null operands and bad shapes with -1 before anything is launched (no GPU is needed to see it)."""
import os

import pytest
import torch

import train_tail_refs as R
from kernel_harness import _STATS, U, _note, _sum_ok

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scnattn_gather_rows_tm", "scnattn_scatter_add_rows_tm", "scnattn_hidden_to_bm", "scnattn_hidden_from_bm",
         "scnattn_colsum_masked", "scnattn_reduce_slabs", "scnattn_copy2d", "scnattn_add_bcast_rows")


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), "%s: %.3e" % (what, err)


# ---- 1. references vs torch fp64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (3, 1028))
def test_loss_reference_equals_torch_fp64(V):
    from torch.nn.utils.rnn import pack_padded_sequence
    scores32, targets = R.gen_ce(V)
    alphas32, _ = R.gen_alphas(5)
    scores = torch.nan_to_num(scores32.double(), nan=0.25).requires_grad_(True)      # torch's packing drops those rows anyway
    alphas = alphas32.double().requires_grad_(True)
    lens = list(R.CE_LENS)
    ps = pack_padded_sequence(scores, lens, batch_first=True).data
    pt = pack_padded_sequence(targets[:, :R.CE_T], lens, batch_first=True).data
    loss = torch.nn.functional.cross_entropy(ps, pt) + R.ALPHA_C * ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    (loss * R.GOUT).backward()
    a = R.alpha_reg_ref(alphas32)
    mine = R.ce_fwd_ref(scores32, targets) + R.ALPHA_C * (a["sm1"] ** 2).mean()
    _close(mine, loss.detach(), "loss")
    r = R.ce_bwd_ref(scores32, targets, R.lse64(scores32))
    _close(r["want"], scores.grad, "dscores")
    assert float(scores.grad[1, 2:].abs().max()) == 0.0 and float(r["want"][1, 2:].abs().max()) == 0.0
    _close(R.dalphas_ref(a["sm1"], R.CE_T)["dalphas"], alphas.grad, "dalphas")
    assert float(alphas.grad[2, 3].abs().min()) > 0.0          # every t has a gradient, decoded or not


@pytest.mark.parametrize("size", R.POOL_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_pool_reference_equals_torch_fp64(size):
    Hin, Win, Ho, Wo = size
    x32, dy32 = R.gen_pool2d(5, size)
    x = x32.double().requires_grad_(True)
    y = torch.nn.functional.adaptive_avg_pool2d(x, (Ho, Wo)).permute(0, 2, 3, 1)
    y.backward(dy32.double())
    _close(R.pool_fwd_ref(x32, Ho, Wo)["y"], y.detach(), "y")
    _close(R.pool_bwd_ref(dy32, Hin, Win)["dx"], x.grad, "dx")


def test_embedding_references_equal_torch_fp64():
    caps, table = R.gen_gather(17)
    emb = torch.nn.Embedding(R.GATHER_V, 17).double()
    emb.weight.data.copy_(table.double())
    want = emb(caps[:, :R.GATHER_T].clamp(0, R.GATHER_V - 1)).permute(1, 0, 2).reshape(-1, 17)      # time-major
    assert torch.equal(R.gather_ref(caps, table, R.GATHER_T).double(), want.detach())
    B, T, V, M = R.SCAT_B, R.SCAT_T, R.SCAT_V, 3
    caps, lens, demb, dtable = R.gen_scatter(M, 1025)
    emb = torch.nn.Embedding(V, M).double()
    tok = caps[:, :T]
    live = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)) & (tok >= 0) & (tok < V)
    out = emb(tok.clamp(0, V - 1))                                                    # [B, T, M]
    d = torch.nan_to_num(demb.double().view(T, B, M).permute(1, 0, 2), nan=0.0) * live.unsqueeze(-1)
    out.backward(d)
    r = R.scatter_ref(caps, lens, demb, dtable, T)
    _close(r["want"] - dtable.double(), emb.weight.grad, "dtable")
    assert int(r["n"][R.SCAT_TOKEN]) == 1025 and int(r["n"][R.SCAT_ABSENT]) == 0 and int(r["present"].sum()) == V - 1
    assert bool(((tok == -3) & live.logical_not() & (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1))).any())
    for count in R.SCAT_COUNTS:
        c2, l2, _, _ = R.gen_scatter(3, count)
        act = torch.arange(T).unsqueeze(0) < torch.tensor(l2).unsqueeze(1)
        assert int(((c2[:, :T] == R.SCAT_TOKEN) & act).sum()) == count
        assert bool(((c2[:, :T] == V + 2) & act).any()) and bool(((c2[:, :T] == -3) & act).any())


def test_adam_reference_equals_clamp_and_torch_adam_fp64():
    n, clip, gs = 257, 5.0, 0.25
    p0, _, _, _ = R.gen_adam(n, 0, zero_state=True)
    w = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([w], lr=R.ADAM_LR, betas=(R.ADAM_B1, R.ADAM_B2), eps=R.ADAM_EPS)
    p, m, v = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for k in (1, 2, 3):
        g = R.gen_adam(n, k)[1].double()
        w.grad = g * gs
        w.grad.clamp_(-clip, clip)
        opt.step()
        r = R.adam_ref(p, g, m, v, R.adam_hyper(k, clip, gs, rounded=False))
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[w]
        _close(m, st["exp_avg"], "m at step %d" % k)
        _close(v, st["exp_avg_sq"], "v at step %d" % k)
        _close(p, w.detach(), "p at step %d" % k)
    c = torch.tensor([R.NAN, R.INF, -R.INF, 7.0], dtype=F64).clamp_(-5.0, 5.0)
    assert bool(c[0].isnan()) and c[1:].tolist() == [5.0, -5.0, 5.0]            # what the fused step is held to
    h = R.adam_hyper(1, 5.0, 1.0, rounded=False)
    r = R.adam_ref(torch.ones(4), torch.tensor([R.NAN, R.INF, -R.INF, 7.0]), torch.zeros(4), torch.zeros(4), h)
    assert bool(r["m"][0].isnan() and r["v"][0].isnan() and r["p"][0].isnan()) and bool(r["p"][1:].isfinite().all())


def test_layout_references_equal_torch_fp64():
    for D in (1, 257):
        for to_bm in (True, False):
            src, mask = R.gen_hidden(D, to_bm)
            B, T = R.HID_B, R.HID_T
            act = (torch.arange(T).unsqueeze(0) < torch.tensor(R.HID_LENS).unsqueeze(1)).reshape(B * T, 1)
            for mk in (None, mask):
                out, rowmask = R.hidden_ref(src, mk, to_bm)
                s = src.view(T, B, D).permute(1, 0, 2).reshape(B * T, D) if to_bm else src
                want = torch.where(act, s * (1.0 if mk is None else mk), torch.zeros(()))           # batch-major
                if not to_bm:
                    want = want.view(B, T, D).permute(1, 0, 2).reshape(T * B, D)
                assert torch.equal(out, want) and torch.equal(rowmask, act.float().reshape(-1))
    x, v = torch.randn(2, 7, 130), torch.randn(2, 130)
    _close(R.bcast_ref(x, v)["x"], x.double() + R.BCAST_SCALE * v.double().unsqueeze(1), "add_bcast_rows")
    vals = torch.randn(16, 3, 259)
    _close(R.slabs_ref(vals)["out"], vals.double().sum(0), "reduce_slabs")
    X, mask, old = R.gen_colsum(65, 17)
    want = torch.where(mask.unsqueeze(1) != 0, X, torch.zeros(())).double().sum(0)
    _close(R.colsum_ref(X, mask, old, 65, 0.0)["out"], want, "colsum_masked")
    _close(R.colsum_ref(X, mask, old, 65, 1.5)["out"], want + 1.5 * old.double(), "colsum_masked beta")


def test_bf16_reference_equals_torch():
    for n in R.BF16_NS:
        for seed in range(7 if n == 4 else 1):
            x = R.gen_bf16(n, seed)
            t = x.to(torch.bfloat16)
            R.judge_bf16("torch", t, x)
            keep = ~x.isnan()
            assert torch.equal((t.view(torch.int16).to(torch.int32) & 0xFFFF)[keep], R.bf16_ref_bits(x)[keep])
    _STATS.clear()


# ---- 2. torch CPU fp32 passes every judge -----------------------------------------------------------------------------------
def _cpu_step(p, g, m, v, step, clip, gs):
    return R.cpu32_adam(p, g, m, v, R.adam_hyper(step, clip, gs))


def _worst(prefix, name):
    return max([s[0] for (k, nm), s in _STATS.items() if k.startswith(prefix) and nm == name] + [0.0])


def _measure(kernel, name, got, want, bound, kind="sum"):
    """_bound_ok without the assertion: the worst err / bound goes to the table whatever it is"""
    want, bound = want.double(), bound.double().expand(want.shape)
    err = (got.double().reshape(want.shape) - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    _note(kernel, name, float(ratio.nan_to_num(1e30).max()) if ratio.numel() else 0.0, kind)


def _ce_ratio():
    _STATS.clear()
    for V in R.CE_VS:
        R.walk_ce("cpu32 ce_bwd", V, R.cpu32_ce_bwd)
    return _worst("cpu32 ce_bwd", "dscores")


def _adam_ratios():
    _STATS.clear()
    for n in R.ADAM_NS:
        R.walk_adam("cpu32 clamp_adam", n, _cpu_step)
    return [_worst("cpu32 clamp_adam", k) for k in "pmv"]


def test_cpu_fp32_sizes_the_slacks(monkeypatch):
    """the derived tier over every case of the GPU test: the ratios at slack 0 and at the slacks used; each slack used is the
    smallest whole number at which torch's CPU fp32 evaluation sits at or below 0.5 of the bound"""
    used = R.CE_SLACK, R.ADAM_SLACK
    assert used[0] == int(used[0]) >= 0 and used[1] == int(used[1]) >= 0
    monkeypatch.setattr(R, "_bound_ok", _measure)
    monkeypatch.setattr(R, "CE_SLACK", 0.0)
    ce0 = _ce_ratio()
    if used[0] > 0:
        monkeypatch.setattr(R, "CE_SLACK", used[0] - 1.0)
        assert (ce0 if used[0] == 1 else _ce_ratio()) > 0.5, "a smaller CE_SLACK would do"
    monkeypatch.setattr(R, "CE_SLACK", used[0])
    ce1 = _ce_ratio()
    monkeypatch.setattr(R, "ADAM_SLACK", 0.0)
    ad0, m0, v0 = _adam_ratios()
    ad1 = ad0
    if used[1] > 0:
        monkeypatch.setattr(R, "ADAM_SLACK", used[1] - 1.0)
        assert (ad0 if used[1] == 1 else _adam_ratios()[0]) > 0.5, "a smaller ADAM_SLACK would do"
        monkeypatch.setattr(R, "ADAM_SLACK", used[1])
        ad1 = _adam_ratios()[0]
    _STATS.clear()
    print("ce_bwd dscores: %.3f at CE_SLACK 0, %.3f at CE_SLACK %g (used)" % (ce0, ce1, used[0]))
    print("clamp_adam p: %.3f at ADAM_SLACK 0, %.3f at ADAM_SLACK %g (used); m %.3f, v %.3f" % (ad0, ad1, used[1], m0, v0))
    assert ce1 <= 0.5 and ad1 <= 0.5 and m0 <= 1.0 and v0 <= 1.0


def test_cpu_fp32_passes_the_derived_judges():
    """... and with the assertions on: nothing a correct fp32 evaluation produces is refused"""
    _STATS.clear()
    for V in R.CE_VS:
        R.walk_ce("cpu32 ce_bwd", V, R.cpu32_ce_bwd)
    for n in R.ADAM_NS[:-1]:            # the largest buffer is walked above (a ratio above 1 fails there too)
        R.walk_adam("cpu32 clamp_adam", n, _cpu_step)
    p, g, m, v = R.gen_adam(257, 1)
    g[100] = R.NAN                      # the planted NaN gradient of the GPU test
    for gs in R.ADAM_GSCALES:
        h = R.adam_hyper(1, 5.0, gs)
        p2, m2, v2 = R.cpu32_adam(p, g, m, v, h)
        R.judge_adam("cpu32 clamp_adam nan", p2, m2, v2, p, g, m, v, h)
        assert bool(p2[100].isnan() and m2[100].isnan() and v2[100].isnan()) and int(p2.isnan().sum()) == 1
    _STATS.clear()


def test_cpu_fp32_passes_every_other_judge():
    _STATS.clear()
    for P in R.CE_PS[1:]:
        alphas, sm1 = R.gen_alphas(P)
        _sum_ok("cpu32 alpha_reg_bwd", "dalphas", R.cpu32_dalphas(sm1, R.CE_T), R.dalphas_ref(sm1, R.CE_T))
        _sum_ok("cpu32 alpha_reg_fwd", "sm1", alphas.sum(dim=1) - 1.0, R.alpha_reg_ref(alphas))
    for M in R.SCAT_MS:
        for count in R.SCAT_COUNTS:
            caps, lens, demb, dtable = R.gen_scatter(M, count)
            R.judge_scatter("cpu32 scatter_add", R.cpu32_scatter(caps, lens, demb, dtable, R.SCAT_T), None, caps, lens, demb,
                            dtable, R.SCAT_T)
    for R_ in R.COLSUM_RS:
        for N in R.COLSUM_NS:
            X, mask, old = R.gen_colsum(R_, N)
            for beta in R.COLSUM_BETAS:
                got = torch.where(mask.unsqueeze(1) != 0, X, torch.zeros(()))[:R_].sum(0) + (beta * old if beta else 0.0)
                _sum_ok("cpu32 colsum_masked", "out", got, R.colsum_ref(X, mask, old, R_, beta))
    for n in R.SLAB_NS:
        for W in R.SLAB_WS:
            vals = R.gen_slabs(n, W)
            _sum_ok("cpu32 reduce_slabs", "out", vals.sum(0), R.slabs_ref(vals))
    for P in R.BCAST_PS:
        for E in R.BCAST_ES:
            x, v = R.gen_bcast(P, E)
            _sum_ok("cpu32 add_bcast_rows", "x", x + torch.tensor(R.BCAST_SCALE) * v.unsqueeze(1), R.bcast_ref(x, v))
    for size in R.POOL_SIZES:
        for C in R.POOL_CS:
            x, dy = R.gen_pool2d(C, size)
            xg = x.clone().requires_grad_(True)
            y = torch.nn.functional.adaptive_avg_pool2d(xg, size[2:]).permute(0, 2, 3, 1)
            y.backward(dy)
            R.judge_pool_fwd("cpu32 pool_fwd", y.detach(), x, *size[2:])
            R.judge_pool_bwd("cpu32 pool_bwd", xg.grad, dy, *size[:2])
    for (kern, name), (ratio, _, _, n) in sorted(_STATS.items()):
        print("%-22s %-8s worst err/bound %.3f over %d cases" % (kern, name, ratio, n))
        assert ratio <= 1.0
    _STATS.clear()


# ---- 3. planted defects -------------------------------------------------------------------------------------------------
def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn("defect", *a)
    _STATS.clear()


def test_planted_loss_defects_fail():
    for V in (1023, 2051):                                  # V % 4 == 3
        scores, targets = R.gen_ce(V)
        lse = R.lse64(scores).float()
        good = R.cpu32_ce_bwd(scores, targets, lse)
        R.judge_ce_bwd("ok", good, scores, targets, lse)
        stale = good.clone()
        stale[0, 0, V - (V % 4):] = 0.0                     # the last V % 4 elements of one row never written
        _fails(R.judge_ce_bwd, stale, scores, targets, lse)
        off = good.clone()                                  # the one-hot one index off, in one row
        tg = int(targets[1, 1])
        g = R.GOUT / len(R.ce_cells())
        off[1, 1, tg] += g
        off[1, 1, tg - 1] -= g
        _fails(R.judge_ce_bwd, off, scores, targets, lse)
        _fails(R.judge_ce_bwd, R.ce_bwd_ref(scores, targets, lse, n_rows=R.CE_B * R.CE_T)["want"].float(), scores, targets, lse)
        leak = good.clone()
        leak[2, 3, 0] = 1e-30                               # an undecoded row that is not exactly 0
        _fails(R.judge_ce_bwd, leak, scores, targets, lse)
        scores, targets = R.gen_ce(V, 2 ** 32 + 3)          # the label narrowed to 32 bits: a one-hot at 3
        narrowed = targets.clone()
        narrowed[0, 2] = 3
        _fails(R.judge_ce_bwd, R.cpu32_ce_bwd(scores, narrowed, lse), scores, targets, lse)
    _, sm1 = R.gen_alphas(5)
    good = R.cpu32_dalphas(sm1, R.CE_T)
    _sum_ok("ok", "dalphas", good, R.dalphas_ref(sm1, R.CE_T))
    cut = good.clone()
    for b, n in enumerate(R.CE_LENS):
        cut[b, n:] = 0.0                                    # d alphas zeroed for t >= decode_length
    with pytest.raises(AssertionError):
        _sum_ok("defect", "dalphas", cut, R.dalphas_ref(sm1, R.CE_T))
    _STATS.clear()


def _adam_defect(n, step, clip, gs, defect, nan_at=None):
    p, g, m, v = R.gen_adam(n, step)
    if nan_at is not None:
        g[nan_at] = R.NAN
    h = R.adam_hyper(step, clip, gs)
    ok = R.cpu32_adam(p, g, m, v, h)
    R.judge_adam("ok", *ok, p, g, m, v, h)
    bad = R.cpu32_adam(p, g, m, v, h, defect)
    return bad, (p, g, m, v, h)


def test_planted_adam_defects_fail():
    bad, case = _adam_defect(257, 2, 5.0, 1.0, "sqrt_outside")             # sqrt(v) / bc2 for sqrt(v / bc2)
    R.judge_nonfinite("ok", "m", bad[1], R.adam_ref(*case)["m"], 4.0 * U * R.adam_ref(*case)["m_abs"] + R.TINY, "=m")
    _fails(R.judge_adam, *bad, *case)                                      # m and v are right: p's judge refuses it
    bad, case = _adam_defect(257, 2, 5.0, 0.25, "clamp_first")             # the clamp applied before gscale
    with pytest.raises(AssertionError):
        R.judge_nonfinite("defect", "m", bad[1], R.adam_ref(*case)["m"], 4.0 * U * R.adam_ref(*case)["m_abs"] + R.TINY, "=m")
    bad, case = _adam_defect(R.ADAM_NS[-1], 2, 5.0, 1.0, "skip_tail")      # the elements past 4096 x 256 skipped
    with pytest.raises(AssertionError):
        R.judge_nonfinite("defect", "m", bad[1], R.adam_ref(*case)["m"], 4.0 * U * R.adam_ref(*case)["m_abs"] + R.TINY, "=m")
    bad, case = _adam_defect(257, 2, 5.0, 1.0, "nan_to_clip", nan_at=100)  # maxNum semantics: a NaN gradient becomes -clip
    with pytest.raises(AssertionError, match="non-finite expectations"):
        R.judge_adam("defect", *bad, *case)
    _STATS.clear()


def test_planted_layout_defects_fail():
    x, _ = R.gen_pool2d(70, (8, 8, 14, 14))
    R.judge_pool_fwd("ok", R.pool_fwd_ref(x, 14, 14)["y"].float(), x, 14, 14)
    _fails(R.judge_pool_fwd, R.pool_fwd_ref(x, 14, 14, floor_hi=True)["y"].float(), x, 14, 14)     # floor where ceil belongs
    caps, lens, demb, dtable = R.gen_scatter(3, 1025)
    R.judge_scatter("ok", R.cpu32_scatter(caps, lens, demb, dtable, R.SCAT_T), None, caps, lens, demb, dtable, R.SCAT_T)
    _fails(R.judge_scatter, R.scatter_ref(caps, lens, demb, dtable, R.SCAT_T, drop_after=1024)["want"].float(), None, caps,
           lens, demb, dtable, R.SCAT_T)                                                           # the 1025th cell dropped
    X, mask, old = R.gen_colsum(65, 17)
    with pytest.raises(AssertionError):                                                            # mask as a factor: NaN * 0
        _sum_ok("defect", "out", R.colsum_ref(X, mask, old, 65, 0.0, multiply=True)["out"].float(), R.colsum_ref(X, mask, old, 65, 0.0))
    x = R.gen_bf16(1028)
    R.judge_bf16("ok", x.to(torch.bfloat16), x)
    trunc = ((x.view(torch.int32) >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16)           # truncation
    _fails(R.judge_bf16, trunc, x)
    src, mask = R.gen_hidden(257, True)
    out, _ = R.hidden_ref(src, mask, True)
    leak = out.clone()
    leak[R.HID_T + 3, 256] = 1e-30                                                                 # an inactive cell not exactly 0
    _fails(R.judge_bits, "out", leak, out)
    _STATS.clear()


# ---- 4. host logic ----------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_declared_and_the_version_stays():
    from scnattn import _lib as L
    h = L.lib()
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    for name in NAMES:
        assert name in L._SIGS and name in L.EXPORTS and hasattr(h, name)
        assert "int %s(void* stream" % name in header
    assert h.scnattn_version() == 109       # new symbols only: they did not bump the version
    assert "#define SCNATTN_VERSION 109" in header


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error(), h.scnattn_last_error()


def test_entry_points_refuse_before_launching():
    from scnattn import _lib as L
    h = L.lib()

    def ga(B=2, T=3, L_=4, M=5, caps=_P, table=_P, V=7, out=_P):
        return h.scnattn_gather_rows_tm(None, B, T, L_, M, caps, table, V, out)

    def sc(B=2, T=3, L_=4, M=5, caps=_P, dl=_P, demb=_P, V=7, dtable=_P, present=_P):
        return h.scnattn_scatter_add_rows_tm(None, B, T, L_, M, caps, dl, demb, V, dtable, present)

    def hb(B=2, T=3, D=5, dl=_P, hs=_P, out=_P):
        return h.scnattn_hidden_to_bm(None, B, T, D, dl, hs, None, out, None)

    def hf(B=2, T=3, D=5, dl=_P, dbm=_P, out=_P):
        return h.scnattn_hidden_from_bm(None, B, T, D, dl, dbm, None, out)

    def cs(R_=4, N=5, X=_P, ld=5, mask=_P, out=_P):
        return h.scnattn_colsum_masked(None, R_, N, X, ld, mask, out, 0.0)

    def rs(rows=3, N=5, slabs=_P, n=2, stride=64, ld=5, out=_P):
        return h.scnattn_reduce_slabs(None, rows, N, slabs, n, stride, ld, out)

    def cp(R_=3, C_=5, src=_P, ldi=5, out=_P, ldo=5):
        return h.scnattn_copy2d(None, R_, C_, src, ldi, out, ldo)

    def ab(B=2, P=3, E=5, v=_P, x=_P):
        return h.scnattn_add_bcast_rows(None, B, P, E, v, 1.0, x)

    _refused(h, ga(caps=None), b"gather_rows_tm: null operand")
    _refused(h, ga(table=None), b"gather_rows_tm: null operand")
    _refused(h, ga(out=None), b"gather_rows_tm: null operand")
    _refused(h, ga(T=5), b"gather_rows_tm: bad shape")                   # T > L
    _refused(h, ga(V=0), b"gather_rows_tm: bad shape")
    _refused(h, ga(M=-1), b"gather_rows_tm: bad shape")
    _refused(h, ga(B=-1), b"gather_rows_tm: bad shape")
    _refused(h, sc(caps=None), b"scatter_add_rows_tm: null operand")
    _refused(h, sc(dl=None), b"scatter_add_rows_tm: null operand")
    _refused(h, sc(demb=None), b"scatter_add_rows_tm: null operand")
    _refused(h, sc(dtable=None), b"scatter_add_rows_tm: null operand")
    _refused(h, sc(present=None), b"scatter_add_rows_tm: null operand")
    _refused(h, sc(T=5), b"scatter_add_rows_tm: bad shape")
    _refused(h, sc(V=0), b"scatter_add_rows_tm: bad shape")
    _refused(h, sc(M=-1), b"scatter_add_rows_tm: bad shape")
    _refused(h, hb(dl=None), b"hidden_to_bm: null operand")
    _refused(h, hb(hs=None), b"hidden_to_bm: null operand")
    _refused(h, hb(out=None), b"hidden_to_bm: null operand")
    _refused(h, hb(D=-1), b"hidden_to_bm: bad shape")
    _refused(h, hf(dl=None), b"hidden_from_bm: null operand")
    _refused(h, hf(dbm=None), b"hidden_from_bm: null operand")
    _refused(h, hf(out=None), b"hidden_from_bm: null operand")
    _refused(h, hf(T=-1), b"hidden_from_bm: bad shape")
    _refused(h, cs(X=None), b"colsum_masked: null operand")
    _refused(h, cs(mask=None), b"colsum_masked: null operand")
    _refused(h, cs(out=None), b"colsum_masked: null operand")
    _refused(h, cs(ld=4), b"colsum_masked: bad shape")                   # ld < N
    _refused(h, cs(R_=-1), b"colsum_masked: bad shape")
    _refused(h, rs(slabs=None), b"reduce_slabs: null operand")
    _refused(h, rs(out=None), b"reduce_slabs: null operand")
    _refused(h, rs(n=0), b"reduce_slabs: bad shape")
    _refused(h, rs(n=17), b"reduce_slabs: bad shape")                    # the fixed-order sum holds 16 slabs at the most
    _refused(h, rs(ld=4), b"reduce_slabs: bad shape")
    _refused(h, cp(src=None), b"copy2d: null operand")
    _refused(h, cp(out=None), b"copy2d: null operand")
    _refused(h, cp(ldi=4), b"copy2d: bad shape")
    _refused(h, cp(ldo=4), b"copy2d: bad shape")
    _refused(h, cp(R_=-1), b"copy2d: bad shape")
    _refused(h, ab(v=None), b"add_bcast_rows: null operand")
    _refused(h, ab(x=None), b"add_bcast_rows: null operand")
    _refused(h, ab(P=0), b"add_bcast_rows: bad shape")
    _refused(h, ab(E=-1), b"add_bcast_rows: bad shape")
    # an empty problem is no error and launches nothing
    assert ga(B=0) == 0 and sc(T=0) == 0 and hb(B=0) == 0 and hf(T=0) == 0 and cs(N=0, ld=0) == 0 and rs(rows=0) == 0
    assert cp(R_=0) == 0 and ab(B=0) == 0
