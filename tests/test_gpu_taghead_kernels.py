"""GPU tests (``-m gpu``) of the tagger head kernels through the C ABI, each entry point alone: scnattn_tag_pool_fwd,
scnattn_tag_pool_bwd, scnattn_bce_fwd, scnattn_bce_bwd (csrc/taghead.hip), judged per element against fp64 with the bounds of
tests/taghead_refs.py.

Buffers are guarded windows (tests/kernel_harness.py GBuf / GBuf16): NaN around every input and in the gaps its strides
leave, the sentinel around and inside every output, which must survive; every leading dimension is wider than its row.  The
maps run channel-contiguous (the vector form when the base is aligned) and batch-major planar (sp = 1: the scalar form), with
the base on and one element off 16 bytes, with the keep mask and without, as fp32 and as bf16.  Every case runs twice and must
give the same bits (fixed summation order).  Every refusal returns -1 and leaves the outputs as the sentinel.

The worst err / bound per kernel and result goes to the run's parity report; profiles/parity_report_taghead_kernels.txt keeps
a copy."""
import functools

import pytest
import torch

import taghead_refs as R
from kernel_harness import GBuf, GBuf16, SENT, _call, _write_report      # noqa: F401  (_write_report: the report fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT_TITLE = ("tagger head kernels vs fp64: worst |got - ref| / bound over all cases; pooled (HW+8) 2^-24 |ks| sum|x|/HW, dx 8 2^-24 |ref| "
                "(bf16: b + 2^-8 (|ref| + b)), rows (S+8) 2^-24 sum|terms| at the stored p, loss (B+8) 2^-24 sum|row|/(B S), dz 8 2^-24 |ref|")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _pool(shape, bf16, with_ks):
    return R.gen_pool(*shape, bf16, with_ks)


@functools.lru_cache(maxsize=None)
def _bce(shape):
    return R.gen_bce(*shape)


def _shift16(buf):
    """move a GBuf16 window one element up: its base is then 2 bytes off the 16-byte grid"""
    host = buf.flat.cpu()
    buf.flat = torch.cat([host[:1], host]).to(buf.flat.device)
    buf.pos, buf.base = buf.pos + 1, buf.base + 1
    buf.ptr = buf.flat.data_ptr() + 2 * buf.base
    return buf


class _Map:
    """the map x[b, q, c] as a guarded window: fp32 (GBuf, any strides) or bf16 (GBuf16: [B*HW][C] or planar [B*C][HW])"""

    def __init__(self, dev, shape, bf16, planar, mis, vals=None):
        B, HW, C = shape
        self.shape, self.bf16, self.planar = shape, bf16, planar
        pad = (8 if bf16 else 4) if not planar else 3
        if planar:
            ld = HW + pad
            self.strides = (C * ld + (0 if bf16 else 5), 1, ld)              # (sb, sp, sc)
        else:
            ld = C + pad
            self.strides = (HW * ld + (0 if bf16 else 2 * pad), ld, 1)
        if bf16:
            v = None if vals is None else (vals.permute(0, 2, 1).reshape(B * C, HW) if planar else vals.reshape(B * HW, C)).to(BF)
            self.buf = GBuf16(dev, B * C if planar else B * HW, HW if planar else C, ld=ld, vals=v)
            if mis:
                _shift16(self.buf)
            self.ptr = self.buf.ptr
        else:
            sb, sp, sc = self.strides
            self.buf = GBuf(dev, shape, (sb, sp, sc), vals=vals, out=vals is None, mis=mis)
            self.ptr = self.buf.ptr

    def read(self, what):
        B, HW, C = self.shape
        got = self.buf.read(what)
        if not self.bf16:
            return got
        got = got.float()
        return got.view(B, C, HW).permute(0, 2, 1).contiguous() if self.planar else got.view(B, HW, C)


_FORMS = [(planar, mis, with_ks) for planar in (False, True) for mis in (0, 1) for with_ks in (True, False)]


def _form(C, bf16, planar, mis):
    """which kernel form the launcher picks: 16-byte accesses need channel-contiguous rows of whole vectors on an aligned base"""
    return " vector" if not planar and not mis and C % (8 if bf16 else 4) == 0 else " scalar"


def _mat(dev, vals, pad):
    return None if vals is None else GBuf(dev, vals.shape, (vals.shape[1] + pad, 1), vals=vals)


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tag_pool_fwd(dev, shape, bf16):
    B, HW, C = shape
    for planar, mis, with_ks in _FORMS:
        x, ks, _ = _pool(shape, bf16, with_ks)
        xm = _Map(dev, shape, bf16, planar, mis, vals=x)
        kb = _mat(dev, ks, 5)
        runs = []
        for _ in range(2):
            out = GBuf(dev, (B, C), (C + 3, 1), out=True)
            _call("scnattn_tag_pool_fwd", dev, B, HW, C, xm.ptr, int(bf16), *xm.strides, None if kb is None else kb.ptr, C + 5,
                  out.ptr, C + 3)
            runs.append(out.read("pooled"))
        what = "tag_pool_fwd%s" % ("16" if bf16 else "")
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "%s: two runs differ" % what
        R.judge_pool_fwd(what + _form(C, bf16, planar, mis), runs[0], x, ks)


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tag_pool_fwd_bf16_mean(dev, shape):
    """bf16 = 2: the mean of a bf16 map rounded to bf16 before the mask (what AdaptiveAvgPool2d hands on under bf16 autocast)"""
    B, HW, C = shape
    for planar, mis, with_ks in _FORMS:
        x, ks, _ = _pool(shape, True, with_ks)
        xm = _Map(dev, shape, True, planar, mis, vals=x)
        kb = _mat(dev, ks, 5)
        runs = []
        for _ in range(2):
            out = GBuf(dev, (B, C), (C + 3, 1), out=True)
            _call("scnattn_tag_pool_fwd", dev, B, HW, C, xm.ptr, 2, *xm.strides, None if kb is None else kb.ptr, C + 5, out.ptr, C + 3)
            runs.append(out.read("pooled"))
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "tag_pool_fwd16 r16: two runs differ"
        R.judge_pool_fwd("tag_pool_fwd16 r16" + _form(C, True, planar, mis), runs[0], x, ks, True)


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tag_pool_bwd(dev, shape, bf16):
    B, HW, C = shape
    for planar, mis, with_ks in _FORMS:
        _, ks, dp = _pool(shape, bf16, with_ks)
        kb, db = _mat(dev, ks, 5), _mat(dev, dp, 7)
        runs = []
        for _ in range(2):
            dx = _Map(dev, shape, bf16, planar, mis)
            _call("scnattn_tag_pool_bwd", dev, B, HW, C, db.ptr, C + 7, None if kb is None else kb.ptr, C + 5, dx.ptr, int(bf16),
                  *dx.strides)
            runs.append(dx.read("dx"))
        what = "tag_pool_bwd%s" % ("16" if bf16 else "")
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "%s: two runs differ" % what
        R.judge_pool_bwd(what + _form(C, bf16, planar, mis), runs[0], dp, ks, HW, bf16)


_LDS = ((4, 0), (3, 0), (4, 1))         # (row padding, base offset in floats): vector rows when S % 4 == 0, odd rows, misaligned base


def _bce_fwd(dev, z, t, pad, mis):
    B, S = z.shape
    ld = S + pad
    zb, tb = GBuf(dev, (B, S), (ld, 1), vals=z, mis=mis), GBuf(dev, (B, S), (ld, 1), vals=t, mis=mis)
    pb, rows, out = GBuf(dev, (B, S), (ld, 1), out=True, mis=mis), GBuf(dev, (2, B), out=True), GBuf(dev, (2,), out=True)
    _call("scnattn_bce_fwd", dev, B, S, zb.ptr, ld, tb.ptr, ld, pb.ptr, ld, rows.ptr, out.ptr)
    return pb.read("probs"), rows.read("rows"), out.read("out")


@pytest.mark.parametrize("shape", R.BCE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bce_fwd(dev, shape):
    B, S = shape
    z, t, planted = _bce(shape)
    for pad, mis in _LDS:
        a, b = _bce_fwd(dev, z, t, pad, mis), _bce_fwd(dev, z, t, pad, mis)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "bce_fwd: two runs differ"
        p, rows, out = a
        what = "bce_fwd vector" if (S % 4 == 0 and pad % 4 == 0 and not mis) else "bce_fwd scalar"
        R.judge_probs(what, p, z, planted)
        R.judge_rows(what, rows[0], p, t)
        R.judge_loss(what, out[0], rows[0], B, S)
        R.judge_agree(what, out[1], p, t)
        assert float(rows[1].sum()) == float(out[1])
        if planted:     # the saturated terms contribute exactly 100 or 0: a row of them alone
            zs = torch.tensor([[120.0, 120.0, -120.0, -120.0]])
            ts = torch.tensor([[0.0, 1.0, 0.0, 1.0]])
            ps, rs, os_ = _bce_fwd(dev, zs, ts, pad, mis)
            assert ps.tolist() == [[1.0, 1.0, 0.0, 0.0]] and float(rs[0, 0]) == 200.0 and float(os_[0]) == 50.0
            assert float(os_[1]) == 2.0


@pytest.mark.parametrize("shape", R.BCE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bce_bwd(dev, shape):
    B, S = shape
    z, t, planted = _bce(shape)
    p, _, _ = _bce_fwd(dev, z, t, 4, 0)          # the kernel's own stored probabilities
    for pad, mis in _LDS:
        ld = S + pad
        for g in (1.0, 0.37):
            gb = GBuf(dev, (1,), vals=torch.tensor([g]))
            runs = []
            for _ in range(2):
                pb, tb = GBuf(dev, (B, S), (ld, 1), vals=p, mis=mis), GBuf(dev, (B, S), (ld, 1), vals=t, mis=mis)
                dz = GBuf(dev, (B, S), (ld, 1), out=True, mis=mis)
                _call("scnattn_bce_bwd", dev, B, S, pb.ptr, ld, tb.ptr, ld, gb.ptr, dz.ptr, ld)
                runs.append(dz.read("dz"))
            assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "bce_bwd: two runs differ"
            what = "bce_bwd vector" if (S % 4 == 0 and pad % 4 == 0 and not mis) else "bce_bwd scalar"
            R.judge_bce_bwd(what, runs[0], p, t, float(torch.tensor(g, dtype=torch.float32)), planted)


def test_refusals_leave_the_outputs_untouched(dev):
    from scnattn import _lib as L
    h = L.lib()
    st = None
    B, HW, C, S = 2, 4, 8, 8
    x = GBuf(dev, (B, HW, C), vals=torch.randn(B, HW, C))
    m = GBuf(dev, (B, C), vals=torch.randn(B, C))
    outs = dict(pooled=GBuf(dev, (B, C), out=True), dx=GBuf(dev, (B, HW, C), out=True), dx16=GBuf16(dev, B * HW, C),
                probs=GBuf(dev, (B, S), out=True), rows=GBuf(dev, (2, B), out=True), out=GBuf(dev, (2,), out=True),
                dz=GBuf(dev, (B, S), out=True))
    o = {k: v.ptr for k, v in outs.items()}
    s = (HW * C, C, 1)
    refused = [
        h.scnattn_tag_pool_fwd(st, B, HW, C, None, 0, *s, m.ptr, C, o["pooled"], C),                    # a null pointer
        h.scnattn_tag_pool_fwd(st, B, HW, C, x.ptr, 0, *s, m.ptr, C, o["pooled"], C - 1),               # ld < width
        h.scnattn_tag_pool_fwd(st, B, HW, C, x.ptr, 0, *s, m.ptr, C - 1, o["pooled"], C),
        h.scnattn_tag_pool_fwd(st, 0, HW, C, x.ptr, 0, *s, m.ptr, C, o["pooled"], C),                   # B = 0
        h.scnattn_tag_pool_fwd(st, B, 0, C, x.ptr, 0, *s, m.ptr, C, o["pooled"], C),                    # HW = 0
        h.scnattn_tag_pool_fwd(st, B, HW, C, x.ptr, 3, *s, m.ptr, C, o["pooled"], C),                   # no such map mode
        h.scnattn_tag_pool_bwd(st, B, 0, C, m.ptr, C, None, C, o["dx"], 0, *s),
        h.scnattn_tag_pool_bwd(st, B, HW, C, m.ptr, C - 1, None, C, o["dx"], 0, *s),
        h.scnattn_tag_pool_bwd(st, B, HW, C, None, C, None, C, o["dx16"], 1, *s),
        h.scnattn_tag_pool_bwd(st, B, HW, C, m.ptr, C, None, C, None, 1, *s),                           # the gradient map is null
        h.scnattn_tag_pool_bwd(st, B, HW, C, m.ptr, C, None, C, o["dx16"], 1, HW * C, 0, 1),            # pixels on one address
        h.scnattn_bce_fwd(st, 0, S, m.ptr, S, m.ptr, S, o["probs"], S, o["rows"], o["out"]),
        h.scnattn_bce_fwd(st, B, S, m.ptr, S - 1, m.ptr, S, o["probs"], S, o["rows"], o["out"]),
        h.scnattn_bce_fwd(st, B, S, m.ptr, S, None, S, o["probs"], S, o["rows"], o["out"]),
        h.scnattn_bce_fwd(st, 4097, 4096, m.ptr, 4096, m.ptr, 4096, o["probs"], 4096, o["rows"], o["out"]),   # B * S > 2^24
        h.scnattn_bce_bwd(st, B, S, m.ptr, S, m.ptr, S, m.ptr, None, S),                                # d logits asked for, null
        h.scnattn_bce_bwd(st, B, S, m.ptr, S, m.ptr, S, None, o["dz"], S),
        h.scnattn_bce_bwd(st, B, S, m.ptr, S, m.ptr, S, m.ptr, o["dz"], S - 1),
        h.scnattn_bce_bwd(st, 4097, 4096, m.ptr, 4096, m.ptr, 4096, m.ptr, o["dz"], 4096),
    ]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert b"invalid argument" in h.scnattn_last_error()
    for k, v in outs.items():
        if isinstance(v, GBuf16):
            assert v.untouched(), k
        else:
            assert bool((v.flat.view(torch.int32) == SENT).all()), k
