"""GPU tests (``-m gpu``) of the tagger loss family through the C ABI: scnattn_tagloss_fwd and scnattn_tagloss_bwd
(csrc/taghead.hip), judged against fp64 with the references, yardsticks and bounds of tests/tagloss_refs.py.

Every case (shape x setting) runs on guarded windows (tests/kernel_harness.py GBuf: NaN around every input and in the padding
of its rows, the NaN sentinel around and between the rows of every output, which must survive) in these layouts: rows padded
by 4 on an aligned base (16-byte accesses when S % 4 == 0), rows padded by 3 (the scalar form), an aligned pitch on a base one
float off the grid, and for the weighted settings pos_weight one float off the grid (its own alignment check).  (4, 40) with a
pitch of 43 is the scalar form on a width that would allow vectors.  Every call runs twice and must give the same bits;
probs and the agreement count must be the bits scnattn_bce_fwd writes for the same logits and targets.  Every refusal returns
-1 and leaves the outputs as the sentinel.

The yardstick (worst element error of the fp32 CPU evaluation) and the kernel's own worst error go to the run's parity
report per case (a table of its own, after the worst err / bound per kernel); profiles/parity_report_tagloss_kernels.txt keeps
a copy."""
import ctypes as C
import functools

import pytest
import torch

import taghead_refs as T
import tagloss_refs as R
from kernel_harness import GBuf, SENT, _call, _write_report      # noqa: F401  (_write_report: the report fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = ("tagger loss kernels vs fp64: worst |got - ref| / bound over all cases; rows ((S+8) 2^-24 + 4 yard) sum|parts|, "
                "loss (B+8) 2^-24 sum|row|/(B S), dz 4 yard |g|/(B S) (|t w dL+| + |(1-t) dL-|), yard = CPU-fp32 worst element error")
_IDS = [R.setting_id(s) for s in R.SETTINGS]
_SHAPES = R.SHAPES + ((4, 40),)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _measured_report():
    R.MEASURED.clear()
    yield
    if not R.MEASURED:
        return
    from test_gpu_parity import _report
    lines = ["%-22s %-6s %-34s %-12s %-12s %s" % ("kernel", "result", "case", "yardstick", "kernel", "kernel/yard")]
    for kern, name, case, yard, got in R.MEASURED:
        lines.append("%-22s %-6s %-34s %-12.3e %-12.3e %.2f" % (kern, name, case, yard, got, got / yard if yard > 0 else 0.0))
    _report(lines, "tagger loss kernels: per case the yardstick (worst element error of the fp32 CPU evaluation against fp64, relative "
                   "to |t w L+| + |(1-t) L-| or its derivative's) and the kernel's worst error in the same measure (rows: the worst row "
                   "error over the row's sum of parts); a kernel is allowed 4 x the yardstick per element")
    R.MEASURED.clear()


@functools.lru_cache(maxsize=None)
def _case(shape, weights):
    return R.gen(*shape, weights)


def _layouts(shape, weights):
    """(row padding, base offset of the matrices, base offset of pos_weight)"""
    if shape == (4, 40):
        return ((3, 0, 0),)
    lay = [(4, 0, 0), (3, 0, 0), (4, 1, 0)]
    if weights and shape[1] % 4 == 0:
        lay.append((4, 0, 1))
    return tuple(lay)


def _form(S, pad, mis, wmis):
    return " vector" if (S % 4 == 0 and pad % 4 == 0 and not mis and not wmis) else " scalar"


def _opts(gp, gn, m):
    from scnattn._lib import TagLossOpts
    return C.byref(TagLossOpts(gp, gn, m))


def _wbuf(dev, w, wmis):
    return None if w is None else GBuf(dev, w.shape, vals=w, mis=wmis)


def _fwd(dev, z, t, w, setting, pad, mis, wmis, name="scnattn_tagloss_fwd"):
    B, S = z.shape
    ld = S + pad
    zb, tb = GBuf(dev, (B, S), (ld, 1), vals=z, mis=mis), GBuf(dev, (B, S), (ld, 1), vals=t, mis=mis)
    pb, rows, out = GBuf(dev, (B, S), (ld, 1), out=True, mis=mis), GBuf(dev, (2, B), out=True), GBuf(dev, (2,), out=True)
    if name == "scnattn_bce_fwd":
        _call(name, dev, B, S, zb.ptr, ld, tb.ptr, ld, pb.ptr, ld, rows.ptr, out.ptr)
    else:
        wb = _wbuf(dev, w, wmis)
        _call(name, dev, B, S, zb.ptr, ld, tb.ptr, ld, None if wb is None else wb.ptr, _opts(*setting[:3]), pb.ptr, ld,
              rows.ptr, out.ptr)
    return pb.read("probs"), rows.read("rows"), out.read("out")


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("setting", R.SETTINGS, ids=_IDS)
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tagloss_fwd(dev, shape, setting):
    B, S = shape
    gp, gn, m, weights = setting
    z, t, w, planted = _case(shape, weights)
    for pad, mis, wmis in _layouts(shape, weights):
        a, b = _fwd(dev, z, t, w, setting, pad, mis, wmis), _fwd(dev, z, t, w, setting, pad, mis, wmis)
        for u, v in zip(a, b):
            assert torch.equal(_bits(u), _bits(v)), "tagloss_fwd: two runs differ"
        p, rows, out = a
        p0, rows0, out0 = _fwd(dev, z, t, w, setting, pad, mis, wmis, name="scnattn_bce_fwd")
        assert torch.equal(_bits(p), _bits(p0)), "probs are not the bits of scnattn_bce_fwd"
        assert torch.equal(_bits(rows[1]), _bits(rows0[1])) and torch.equal(_bits(out[1]), _bits(out0[1])), "agree differs"
        what = "tagloss_fwd" + _form(S, pad, mis, wmis)
        case = "%dx%d %s pad%d mis%d%d" % (B, S, R.setting_id(setting), pad, mis, wmis)
        R.judge_rows(what, rows[0], z, t, w, gp, gn, m, case)
        R.judge_loss(what, out[0], rows[0], B, S)
        T.judge_agree(what, out[1], p, t)
        if planted and m == 0.0:       # nothing is clamped at -100: a row of saturated logits alone
            zs, ts = torch.tensor([[120.0, 120.0, -120.0, -120.0]]), torch.tensor([[0.0, 1.0, 0.0, 1.0]])
            ws = None if w is None else torch.tensor([1.0, 1.0, 1.0, 2.5])
            ps, rs, os_ = _fwd(dev, zs, ts, ws, setting, pad, mis, 0)
            assert ps.tolist() == [[1.0, 1.0, 0.0, 0.0]] and float(os_[1]) == 2.0
            assert float(rs[0, 0]) == 120.0 + 120.0 * (1.0 if w is None else 2.5)


@pytest.mark.parametrize("setting", R.SETTINGS, ids=_IDS)
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tagloss_bwd(dev, shape, setting):
    B, S = shape
    gp, gn, m, weights = setting
    z, t, w, planted = _case(shape, weights)
    gb = GBuf(dev, (1,), vals=torch.tensor([R.G]))
    g32 = R.f32(R.G)
    for pad, mis, wmis in _layouts(shape, weights):
        ld = S + pad
        runs = []
        for _ in range(2):
            zb, tb = GBuf(dev, (B, S), (ld, 1), vals=z, mis=mis), GBuf(dev, (B, S), (ld, 1), vals=t, mis=mis)
            wb = _wbuf(dev, w, wmis)
            dz = GBuf(dev, (B, S), (ld, 1), out=True, mis=mis)
            _call("scnattn_tagloss_bwd", dev, B, S, zb.ptr, ld, tb.ptr, ld, None if wb is None else wb.ptr, _opts(gp, gn, m),
                  gb.ptr, dz.ptr, ld)
            runs.append(dz.read("dz"))
        assert torch.equal(_bits(runs[0]), _bits(runs[1])), "tagloss_bwd: two runs differ"
        case = "%dx%d %s pad%d mis%d%d" % (B, S, R.setting_id(setting), pad, mis, wmis)
        R.judge_dz("tagloss_bwd" + _form(S, pad, mis, wmis), runs[0], z, t, w, gp, gn, m, g32, planted, case)


def test_identity_setting_trains_where_bce_saturates(dev):
    """(1, 0, 0, 0): the loss of BCELoss away from its clamp, and a gradient where the BCE pair has none"""
    z = torch.tensor([[-120.0, 120.0, 30.0, -30.0, 2.0, -1.0, 0.0, 0.5]])
    t = torch.tensor([[1.0, 0.0, 1.0, 0.0, 1.0, 0.3, 1.0, 0.0]])
    gb = GBuf(dev, (1,), vals=torch.tensor([1.0]))
    zb, tb, dz = GBuf(dev, (1, 8), vals=z), GBuf(dev, (1, 8), vals=t), GBuf(dev, (1, 8), out=True)
    _call("scnattn_tagloss_bwd", dev, 1, 8, zb.ptr, 8, tb.ptr, 8, None, _opts(0.0, 0.0, 0.0), gb.ptr, dz.ptr, 8)
    got = dz.read("dz")
    assert got[0, :2].tolist() == [-0.125, 0.125]
    want = R.bwd_ref(z, t, None, 0.0, 0.0, 0.0, 1.0)["dz"]
    assert float((got.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    p, _, _ = _fwd(dev, z, t, None, None, 0, 0, 0, name="scnattn_bce_fwd")
    pb, d0 = GBuf(dev, (1, 8), vals=p), GBuf(dev, (1, 8), out=True)
    _call("scnattn_bce_bwd", dev, 1, 8, pb.ptr, 8, tb.ptr, 8, gb.ptr, d0.ptr, 8)
    assert d0.read("dz")[0, :2].tolist() == [0.0, 0.0]


def test_refusals_leave_the_outputs_untouched(dev):
    from scnattn import _lib as L
    h = L.lib()
    B, S = 2, 8
    m = GBuf(dev, (B, S), vals=torch.randn(B, S))
    outs = dict(probs=GBuf(dev, (B, S), out=True), rows=GBuf(dev, (2, B), out=True), out=GBuf(dev, (2,), out=True),
                dz=GBuf(dev, (B, S), out=True))
    o = {k: v.ptr for k, v in outs.items()}
    ok = _opts(0.0, 4.0, 0.05)

    def fw(B_=B, S_=S, z=m.ptr, ldz=S, t=m.ptr, ldt=S, w=None, op=ok, p=o["probs"], ldp=S, rows=o["rows"], out=o["out"]):
        return h.scnattn_tagloss_fwd(None, B_, S_, z, ldz, t, ldt, w, op, p, ldp, rows, out)

    def bw(B_=B, S_=S, z=m.ptr, ldz=S, t=m.ptr, ldt=S, w=None, op=ok, g=m.ptr, dz=o["dz"], lddz=S):
        return h.scnattn_tagloss_bwd(None, B_, S_, z, ldz, t, ldt, w, op, g, dz, lddz)

    bad = [_opts(-1.0, 0.0, 0.0), _opts(0.0, 16.5, 0.0), _opts(float("nan"), 0.0, 0.0), _opts(0.0, float("inf"), 0.0),
           _opts(0.0, 0.0, 1.0), _opts(0.0, 0.0, -0.1), _opts(0.0, 0.0, float("nan")), _opts(0.0, 0.5, 0.05),
           C.POINTER(L.TagLossOpts)()]
    refused = [f(op=b) for b in bad for f in (fw, bw)]
    refused += [fw(B_=0), fw(S_=0), fw(z=None), fw(t=None), fw(p=None), fw(rows=None), fw(out=None), fw(ldz=S - 1),
                fw(ldt=S - 1), fw(ldp=S - 1), fw(B_=4097, S_=4096, ldz=4096, ldt=4096, ldp=4096),
                bw(B_=0), bw(S_=0), bw(z=None), bw(t=None), bw(g=None), bw(dz=None), bw(ldz=S - 1), bw(ldt=S - 1),
                bw(lddz=S - 1), bw(B_=4097, S_=4096, ldz=4096, ldt=4096, lddz=4096)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert b"invalid argument" in h.scnattn_last_error()
    for k, v in outs.items():
        assert bool((v.flat.view(torch.int32) == SENT).all()), k
