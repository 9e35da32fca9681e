"""GPU tests (``-m gpu``) of the eval BatchNorm epilogue on bf16 maps: scnattn_conv1x1_fwd_bn_eval16 and
scnattn_conv3x3_fwd_bn_eval16 through the C ABI (csrc/cgemm16.hip EPI 3, the eval creduce16_kernel), every case of
tests/eval16_refs.py judged per element against fp64 with the derived bound stated there.

Buffers are guarded windows in the manner of tests/kernel_harness.py, in bf16 (GBuf16): NaN around every input (the
residual has ldres = Cout + 8, so NaN sits between its rows too), a NaN-pattern sentinel around the output, which must
survive.  The two entries write dense rows (ldc = Cout), so there is no [Cout, ldc) gap in y to watch; the gap of the
residual rows is where a column-range mistake of the epilogue would read.  Every case runs twice and must give the same
bits (split sums are taken in slab order).  The refusals leave y as the sentinel.

Which instance a case reaches is asked of the library: `_launch` on the CPU device sends the same call through
scnattn_plan_next (kernel_harness._call) and eval16_refs.describe reads the plan.
The worst err / bound per kernel instance goes to the run's parity report (test_gpu_parity._report);
profiles/parity_report_eval16_kernels.txt keeps a copy."""
import ctypes as C

import pytest
import torch

import eval16_refs as E
from kernel_harness import CPU, GBuf16, SENT16, _call  # noqa: F401

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_WORST = {}             # instance name -> [worst err/bound, cases]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    """fp32 split-K workspace of WS_FLOATS with a sentinel tail that must survive the module"""
    t = torch.full((E.WS_FLOATS + 64,), float("nan"), device=dev)
    t[E.WS_FLOATS:] = 12345.0
    yield t
    assert bool((t[E.WS_FLOATS:] == 12345.0).all()), "a split product wrote past the workspace it was given"


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    _WORST.clear()
    yield
    if not _WORST:
        return
    from test_gpu_parity import _report
    _report(["%-74s %-9s %s" % ("instance", "err/bound", "cases")] + ["%-74s %-9.3f %d" % (k, r, n) for k, (r, n) in sorted(_WORST.items())],
            "bf16 eval BatchNorm epilogue vs fp64: worst |got - ref| / bound per instance, bound = b + 2^-8 (|pre| + b), "
            "b = (n+16) 2^-24 mag")


def _inst_name(c, d):
    mi, epi, gather, c3 = d["inst"]
    s = "cgemm16<MI %d, EPI %d, %s, bf16, C3 %d>" % (mi, epi, "gather" if gather else "plain", c3)
    return s + (" + creduce16<eval> (%s S=%d)" % ("forced" if d["forced"] else "policy", d["S"]) if d["S"] > 1 else "")


def _launch(c, I, dev, ws, y=None, wsf=E.WS_FLOATS):
    """the case's call -> the output window; on the CPU device nothing runs: -> the launch plan of the same call"""
    from scnattn import _lib as L
    rows_in = I["x"].shape[0]
    xb = GBuf16(dev, rows_in, c.Cin, vals=I["x"])
    taps = I["w"].shape[1]
    wb = GBuf16(dev, c.Cout, taps * c.Cin, vals=I["w"])
    rb = GBuf16(dev, c.R, c.Cout, ld=c.Cout + 8, vals=I["res"]) if I["res"] is not None else None
    y = y or GBuf16(dev, c.R, c.Cout)
    vec = [I[k].to(dev) for k in ("gamma", "beta", "mean", "var")]
    bn = L.BnEval16(gamma=vec[0].data_ptr(), beta=vec[1].data_ptr(), mean=vec[2].data_ptr(), var=vec[3].data_ptr(), eps=c.eps,
                    res=rb.ptr if rb else None, ldres=c.Cout + 8 if rb else 0, relu=1 if c.relu else 0)
    wsp = ws.data_ptr() if wsf else None
    if c.op == "f3":
        ex = L.ConvExtra(force_split=c.split, force_mi=c.mi)
        plan = _call("scnattn_conv3x3_fwd_bn_eval16", dev, c.N, c.Hi, c.Hi, c.Cin, c.Cout, c.s, xb.ptr, wb.ptr, y.ptr, C.byref(bn),
                     C.byref(ex), wsp, wsf)
    else:
        Ho = (c.Hi - 1) // c.s + 1 if c.gather else 0
        ex = L.ConvExtra(stride=c.s, Hi=c.Hi, Wi=c.Hi, Ho=Ho, Wo=Ho, force_split=c.split, force_mi=c.mi)
        plan = _call("scnattn_conv1x1_fwd_bn_eval16", dev, c.R, c.Cin, c.Cout, xb.ptr, wb.ptr, y.ptr, C.byref(bn), C.byref(ex), wsp, wsf)
    return plan if dev.type == "cpu" else y


def dispatch(c, wsf=E.WS_FLOATS):
    """-> eval16_refs.describe of the case, from the launch plan of its own call"""
    return E.describe(c, _launch(c, E.inputs(c), CPU, torch.empty(E.WS_FLOATS + 64), wsf=wsf))


@pytest.mark.parametrize("i", range(len(E.CASES)), ids=[E.case_id(c) for c in E.CASES])
def test_bn_eval16_case_vs_fp64(dev, ws, i):
    c = E.CASES[i]
    I = E.inputs(c, i)
    ref = E.reference(c, I)
    d = dispatch(c)
    got = _launch(c, I, dev, ws).read(E.case_id(c))
    ok, ratio = E.judge(got, ref)
    name = _inst_name(c, d)
    print("%s -> %s: worst err/bound %.3f" % (E.case_id(c), name, ratio))
    w = _WORST.setdefault(name, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1
    assert ok, "%s (%s): worst err/bound %.3f, %d NaN" % (E.case_id(c), name, ratio, int(got.float().isnan().sum()))
    again = _launch(c, I, dev, ws).read(E.case_id(c))
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two runs of %s differ" % E.case_id(c)


def test_refusals_leave_y_untouched(dev, ws):
    from scnattn import _lib as L
    h = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    R, Cin, Cout = 64, 64, 64
    x = torch.zeros(R, Cin, device=dev, dtype=BF)
    w = torch.zeros(Cout, 9 * Cin, device=dev, dtype=BF)
    v = torch.ones(Cout + 4, device=dev)
    res = torch.zeros(R * (Cout + 8) + 8, device=dev, dtype=BF)
    y = GBuf16(dev, R, Cout)

    def bn(**kw):
        d = dict(gamma=v.data_ptr(), beta=v.data_ptr(), mean=v.data_ptr(), var=v.data_ptr(), eps=1e-5, res=None, ldres=0, relu=1)
        d.update(kw)
        return L.BnEval16(**d)

    def f1(b, ex=None, Cin_=Cin, Cout_=Cout, wsf=E.WS_FLOATS):
        return h.scnattn_conv1x1_fwd_bn_eval16(st, R, Cin_, Cout_, x.data_ptr(), w.data_ptr(), y.ptr, None if b is None else C.byref(b),
                                               None if ex is None else C.byref(ex), ws.data_ptr(), wsf)

    def f3(b, ex=None, Cin_=Cin, s=1):
        return h.scnattn_conv3x3_fwd_bn_eval16(st, 1, 8, 8, Cin_, Cout, s, x.data_ptr(), w.data_ptr(), y.ptr, None if b is None else C.byref(b),
                                               None if ex is None else C.byref(ex), ws.data_ptr(), E.WS_FLOATS)

    calls = [
        (lambda: f1(None), b"bn is NULL"), (lambda: f1(bn(), L.ConvExtra(epi=1)), b"geometry only"),
        (lambda: f1(bn(), L.ConvExtra(pro=1)), b"geometry only"),
        (lambda: f1(bn(var=None)), b"non-null and 16-byte aligned"), (lambda: f1(bn(mean=v.data_ptr() + 4)), b"non-null and 16-byte aligned"),
        (lambda: f1(bn(res=res.data_ptr() + 2, ldres=Cout + 8)), b"residual must be"),
        (lambda: f1(bn(res=res.data_ptr(), ldres=Cout + 4)), b"residual must be"),
        (lambda: f1(bn(res=res.data_ptr(), ldres=Cout - 8)), b"residual must be"),
        (lambda: f1(bn(), Cin_=60), b"multiples of 8"), (lambda: f1(bn(), Cout_=60), b"multiples of 8"),
        (lambda: f1(bn(), L.ConvExtra(stride=2)), b"gather geometry"),
        (lambda: f1(bn(), L.ConvExtra(force_split=2), wsf=16), b"forced split does not fit"),
        (lambda: f3(None), b"bn is NULL"), (lambda: f3(bn(), L.ConvExtra(epi=3)), b"geometry only"),
        (lambda: f3(bn(), Cin_=48), b"multiple of 32"), (lambda: f3(bn(), s=3), b"geometry"),
        (lambda: f3(bn(gamma=None)), b"non-null and 16-byte aligned"),
    ]
    for call, text in calls:
        assert call() == -1
        msg = h.scnattn_last_error()
        assert text in msg, msg
    torch.cuda.synchronize()
    assert y.untouched(), "a refused call wrote to y"
