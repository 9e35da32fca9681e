"""GPU tests (``-m gpu``) of the bf16 TRAINING convolution kernels through the C ABI: scnattn_cgemm16 (EPI 0 / 1 / 2, plain and
gathered, bf16 and fp32 output, beta, split through creduce16), scnattn_conv3x3_fwd16, scnattn_conv3x3_dgrad16 (stride 1 with
the mask epilogue, stride 2 by parity classes), scnattn_wgrad16_3x3, scnattn_wgrad16_rows and scnattn_bf16_weights -- every
case of tests/conv16_refs.py judged per element against fp64 with the bounds derived there (conv16_refs.judge).

Buffers are guarded windows (tests/kernel_harness.py GBuf / GBuf16): NaN around every input and inside its gaps
(scnattn_cgemm16 runs with lda = K + 8, ldb = K + 8, ldz = N + 8), the sentinel around and inside every output and partial
array (ldc = N + 8 for bf16, N + 4 for fp32, ldo = Cin + 4 for scnattn_wgrad16_rows), which must survive -- so must the
slots [row_tiles, stat_ld) of the partials and the tail of the split workspace.  The 3x3 entry points and scnattn_wgrad16_3x3
fix dense rows; their maps are guarded in front and behind.  Every case runs twice and must give the same bits: slab order
and the four-wave meet are fixed.  Every refusal returns -1 and leaves the output window as the sentinel.

The worst err / bound per kernel instance (conv16_refs.names renders it from the launch plan of the case's own call,
scnattn_plan_next on host windows: `_run` on the CPU device) and result goes to the run's parity report;
profiles/parity_report_conv16_kernels.txt keeps a copy."""
import ctypes as C

import pytest
import torch

import conv16_refs as R
import conv_refs as CR
from kernel_harness import CPU, GBuf, GBuf16, SENT, _call

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT_TITLE = ("bf16 training convolution kernels vs fp64: worst |got - ref| / bound per instance; b = (n+8) 2^-24 sum|terms|, "
                "fp32 output: b, bf16 output: b + 2^-8 (|ref| + b), partials: tests/conv16_refs.py")
_WORST = {}             # (instance names, result) -> [worst err/bound, cases]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    """fp32 split workspace of WS_FLOATS with a sentinel tail that must survive the module"""
    t = torch.full((R.WS_FLOATS + 64,), float("nan"), device=dev)
    t[R.WS_FLOATS:] = 12345.0
    yield t
    assert bool((t[R.WS_FLOATS:] == 12345.0).all()), "a split product wrote past the workspace it was given"


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    _WORST.clear()
    yield
    if not _WORST:
        return
    from test_gpu_parity import _report
    _report(["%-78s %-7s %-9s %s" % ("instance", "result", "err/bound", "cases")] +
            ["%-78s %-7s %-9.3f %d" % (k[0], k[1], r, n) for k, (r, n) in sorted(_WORST.items())], REPORT_TITLE)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _vec(dev, v):
    return GBuf(dev, v.shape, vals=v)


def _run(c, I, dev, ws, wsf=R.WS_FLOATS):
    """one launch sequence of a case -> dict(out, part) read back through the guard checks; on the CPU device nothing runs:
    -> the launch plan of the same call (kernel_harness._call; the nine launches of a "t" case share one plan)"""
    from scnattn import _lib as L
    cid = R.case_id(c)
    wsp = ws.data_ptr() if wsf else None
    rows, cols = R.out_shape(c)
    keep = []                                   # the guarded inputs stay alive until the synchronize
    part = None
    if c.op in ("w9", "w1"):
        dy = GBuf16(dev, R.rows_out(c), c.Cout, vals=I["dy"])
        x = GBuf16(dev, R.rows_in(c), c.Cin, vals=I["x"])
        if c.op == "w9":
            out = GBuf(dev, (rows, cols), out=True)
            plan = _call("scnattn_wgrad16_3x3", dev, c.N, c.Hi, c.Wi, c.Cin, c.Cout, dy.ptr, x.ptr, out.ptr, wsp, wsf, c.split)
        elif "t" in c.var:                      # nine launches into one [Cout][9][Cin] window
            out = GBuf(dev, (rows, cols), out=True)
            Ho, Wo = R.out_hw(c)
            for t in range(9):
                plan = _call("scnattn_wgrad16_rows", dev, R.rows_out(c), c.Cin, c.Cout, dy.ptr, x.ptr, R.rows_in(c),
                             out.ptr.value + 4 * t * c.Cin, 9 * c.Cin, c.s, c.Hi, c.Wi, Ho, Wo, t // 3 - 1, t % 3 - 1, wsp,
                             wsf, c.split)
        else:
            out = GBuf(dev, (rows, cols), (c.Cin + 4, 1), out=True)
            Ho, Wo = R.out_hw(c)
            g = (c.s, c.Hi, c.Wi, Ho, Wo) if c.s > 1 else (0, 0, 0, 0, 0)
            plan = _call("scnattn_wgrad16_rows", dev, R.rows_out(c), c.Cin, c.Cout, dy.ptr, x.ptr, R.rows_in(c), out.ptr, c.Cin + 4, *g, 0, 0,
                         wsp, wsf, c.split)
        return plan if dev.type == "cpu" else dict(out=out.read(cid), part=None)

    ex = L.ConvExtra(epi=c.epi, force_split=c.split, force_mi=c.mi)
    if c.epi in (1, 2):
        part = GBuf(dev, (2, cols, CR.stat_ld(rows)), out=True)
        ex.stat_partial = part.ptr.value
    if c.epi == 1 and "s" in c.var:
        keep.append(_vec(dev, I["shift"]))
        ex.stat_shift = keep[-1].ptr.value
    dense = c.op in ("f3", "d3", "s3")          # the 3x3 entry points fix the leading dimensions
    if c.epi == 2:
        z = GBuf16(dev, rows, cols, ld=cols if dense else cols + 8, vals=I["z"])
        vs = [_vec(dev, I[k]) for k in ("mean", "invstd", "gamma", "beta")]
        keep += [z] + vs
        ex.ez, ex.ldz = z.ptr, z.ld
        ex.emean, ex.einvstd, ex.egamma, ex.ebeta = (v.ptr.value for v in vs)
    old = (I["c0"] if c.obf else I["c0f"]) if "b" in c.var else None
    if c.obf:
        out = GBuf16(dev, rows, cols, ld=cols if dense else cols + 8, vals=old, out=True)
        optr = out.ptr
    else:
        out = GBuf(dev, (rows, cols), (cols + 4, 1), vals=old, out=True)
        optr = out.ptr
    if c.op in ("f1", "d1"):
        p = R.gemm_of(c)
        a = GBuf16(dev, R.rows_in(c), p["K"], ld=p["K"] + 8, vals=I["x"] if c.op == "f1" else I["dy"])
        b = GBuf16(dev, p["N"], p["K"], ld=p["K"] + 8, vals=I["w"][:, 0] if c.op == "f1" else I["wt"][:, 0])
        if p["gather"]:
            ex.stride, ex.Hi, ex.Wi = c.s, c.Hi, c.Wi
            ex.Ho, ex.Wo = R.out_hw(c)
        plan = _call("scnattn_cgemm16", dev, p["M"], p["N"], p["K"], a.ptr, a.ld, b.ptr, b.ld, 1.0 if old is not None else 0.0, optr,
                               cols + 8 if c.obf else cols + 4, c.obf, wsp, wsf, C.byref(ex))
    elif c.op == "f3":
        a = GBuf16(dev, R.rows_in(c), c.Cin, vals=I["x"])
        b = GBuf16(dev, c.Cout, 9 * c.Cin, vals=I["w"])
        plan = _call("scnattn_conv3x3_fwd16", dev, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, a.ptr, b.ptr, optr, C.byref(ex), wsp, wsf)
    else:
        a = GBuf16(dev, R.rows_out(c), c.Cout, vals=I["dy"])
        b = GBuf16(dev, c.Cin, 9 * c.Cout, vals=I["wt"])
        plan = _call("scnattn_conv3x3_dgrad16", dev, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, a.ptr, b.ptr, optr, C.byref(ex), wsp, wsf)
    if dev.type == "cpu":
        return plan
    return dict(out=out.read(cid), part=part.read(cid + " partials") if part is not None else None)


_PLANS = {}


def dispatch(c):
    """-> conv16_refs.names of the case: its kernel instances in launch order and the plan fields, from the library"""
    key = R.case_id(c)
    if key not in _PLANS:
        _PLANS[key] = R.names(_run(c, R.inputs(c), CPU, torch.empty(R.WS_FLOATS + 64)))
    return _PLANS[key]


def _bits(t):
    return None if t is None else t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_conv16_case_vs_fp64(dev, ws, i):
    c = R.CASES[i]
    I = R.inputs(c)
    names = " + ".join(dispatch(c)["names"])
    got = _run(c, I, dev, ws)
    ok, ratios, fails = R.judge(c, I, got)
    for k, v in ratios.items():
        print("%s -> %s %s: worst err/bound %.3f" % (R.case_id(c), names, k, v))
        w = _WORST.setdefault((names, k), [0.0, 0])
        w[0], w[1] = max(w[0], v), w[1] + 1
    assert ok, "%s (%s): %s" % (R.case_id(c), names, "; ".join(fails))
    again = _run(c, I, dev, ws)
    assert torch.equal(_bits(got["out"]), _bits(again["out"])), "two runs of %s differ" % R.case_id(c)
    if got["part"] is not None:
        assert torch.equal(_bits(got["part"]), _bits(again["part"])), "two runs of %s differ in the partials" % R.case_id(c)


def test_bf16_weights_bit_equal_to_torch(dev):
    """ONE launch over the four weights of conv16_refs.CV_WEIGHTS; both destinations guarded"""
    from scnattn import _lib as L
    from scnattn.conv16 import _WeightDesc
    masters = R.cv_masters()
    src = [GBuf(dev, (w.numel(),), vals=w.reshape(-1)) for w in masters]
    dst = [GBuf16(dev, co, taps * ci) for (co, taps, ci) in R.CV_WEIGHTS]
    dstt = [GBuf16(dev, ci, taps * co) for (co, taps, ci) in R.CV_WEIGHTS]
    descs, prefix = [], [0]
    for (co, taps, ci), s, d, dt in zip(R.CV_WEIGHTS, src, dst, dstt):
        descs.append(_WeightDesc(s.ptr.value, d.ptr, dt.ptr, co, taps, ci, 0))
        prefix.append(prefix[-1] + taps * (co // 32) * (ci // 32))
    desc = torch.tensor(list(b"".join(bytes(d) for d in descs)), dtype=torch.uint8, device=dev)
    pre = torch.tensor(prefix, dtype=torch.int32, device=dev)
    for _ in range(2):
        L.check(L.lib().scnattn_bf16_weights(_stream(dev), len(descs), desc.data_ptr(), pre.data_ptr(), prefix[-1]), "scnattn_bf16_weights")
        torch.cuda.synchronize()
        for w, d, dt, shape in zip(masters, dst, dstt, R.CV_WEIGHTS):
            got = (d.read("plain copy").view(torch.int16), dt.read("transposed copy").view(torch.int16))
            for which, name in enumerate(("plain", "transposed")):
                diff = R.cv_mismatch(w, got[which], which)
                assert diff.numel() == 0, "%s copy of %s: %d elements differ from torch's .to(bfloat16), first %#06x vs %#06x" % (
                    name, shape, diff.numel(), int(got[which].reshape(-1)[diff[0]]) & 0xffff,
                    int(R.cv_expected(w)[0][which].reshape(-1)[diff[0]]) & 0xffff)
    _WORST[("bf16_weights_kernel", "bits")] = [0.0, len(masters)]


def test_refusals_leave_the_output_untouched(dev, ws):
    from scnattn import _lib as L
    h, st = L.lib(), _stream(dev)
    M, N, K = 64, 64, 64
    a = torch.zeros(M * 9 * K + 64, device=dev, dtype=BF)
    b = torch.zeros(N * 9 * K + 64, device=dev, dtype=BF)
    v = torch.ones(N + 4, device=dev)
    part = GBuf(dev, (2, N, CR.stat_ld(M)), out=True)
    y16 = GBuf16(dev, M, N, ld=N + 8)
    y32 = GBuf(dev, (M, 9 * N), (9 * N + 4, 1), out=True)

    def ex(**kw):
        return C.byref(L.ConvExtra(**kw))

    def mask(**kw):
        d = dict(epi=2, stat_partial=part.ptr.value, ez=a.data_ptr(), ldz=N + 8, emean=v.data_ptr(), einvstd=v.data_ptr(), egamma=v.data_ptr(),
                 ebeta=v.data_ptr())
        d.update(kw)
        return ex(**d)

    def gemm(K_=K, ldc=N + 8, beta=0.0, obf=1, e=None, wsf=R.WS_FLOATS):
        return h.scnattn_cgemm16(st, M, N, K_, a.data_ptr(), K_ + 8, b.data_ptr(), K_ + 8, beta, y16.ptr if obf else y32.ptr, ldc, obf,
                                 ws.data_ptr(), wsf, e)

    def w1(R_=64, Cin=64, Cout=64, ksl=0, g=(0, 0, 0, 0, 0)):
        return h.scnattn_wgrad16_rows(st, R_, Cin, Cout, a.data_ptr(), b.data_ptr(), R_, y32.ptr, Cin + 4, *g, 0, 0, ws.data_ptr(), R.WS_FLOATS, ksl)

    calls = [
        (lambda: gemm(K_=36), b"multiples of 8"),                                               # K not a multiple of 8
        (lambda: gemm(ldc=N + 4), b"N / ldc granularity"), (lambda: gemm(ldc=N + 2, obf=0), b"N / ldc granularity"),
        (lambda: gemm(beta=1.0, e=ex(epi=1, stat_partial=part.ptr.value)), b"needs a plain product"),   # statistics with beta
        (lambda: gemm(beta=1.0, e=mask()), b"needs a plain product"),
        (lambda: gemm(obf=0, ldc=N + 4, e=mask()), b"mask epilogue needs a bf16 output"),       # EPI 2 with an fp32 output
        (lambda: gemm(e=mask(stride=2, Hi=8, Wi=16, Ho=4, Wo=8)), b"mask epilogue needs a bf16 output, an un-gathered product"),
        (lambda: h.scnattn_conv3x3_fwd16(st, 1, 8, 8, 48, N, 1, a.data_ptr(), b.data_ptr(), y16.ptr, None, ws.data_ptr(), R.WS_FLOATS),
         b"channel multiple of 32"),
        (lambda: h.scnattn_conv3x3_dgrad16(st, 1, 5, 8, N, 64, 2, a.data_ptr(), b.data_ptr(), y16.ptr, None, ws.data_ptr(), R.WS_FLOATS),
         b"conv3x3_dgrad16: geometry"),                                                         # stride-2 d input on an odd map
        (lambda: gemm(e=ex(force_split=2), wsf=16), b"forced split does not fit"),
        (lambda: h.scnattn_wgrad16_3x3(st, 1, 8, 8, 48, 64, a.data_ptr(), b.data_ptr(), y32.ptr, ws.data_ptr(), R.WS_FLOATS, 0), b"wgrad16_3x3: shape"),
        (lambda: w1(Cin=96), b"multiples of 64"), (lambda: w1(Cout=32), b"multiples of 64"),
        (lambda: w1(R_=62, g=(2, 8, 16, 4, 8)), b"gather geometry"),                            # R % (gHo * gWo) != 0
        (lambda: w1(R_=257, ksl=2), b"wgrad16_rows: forced split does not fit"),                # 17 lines: the clamp gives 1
        (lambda: h.scnattn_wgrad16_3x3(st, 2, 9, 20, 64, 64, a.data_ptr(), b.data_ptr(), y32.ptr, ws.data_ptr(), R.WS_FLOATS, 3),
         b"wgrad16_3x3: forced split does not fit"),                                            # 36 lines: the clamp gives 2
    ]
    for call, text in calls:
        assert call() == -1
        msg = h.scnattn_last_error()
        assert text in msg, msg
    torch.cuda.synchronize()
    assert y16.untouched(), "a refused call wrote to the bf16 output"
    assert bool((y32.flat.view(torch.int32) == SENT).all()), "a refused call wrote to the fp32 output"
    assert bool((part.flat.view(torch.int32) == SENT).all()), "a refused call wrote to the partials"
