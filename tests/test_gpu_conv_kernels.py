"""The fp32 convolution forms of the trunk -- scnattn_cgemm with a scnattn_conv_extra, scnattn_conv1x1_fwd / _dgrad / _wgrad,
scnattn_conv3x3_fwd / _dgrad / _dgrad_strided / _wgrad (gathered form and the halo-staged kernel of csrc/conv3.hip) and the two
_bn_eval forms (csrc/cgemm.hip) -- per element against the fp64 references of tests/conv_refs.py, one launch per call.

How a case is judged (the harness of tests/kernel_harness.py; the judges are conv_refs.judge):
  * every operand is a GBuf window: inputs in NaN, outputs and partials in the sentinel, inside too until written (an element
    the kernel never writes fails as a NaN, a store outside the window fails the guard check); maps are [rows][C] with ld = C
    (the entry points fix it); ldz and ldres are wider than the rows with NaN in the gap, and the rows through scnattn_cgemm
    itself (flag g) have lda / ldb / ldc wider than the rows; the split-K workspace starts as NaN;
  * products (y, dx, dw): |got - ref| <= (n + 8) * 2^-24 * sum|terms| per element, n the K of the launch (9 * C for the 3x3
    forms; for the halo kernel the in-image terms of the element's tap), sum|terms| over the in-image taps, + 1 with a prologue
    (its fma, the operand being relu(x * scale + shift) in fp64 from the fp32 inputs);
  * statistics partials (epi 1): every entry (which, channel, block < row_tiles) against the fp64 sums of the kernel's OWN
    stored output over that block's rows, same bound with n = rows of the block.  The slots [row_tiles, ldp) and the margins
    lie outside the GBuf window [2][C][row_tiles] (strides C * ldp, ldp, 1): they must still hold the sentinel -- no path
    writes zeros there;
  * mask epilogue (epi 2): the mask is decided on the CPU exactly as bn_relu_on does (conv_refs.bn_mask); masked elements are
    +0.0 bit for bit, unmasked ones meet the product bound; the partials sum g, sum g * xhat against the kernel's own stored g.
    z holds elements where the mask expression is exactly 0 and one ulp either side, and one where only the FUSED
    multiply-add is positive (conv_refs._plant_mask_edges);
  * eval epilogue (epi 3): conv_refs.bn_eval, bound (n + 16) * 2^-24 * (sum|terms| * |scale| + |mean * scale| + |beta| + |res|)
    (derivation there); under ReLU an element whose reference lies below zero by more than its bound must be 0;
  * same bits: cgemm_combine 0 / 1 / 2 on a split case of each epilogue, every split case and the halo kernel run twice;
  * refusals return < 0 with scnattn_last_error() set (the RuntimeError of scnattn._lib.check) and leave the output untouched.
The worst err / bound per (instance, result) goes to the run's parity report; profiles/parity_report_conv_kernels.txt keeps a
copy, profiles/conv_kernel_tests_kernel_coverage.txt the instances reached.  Wall time of the module on an MI355X: under 4 s.

Which instance and which second launch a case reaches is asked of the library: `_run` on the CPU device sends the case's own
call, on host windows of the same alignment and leading dimensions, through scnattn_plan_next (kernel_harness._call) and
conv_refs.name renders the plan (`dispatch`); the row selections below are made from those plans at collection time, so the
library is a prerequisite of this module.  tests/test_conv_refs.py asserts without a GPU that every instance is reached.
The policy, for orientation (cgemm_plan of csrc/cgemm.hip states it):
  api.cpp                    which product an entry point is (layout, M / N / K, the 3x3 mode, gather)
  cgemm_plan                 vector store; row tile mi (1 when the 128-row grid has < 256 tiles and M > 64, never for 3x3
                             forward / d input; stride-2 d input: 1 below 768 class tiles; 4 when N <= 64 and M >= 128;
                             option cgemm_mi, ex->force_mi);
                             S: policy (K >= 256), 3x3 forward / d input min(4, 512 / tiles), the stride-2 d input never,
                             ex->force_split, epi 3 clamped to the in-launch combine; kper in whole 16s;
                             epi_in (the mask epilogue runs in the launch only on NN without gather, or 3x3 d input);
                             in-launch combine when S <= cgemm_combine_max and option cgemm_combine; kepi;
                             second launch: creduce_kernel<true> (epi 0), cstats_kernel<1> / <2> from slabs, or <2> reading C
                             back (S = 0) for the mask epilogue on the NT layout (w_transposed)
  launch_layout              launch_ev / launch_conv3: the template instance
  conv3x3_wgrad_halo         SEG 16 / 8, Q, wgrad_split (csrc/tile.h), cgemm_reduce when S > 1
"""
import ctypes as C

import pytest
import torch

import conv_refs as R
from kernel_harness import CPU, GBuf, NAN, SENT, _bound_ok, _call, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "fp32 convolution kernels vs fp64: worst |got - ref| / bound over all cases"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


class _Options:
    """scnattn_set_option values of a case, restored to the defaults whatever happens"""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from scnattn.functional import set_option
        try:
            for k, v in self.opts.items():
                set_option(k, v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from scnattn.functional import set_option
        for k, v in R.OPTION_DEFAULTS.items():
            set_option(k, v)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _vec(dev, v):
    return GBuf(dev, v.shape, None, v)


def _run(dev, c, opts=None, wsf=None, bufs=None, arm=False):
    """one call of the case's entry point -> (out [rows][cols], partials [2][C][row_tiles] or None, inputs); every guard word
    of the output and of the partials is checked.  `bufs` receives the output GBuf before the call (refusals).
    On the CPU device, or with `arm` on the GPU, nothing runs: -> the launch plan of the same call (kernel_harness._call)."""
    from scnattn._lib import BnEval, ConvExtra, lib
    I = R.inputs(c)
    wide = "g" in c.var
    Ri, Ro = R.rows_in(c), R.rows_out(c)
    orows, ocols = R.out_shape(c)
    ld = (lambda n, extra: (n + extra, 1)) if wide else (lambda n, extra: None)      # wide: A rows + 4, B rows + 8, C rows + 4
    b_x = GBuf(dev, (Ri, c.Cin), ld(c.Cin, 8 if c.op == "w1" else 4), I["x"])
    b_dy = GBuf(dev, (Ro, c.Cout), ld(c.Cout, 4), I["dy"])
    w = I["w"].reshape(c.Cout, -1)
    if "t" in c.var:
        w = w.t().contiguous()                                   # [Cin][Cout]
    b_w = GBuf(dev, w.shape, ld(w.shape[1], 8), w)
    beta = 1.0 if "b" in c.var else 0.0
    b_out = GBuf(dev, (orows, ocols), ld(ocols, 4), I["dx0"] if beta else None, out=True)
    if bufs is not None:
        bufs["out"] = b_out
    wsf = R.ws_floats(c) if wsf is None else wsf
    # NaN: a slab read before it is written shows (a plan query touches no memory)
    ws = (torch.empty(wsf + 4) if dev.type == "cpu" else torch.full((wsf + 4,), NAN, device=dev)) if wsf else None
    wsp = None if ws is None else C.c_void_p(ws.data_ptr())
    keep, b_part = [], None
    ex = ConvExtra()
    ex.pro, ex.epi = c.pro, (0 if c.epi == 3 else c.epi)
    ex.stride, ex.force_mi, ex.force_split = c.s, c.mi, max(c.split, 0)
    if c.op in ("f1", "w1", "d1") and c.s > 1:
        ex.Hi, ex.Wi = c.Hi, c.Wi
        ex.Ho, ex.Wo = R.out_hw(c)
    if c.pro or (c.epi == 2 and "f" in c.var):
        keep.append(_vec(dev, I["ss"]))
        ex.pro_ss = keep[-1].ptr.value
    if c.epi in (1, 2):
        rows = R.stat_rows(c)
        mt, ldp = lib().scnattn_cgemm_row_tiles(rows), lib().scnattn_cgemm_stat_ld(rows)
        assert (mt, ldp) == (R.row_tiles(rows), R.stat_ld(rows)) and ldp % 4 == 0 and mt <= ldp < mt + 4
        b_part = GBuf(dev, (2, ocols, mt), (ocols * ldp, ldp, 1), out=True)
        ex.stat_partial = b_part.ptr.value
    if c.epi == 1 and "s" in c.var:
        keep.append(_vec(dev, I["shift"]))
        ex.stat_shift = keep[-1].ptr.value
    if c.epi == 2:
        ldz = c.Cin + 4
        keep += [GBuf(dev, (Ri, c.Cin), (ldz, 1), I["z"])] + [_vec(dev, I[k]) for k in ("mean", "invstd", "gamma", "beta")]
        ex.ez, ex.emean, ex.einvstd, ex.egamma, ex.ebeta = (b.ptr.value for b in keep[-5:])
        ex.ldz = ldz
        if "f" in c.var:
            ex.egamma = ex.ebeta = None
    bn = None
    if c.epi == 3:
        keep += [_vec(dev, I[k]) for k in ("bn_gamma", "bn_beta", "bn_mean", "bn_var")]
        bn = BnEval()
        bn.gamma, bn.beta, bn.mean, bn.var = (b.ptr.value for b in keep[-4:])
        bn.eps, bn.relu = R.BN_EPS, int("l" in c.var)
        if "r" in c.var:
            keep.append(GBuf(dev, (Ro, c.Cout), (c.Cout + 4, 1), I["res"]))
            bn.res, bn.ldres = keep[-1].ptr.value, c.Cout + 4
    exp = C.byref(ex)
    geo = (c.N, c.Hi, c.Wi, c.Cin, c.Cout)
    if wide:        # scnattn_cgemm itself: the product of the 1x1 form, on rows wider than the matrices
        A, B, tA, tB, K = {"f1": (b_x, b_w, 0, 1, c.Cin), "d1": (b_dy, b_w, 0, int("t" in c.var), c.Cout),
                           "w1": (b_dy, b_x, 1, 0, Ro)}[c.op]
        call = ("scnattn_cgemm", tA, tB, orows, ocols, K, 1.0, A.ptr, A.pos.shape[1] + 4, B.ptr, B.pos.shape[1] + 8, beta, b_out.ptr,
                ocols + 4, None, None, 1, 0, 0, 0, wsp, wsf, exp)
    elif c.op == "f1" and c.epi == 3:
        call = ("scnattn_conv1x1_fwd_bn_eval", Ro, c.Cin, c.Cout, b_x.ptr, b_w.ptr, b_out.ptr, C.byref(bn), exp, wsp, wsf)
    elif c.op == "f1":
        call = ("scnattn_conv1x1_fwd", Ro, c.Cin, c.Cout, b_x.ptr, b_w.ptr, b_out.ptr, exp, wsp, wsf)
    elif c.op == "d1":
        call = ("scnattn_conv1x1_dgrad", Ri, c.Cin, c.Cout, b_dy.ptr, b_w.ptr, int("t" in c.var), beta, b_out.ptr, exp, wsp, wsf)
    elif c.op == "w1":
        call = ("scnattn_conv1x1_wgrad", Ro, c.Cin, c.Cout, b_dy.ptr, b_x.ptr, b_out.ptr, exp, wsp, wsf)
    elif c.op == "f3" and c.epi == 3:
        call = ("scnattn_conv3x3_fwd_bn_eval", *geo, c.s, b_x.ptr, b_w.ptr, b_out.ptr, C.byref(bn), exp, wsp, wsf)
    elif c.op == "f3":
        call = ("scnattn_conv3x3_fwd", *geo, c.s, b_x.ptr, b_w.ptr, b_out.ptr, exp, wsp, wsf)
    elif c.op == "d3":
        call = ("scnattn_conv3x3_dgrad", *geo, b_dy.ptr, b_w.ptr, b_out.ptr, exp, wsp, wsf)
    elif c.op == "s3":
        call = ("scnattn_conv3x3_dgrad_strided", *geo, c.s, b_dy.ptr, b_w.ptr, b_out.ptr, wsp, wsf)
    else:
        call = ("scnattn_conv3x3_wgrad", *geo, c.s, b_dy.ptr, b_x.ptr, b_out.ptr, wsp, wsf, c.split)
    with _Options(c.opts if opts is None else opts):
        plan = _call(call[0], dev, *call[1:], arm=arm)
    if dev.type == "cpu" or arm:
        return plan
    return b_out.read("out"), (None if b_part is None else b_part.read("partials")), I


_PLANS = {}


def dispatch(c):
    """-> (instance, second launch or None, info) of the case, from the launch plan of its own call"""
    key = R.case_id(c)
    if key not in _PLANS:
        _PLANS[key] = R.name(_run(CPU, c))
    return _PLANS[key]


def _kernel(c):
    inst, second, _ = dispatch(c)
    return inst if second is None else "%s + %s" % (inst, second)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_conv_per_element(dev, c):
    out, part, I = _run(dev, c)
    R.judge(c, I, out, part, _kernel(c), _bound_ok)


# ==== same bits ==========================================================================================================
def _split_rows(pred):
    rows = []
    for c in R.CASES:
        if c.op != "h3" and not c.opts and dispatch(c)[2]["S"] > 1 and dispatch(c)[2]["comb"] and pred(c):
            rows.append(c)
    return rows


def _first_per(rows, key):
    seen = {}
    for c in rows:
        seen.setdefault(key(c), c)
    return list(seen.values())


_COMBINE_ROWS = _first_per(_split_rows(lambda c: True), lambda c: (c.op, c.pro, c.epi, "f" in c.var, "b" in c.var))


@pytest.mark.parametrize("c", _COMBINE_ROWS, ids=R.case_id)
def test_combine_modes_are_bit_identical(dev, c):
    """The reduce launch (cgemm_combine = 0), the write-through combine (1) and the release combine (2) sum the slabs in slab
    order and apply the same epilogue: the same bits in the product / the masked g.  The partials are compared between the two
    in-launch forms only (cstats_kernel adds a block's rows in another order).  The eval epilogue has no second-launch form --
    with cgemm_combine = 0 it runs un-split (cgemm_plan), another order of the same sum -- so modes 1 and 2."""
    modes = (1, 2) if c.epi == 3 else (0, 1, 2)
    res = [_run(dev, c, {"cgemm_combine": m}) for m in modes]
    for r in res[1:]:
        assert torch.equal(_bits(res[0][0]), _bits(r[0]))
    if res[0][1] is not None:
        assert torch.equal(_bits(res[-2][1]), _bits(res[-1][1]))


_TWICE_ROWS = _first_per(_split_rows(lambda c: True), lambda c: (c.op, c.epi, dispatch(c)[2]["mi"])) + \
    _first_per([c for c in R.CASES if c.op == "h3"], lambda c: (dispatch(c)[0], dispatch(c)[2]["S"]))


@pytest.mark.parametrize("c", _TWICE_ROWS, ids=R.case_id)
def test_twice_is_bit_identical(dev, c):
    """outputs and partials: the arrival counters of the in-launch combine are back at zero, the slab order is fixed"""
    (o1, p1, _), (o2, p2, _) = _run(dev, c), _run(dev, c)
    assert torch.equal(_bits(o1), _bits(o2))
    assert p1 is None or torch.equal(_bits(p1), _bits(p2))


def test_armed_call_launches_nothing(dev):
    """scnattn_plan_next on the GPU's own buffers: the armed call returns its plan and leaves the sentinel-filled output
    window and its guard words as they were; the same call right after, un-armed, is judged as usual"""
    c = R.case("f1", 65, 1, 1, 16, 16)
    bufs = {}
    plan = _run(dev, c, bufs=bufs, arm=True)
    assert R.name(plan) == dispatch(c) and plan.grid_x >= 1
    assert bool((bufs["out"].flat.cpu().view(torch.int32) == SENT).all()), "an armed call wrote to its output"
    out, part, I = _run(dev, c)
    R.judge(c, I, out, part, _kernel(c), _bound_ok)


# ==== helpers ============================================================================================================
def test_row_tiles_and_stat_ld(dev):
    from scnattn._lib import lib
    for M in (1, 63, 64, 65, 128, 129, 255, 256, 257, 4096, 100000):
        assert lib().scnattn_cgemm_row_tiles(M) == R.row_tiles(M) == -(-M // 64)
        assert lib().scnattn_cgemm_stat_ld(M) == R.stat_ld(M) == (R.row_tiles(M) + 3) // 4 * 4


# ==== refusals: host-side argument checks, nothing is launched ===========================================================
REFUSALS = [
    ("epi with beta != 0", R.case("d1", 65, 1, 1, 16, 16, epi=2, var="b"), None, "statistics epilogue needs a plain product"),
    ("a TN product with epi", R.case("w1", 36, 1, 1, 16, 4, epi=1, var="g"), None, "TN product takes no statistics epilogue"),
    ("1x1 d input with a stride", R.case("d1", 36, 1, 1, 16, 16, s=2), None, "conv1x1_dgrad: no prologue / stride here"),
    ("3x3 forward, Cin % 16 != 0", R.case("f3", 2, 3, 5, 20, 16), None, "3x3 mode / layout / channel multiple"),
    ("strided 3x3 d weight, Cin % 128 != 0", R.case("w3", 2, 5, 4, 32, 32, s=2), None, "3x3 mode / layout / channel multiple"),
    ("stride-2 d input on an odd map", R.case("s3", 2, 5, 4, 16, 16, s=2), None, "conv3x3_dgrad_strided: stride 2, even map"),
    ("_bn_eval with a prologue", R.case("f1", 65, 1, 1, 16, 16, pro=1, epi=3), None, "ex carries geometry only"),
    ("halo k_slices above Q / 16", R.case("h3", 2, 3, 16, 32, 32, split=2), None, "conv3x3_wgrad_halo: forced split does not fit"),
    ("forced split beyond the workspace", R.case("f1", 129, 1, 1, 144, 68, split=2), 129 * 68, "cgemm: forced split does not fit"),
]


@pytest.mark.parametrize("what,c,wsf,msg", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(dev, what, c, wsf, msg):
    bufs = {}
    with pytest.raises(RuntimeError, match=msg):
        _run(dev, c, wsf=wsf, bufs=bufs)
    got = bufs["out"].read("out")
    if "b" in c.var:              # with beta the window holds C0: unchanged
        assert torch.equal(got, R.inputs(c)["dx0"]), what
    else:
        assert bool((bufs["out"].flat.cpu().view(torch.int32) == SENT).all()), what
