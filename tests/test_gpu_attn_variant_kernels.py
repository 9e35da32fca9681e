"""The instances of csrc/attention.hip that only the sequence drivers launch -- every bf16_t instance (the streamed operand
att1 / enc / x as raw bf16: option decoder_bf16) and every pooled one (scnattn_pool: the timed training path) -- one kernel
per call through the test-facing entries scnattn_attn_*_bf16, scnattn_attn_context_pooled, scnattn_attn_softmax_bwd_pooled,
scnattn_weighted_rows, scnattn_pool_expand, scnattn_pool_transpose and scnattn_add_bcast_rows_w, against the fp64 references
of tests/decoder_kernel_refs.py.

Judged exactly as tests/test_gpu_decoder_kernels.py judges the fp32 dense instances (its docstring): guard bands
(NaN around every input window, the sentinel around every output window, an optional output passed as NULL leaves nothing
written), (n + 8) * 2^-24 * sum|terms| per element for results that are sums, 4 x the worst CPU-fp32 element error (never
more than TOL_OUT of the row maximum) for what goes through expf / sigmoid / the division.  The constants and the judges are
that module's.

bf16 inputs are made exact: every value of the streamed operand survives x.to(bfloat16).float() unchanged (asserted), so the
bf16 instance computes the same function of the same numbers as the fp32 instance and owes the fp32 bounds, not a bf16
tolerance.  ReLU masks: att1 = k/64 with |k| < 256 (bf16-representable), att2 = (j + 1/2)/64 in fp32: sums are exact and
|att1 + att2| >= 1/128, asserted on the fp64 side, and then ALL elements are compared.

Second tier, bit equality: fed the same values as fp32 (at an alignment that selects the same VEC form) the fp32 instance
accumulates in the same order -- CU, U and RW change the batching of the loads, not the order of the sums -- so the two
results are compared as int32.

The tables mirror the launchers of csrc/attention.hip: attn_scores (vec_ok: A % 4 and 8-byte alignment for bf16); attn_context
(dense bf16: always <VEC,0,13>, the scalar form <false,0,8>; whatever P and option attn_depth are); attn_context_pooled (bf16:
always CU 8; fp32: CU by ceil(Q/8): <= 8 -> 8, 9..13 -> 13, 14..16 -> 8, > 16 -> 13, attn_depth = 0 -> 8); attn_dalpha (bf16:
<8,2> for E >= 2048 and P <= 128, else <4,4>, scalar <false,2,4>; attn_depth is ignored); attn_softmax_bwd (+ DalphaTaps: the
pooled form stages dalphaq in the array it later reuses for the partial sums); attn_datt1_post; weighted_rows (MODE 2);
pool_expand / pool_transpose / add_bcast_rows_w (one f32x4 per thread, 256 threads per workgroup).  Options are paired
round-robin, no cross products; each row's comment names the instance or edge it is there for.
"""
import ctypes as C

import pytest
import torch

import decoder_kernel_refs as K
from kernel_harness import BF, GBuf, GBuf16, NAN, SENT, U, _bound_ok, _call, _slab_buf, _sum_ok, _write_report  # noqa: F401 (fixture)
from test_gpu_decoder_kernels import DATT1_POST, TOL_OUT, _f64, _gen, _ptr, _scores, _yard_ok

pytestmark = pytest.mark.gpu

REPORT_TITLE = ("bf16 and pooled attention kernels vs fp64 (bf16-representable inputs, fp32 bounds): worst |got - ref| / bound "
                "over all cases")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _grid16(g, *shape, half=False):
    """multiples of 1/64 in (-4, 4): 8 significant bits, so exact in bf16 (+ half a step for att2, which stays fp32)"""
    k = torch.randint(-255, 256, shape, generator=g).to(torch.float32)
    return (k + (0.5 if half else 0.0)) / 64.0


def _rand16(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).float()


def _streamed(dev, vals, bf, mis):
    """The streamed operand [..., W]: a bf16 window `mis` elements off its 128-byte aligned base, or (bf = 0) the same values
    in an fp32 window one float off when mis != 0 -- the alignment at which the fp32 launcher picks the same VEC form."""
    assert torch.equal(vals.to(BF).float(), vals), "the streamed operand must be bf16-representable"
    if bf:
        b = GBuf16(dev, vals.numel() // vals.shape[-1], vals.shape[-1], vals=vals.to(BF), mis=mis)
        return b, C.c_void_p(b.ptr)
    b = GBuf(dev, vals.shape, None, vals, mis=1 if mis else 0)
    return b, b.ptr


def _same_bits(kernel, a, b, what="the bf16 instance differs from the fp32 instance fed the same values"):
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s %s: %s" % (kernel, k, what)


def _untouched(buf, what):
    buf.read(what)
    assert bool((buf.flat.cpu().view(torch.int32) == SENT).all()), what + " was written"


def _pool(dev, shape):
    from scnattn.functional import pool_taps
    return pool_taps(*shape, dev)


# ==== attn_scores, bf16 ==================================================================================================
SCORES16 = [
    # rows, P, A, nslab, dec_bias, b0, att2_out, mis (bf16 elements)
    (1, 1, 4, 1, 0, 0, 0, 0),        # attn_scores_kernel<true, bf16_t>: early, every lane clamped to a = A - 4 = 0
    (5, 15, 5, 3, 1, 1, 1, 0),       # attn_scores_kernel<false, bf16_t>: A % 4; pixel tail 15 of 16
    (5, 17, 256, 8, 0, 1, 0, 0),     # <true, bf16_t> early, one full batch; second workgroup holds 1 pixel row
    (1, 64, 260, 3, 1, 1, 0, 0),     # <true, bf16_t> early, second batch clamped by min(.., A - 4)
    (5, 64, 516, 1, 1, 0, 0, 0),     # <true, bf16_t> loop form A > 512, last trip 4 columns
    (1, 17, 1030, 3, 0, 1, 1, 0),    # <false, bf16_t>, A > 1024
    (1, 196, 512, 8, 1, 1, 1, 0),    # <true, bf16_t> early, production size
    (5, 15, 512, 3, 1, 1, 1, 1),     # att1 one element (2 bytes) off: <false, bf16_t> although A % 4 == 0
    (1, 196, 516, 8, 0, 0, 0, 2),    # att1 two elements off: 4-byte but not 8-byte aligned, must take <false, bf16_t>
]


@pytest.mark.parametrize("rows,P,A,nslab,has_bd,has_b0,has_out,mis", SCORES16)
def test_attn_scores_bf16(dev, rows, P, A, nslab, has_bd, has_b0, has_out, mis):
    g = _gen(21000 + A + P)
    att1, slabs = _grid16(g, rows, P, A), _grid16(g, nslab, rows, A)
    bd = _grid16(g, A) if has_bd else None
    (bd if has_bd else slabs[0]).add_(0.5 / 64.0)             # the half step that keeps att1 + att2 off 0
    w, b0 = torch.randn(A, generator=g), (torch.randn(1, generator=g) if has_b0 else None)
    ref = K.attn_scores(_f64(att1), _f64(slabs), _f64(bd), _f64(w), _f64(b0))
    assert float(ref["pre"].abs().min()) >= 1.0 / 128        # mask-unambiguous: nothing is excluded below

    def run(bf):
        _, p_att1 = _streamed(dev, att1, bf, mis)
        b_att2, stride, ld = _slab_buf(dev, slabs)
        b_bd, b_w, b_b0 = (None if bd is None else GBuf(dev, (A,), None, bd)), GBuf(dev, (A,), None, w), \
            (None if b0 is None else GBuf(dev, (1,), None, b0))
        b_e = GBuf(dev, (rows, P), None, out=True)
        b_out = GBuf(dev, (rows, A), None, out=True) if has_out else None
        _call("scnattn_attn_scores_bf16" if bf else "scnattn_attn_scores", dev, rows, P, A, p_att1, b_att2.ptr, nslab, stride,
              ld, _ptr(b_bd), b_w.ptr, _ptr(b_b0), b_e.ptr, _ptr(b_out))
        return {"e": b_e.read("e"), "att2": b_out.read("att2_out") if has_out else None}
    got = run(1)
    _sum_ok("attn_scores bf16", "e", got["e"], ref)
    if has_out:
        _sum_ok("attn_scores bf16", "att2", got["att2"], ref)
    _same_bits("attn_scores", got, run(0))


# ==== attn_context, bf16 dense and pooled ================================================================================
def _run_context(dev, kernel, bf, pool, rows, P, E, x, e, gp, bb, has_aout, has_asave, has_aq, has_gate, has_z, mis, ref, r32):
    """one call of scnattn_attn_context / _bf16 (pool None) or scnattn_attn_context_pooled, judged; returns what it wrote"""
    nslab = 0 if gp is None else gp.shape[0]
    _, p_x = _streamed(dev, x, bf, mis)
    b_e = GBuf(dev, e.shape, None, e)
    b_gp, stride, ld = _slab_buf(dev, gp) if nslab else (None, 0, 0)
    b_bb = GBuf(dev, (E,), None, bb) if bb is not None else None
    ald = P + 5
    b_aout = GBuf(dev, (rows, P), (ald, 1), out=True) if has_aout else None
    b_asave = GBuf(dev, (rows, P), None, out=True) if has_asave else None
    b_aq = GBuf(dev, (rows, pool.Q), None, out=True) if pool is not None and has_aq else None
    b_awe = GBuf(dev, (rows, E), None, out=True)
    b_gate = GBuf(dev, (rows, E), None, out=True) if has_gate else None
    b_z = GBuf(dev, (rows, E), None, out=True) if has_z else None
    if pool is None:
        _call("scnattn_attn_context_bf16" if bf else "scnattn_attn_context", dev, rows, P, E, p_x, b_e.ptr, _ptr(b_gp), nslab,
              stride, ld, _ptr(b_bb), _ptr(b_aout), ald, _ptr(b_asave), b_awe.ptr, _ptr(b_gate), _ptr(b_z))
    else:
        _call("scnattn_attn_context_pooled", dev, rows, P, E, p_x, bf, C.byref(pool.cstruct), b_e.ptr, _ptr(b_gp), nslab, stride,
              ld, _ptr(b_bb), _ptr(b_aout), ald, _ptr(b_asave), _ptr(b_aq), b_awe.ptr, _ptr(b_gate), _ptr(b_z))
    out = {"alpha_out": b_aout.read("alpha_out") if has_aout else None,
           "alpha_save": b_asave.read("alpha_save") if has_asave else None,
           "alphaq": b_aq.read("alphaq_save") if b_aq is not None else None, "awe": b_awe.read("awe"), "gate": None,
           "z": b_z.read("z") if has_z else None}
    for k in ("alpha_out", "alpha_save"):
        if out[k] is not None:
            _yard_ok(kernel, "alpha", out[k], ref["alpha"], r32["alpha"], TOL_OUT)
            assert bool((out[k] >= 0).all()) and float((out[k].double().sum(1) - 1).abs().max()) <= P * 2.0 ** -23
    if has_aout and has_asave:
        _same_bits(kernel, {"alpha_out": out["alpha_out"]}, {"alpha_out": out["alpha_save"]}, "alpha_out != alpha_save")
    if out["alphaq"] is not None:
        _yard_ok(kernel, "alphaq", out["alphaq"], ref["alphaq"], r32["alphaq"], TOL_OUT)
    _yard_ok(kernel, "awe", out["awe"], ref["awe"], r32["awe"], TOL_OUT)
    if has_gate and nslab:
        out["gate"] = b_gate.read("gate")
        _yard_ok(kernel, "gate", out["gate"], ref["gate"], r32["gate"], TOL_OUT)
    elif has_gate:          # no gpre: the gate is not computed and must not be written
        _untouched(b_gate, "gate (no gpre)")
    if has_z:
        _yard_ok(kernel, "z", out["z"], ref["z"], r32["z"], TOL_OUT)
    return out


CONTEXT16 = [
    # rows, P, E, gpre slabs (0: none), gate_bias, alpha_out, alpha_save, gate, z, mis (bf16 elements), scores
    (16, 1, 4, 0, 0, 1, 0, 0, 0, 0, "rand"),        # attn_context_kernel<true,0,13,false,bf16_t>: one pixel, every load clamped
    (2, 8, 256, 1, 1, 1, 1, 1, 1, 0, "spread"),     # <true,0,13,false,bf16_t>: P <= 8, 12 of a wave's 13 loads clamped
    (2, 64, 260, 2, 0, 0, 1, 0, 1, 0, "rand"),      # <true,0,13,..>: the fp32 launcher takes CU 8 here; 4 columns in workgroup 2
    (2, 104, 256, 8, 1, 1, 0, 1, 0, 0, "equal"),    # <true,0,13,..>: exactly one batch of 13 x 8 rows
    (2, 105, 2048, 2, 1, 1, 1, 1, 1, 0, "rand"),    # <true,0,13,..>: one row into the second batch (fp32: CU 8)
    (2, 196, 2048, 8, 1, 1, 1, 1, 1, 0, "spread"),  # <true,0,13,..>: production size
    (1, 209, 256, 0, 0, 1, 1, 1, 1, 0, "rand"),     # <true,0,13,..>: three batches; gate without gpre is not written, z = awe
    (12, 8, 6, 1, 1, 1, 1, 1, 1, 0, "rand"),        # attn_context_kernel<false,0,8,false,bf16_t>: E % 4
    (1, 196, 513, 2, 0, 0, 0, 1, 0, 0, "spread"),   # <false,0,8,false,bf16_t>: third workgroup holds one column; gate without z
    (2, 196, 256, 2, 1, 1, 1, 1, 1, 1, "rand"),     # enc one element off: <false,..,bf16_t> although E % 4 == 0
    (2, 64, 256, 1, 1, 1, 0, 0, 1, 2, "equal"),     # enc two elements off (4-byte, not 8-byte aligned): <false,..,bf16_t>
    (1, 64, 2048, 0, 0, 0, 0, 0, 0, 0, "rand"),     # every optional pointer NULL
]


def _context_case(dev, rows, P, E, nslab, has_bb, kind, seed, Q=None):
    g = _gen(seed + P + E)
    x, e = _rand16(g, rows, Q or P, E), _scores(g, rows, P, kind)
    gp = torch.randn(nslab, rows, E, generator=g) * 2 if nslab else None
    bb = torch.randn(E, generator=g) if has_bb else None
    return x, e, gp, bb


@pytest.mark.parametrize("rows,P,E,nslab,has_bb,has_aout,has_asave,has_gate,has_z,mis,kind", CONTEXT16)
def test_attn_context_bf16(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind):
    x, e, gp, bb = _context_case(dev, rows, P, E, nslab, has_bb, kind, 22000)
    ref, r32 = K.attn_context(_f64(x), _f64(e), _f64(gp), _f64(bb)), K.attn_context(x, e, gp, bb)
    args = (rows, P, E, x, e, gp, bb, has_aout, has_asave, 0, has_gate, has_z, mis, ref, r32)
    got = _run_context(dev, "attn_context bf16", 1, None, *args)
    _same_bits("attn_context", got, _run_context(dev, "attn_context (fp32, bf16 values)", 0, None, *args))


def test_attn_context_bf16_ignores_attn_depth(dev):
    """option attn_depth = 0 moves the fp32 launcher to CU 8; the dense bf16 launcher stays on <true,0,13,false,bf16_t>"""
    from scnattn.functional import set_option
    rows, P, E = 2, 105, 2048
    x, e, gp, bb = _context_case(dev, rows, P, E, 2, 1, "rand", 22000)
    ref, r32 = K.attn_context(_f64(x), _f64(e), _f64(gp), _f64(bb)), K.attn_context(x, e, gp, bb)
    args = (rows, P, E, x, e, gp, bb, 1, 1, 0, 1, 1, 0, ref, r32)
    one = _run_context(dev, "attn_context bf16", 1, None, *args)
    set_option("attn_depth", 0)
    try:
        zero = _run_context(dev, "attn_context bf16", 1, None, *args)
    finally:
        set_option("attn_depth", 1)
    _same_bits("attn_context bf16", one, zero, "attn_depth = 0 changed the result")


P11, P35, P88, P1010, P1111, P1212, P1414 = (1, 1, 2, 2), (3, 5, 4, 7), (8, 8, 14, 14), (10, 10, 14, 14), (11, 11, 14, 14), \
    (12, 12, 14, 14), (14, 14, 14, 14)

CONTEXT_POOLED = [
    # pool, rows, E, gpre slabs, gate_bias, alpha_out, alpha_save, alphaq_save, gate, z, mis (elements), scores
    # each row runs attn_context_kernel<VEC,0,CU,true> (fp32) and <VEC,0,8,true,bf16_t>
    (P11, 200, 4, 0, 0, 1, 0, 1, 0, 0, 0, "rand"),         # Q = 1 (alphaq == sum of alpha; many rows: the yardstick is a sample)
    (P35, 3, 260, 1, 1, 1, 1, 1, 1, 1, 0, "spread"),       # rectangular 3x5 -> 4x7, Q = 15, P = 28: <true,0,8,true>
    (P88, 2, 2048, 8, 1, 1, 1, 1, 1, 1, 0, "rand"),        # production: Q = 64, <true,0,8,true> / <true,0,8,true,bf16_t>
    (P1010, 2, 260, 2, 0, 0, 1, 0, 0, 1, 0, "rand"),       # Q = 100: fp32 <true,0,13,true>, bf16 CU 8 with two batches
    (P1111, 2, 4, 1, 1, 1, 0, 1, 1, 0, 0, "equal"),        # Q = 121, ceil(Q/8) = 16: CU 8 with two batches in both
    (P1212, 1, 260, 0, 0, 1, 1, 1, 1, 1, 0, "rand"),       # Q = 144: fp32 <true,0,13,true>; gate without gpre is not written
    (P1414, 2, 2048, 2, 1, 1, 1, 1, 1, 1, 0, "spread"),    # identity, Q = P = 196
    (P88, 3, 6, 1, 1, 1, 1, 1, 1, 1, 0, "rand"),           # <false,0,8,true> / <false,0,8,true,bf16_t>: E % 4 (the scalar branch)
    (P1010, 2, 260, 2, 1, 1, 1, 1, 1, 1, 1, "rand"),       # x one element off: the scalar forms although E % 4 == 0
    (P88, 2, 260, 1, 0, 1, 0, 1, 0, 1, 2, "equal"),        # x two elements off (bf16: 4-byte, not 8-byte aligned)
    (P88, 1, 2048, 0, 0, 0, 0, 0, 0, 0, 0, "rand"),        # every optional pointer NULL
]


def _pooled_case(dev, shape, rows, E, nslab, has_bb, kind):
    pool = _pool(dev, shape)
    x, e, gp, bb = _context_case(dev, rows, pool.P, E, nslab, has_bb, kind, 23000 + pool.Q, Q=pool.Q)
    ref = K.attn_context_pooled(_f64(x), pool, _f64(e), _f64(gp), _f64(bb))
    return pool, x, e, gp, bb, ref, K.attn_context_pooled(x, pool, e, gp, bb)


@pytest.mark.parametrize("shape,rows,E,nslab,has_bb,has_aout,has_asave,has_aq,has_gate,has_z,mis,kind", CONTEXT_POOLED)
def test_attn_context_pooled(dev, shape, rows, E, nslab, has_bb, has_aout, has_asave, has_aq, has_gate, has_z, mis, kind):
    pool, x, e, gp, bb, ref, r32 = _pooled_case(dev, shape, rows, E, nslab, has_bb, kind)
    args = (rows, pool.P, E, x, e, gp, bb, has_aout, has_asave, has_aq, has_gate, has_z, mis, ref, r32)
    f32 = _run_context(dev, "attn_context_pooled", 0, pool, *args)
    b16 = _run_context(dev, "attn_context_pooled bf16", 1, pool, *args)
    _same_bits("attn_context_pooled", b16, f32)


def test_attn_context_pooled_with_stale_nan_in_the_lds(dev):
    """The -1 taps that pad a row of qtap_idx carry weight 0 and must be clamped to a staged alpha: un-clamped they read the
    LDS word in front of the alpha array, which this kernel never writes -- whatever an earlier kernel left there, times 0.
    That only shows when the word is not finite, so it is made so, the way input windows sit in NaN: a launch of attn_scores
    whose staged vectors (att2, w: 2 x 1032 floats, past that word) are NaN, with enough workgroups (8 per CU) that every
    CU's LDS holds them, directly before each pooled call on the 8x8 -> 14x14 table (48 of its 64 rows are padded)."""
    pool, x, e, gp, bb, ref, r32 = _pooled_case(dev, P88, 2, 2048, 2, 1, "rand")
    assert bool((pool.qtap_idx < 0).any())
    R, A = 2048, 1032
    att1, nan2, nanw = torch.zeros(R, 1, A, device=dev), torch.full((R, A), NAN, device=dev), torch.full((A,), NAN, device=dev)
    sink = torch.empty(R, 1, device=dev)
    args = (2, pool.P, 2048, x, e, gp, bb, 1, 1, 1, 1, 1, 0, ref, r32)
    for bf in (0, 1):
        _call("scnattn_attn_scores", dev, R, 1, A, C.c_void_p(att1.data_ptr()), C.c_void_p(nan2.data_ptr()), 1, 0, A, None,
              C.c_void_p(nanw.data_ptr()), None, C.c_void_p(sink.data_ptr()), None)
        assert bool(sink.isnan().all())
        _run_context(dev, "attn_context_pooled bf16" if bf else "attn_context_pooled", bf, pool, *args)


def test_attn_context_pooled_attn_depth_0(dev):
    """option attn_depth = 0 forces <true,0,8,true> at Q = 100 (two batches instead of one): the same sums in the same order"""
    from scnattn.functional import set_option
    pool, x, e, gp, bb, ref, r32 = _pooled_case(dev, P1010, 2, 260, 2, 1, "rand")
    args = (2, pool.P, 260, x, e, gp, bb, 1, 1, 1, 1, 1, 0, ref, r32)
    one = _run_context(dev, "attn_context_pooled", 0, pool, *args)
    set_option("attn_depth", 0)
    try:
        zero = _run_context(dev, "attn_context_pooled", 0, pool, *args)
    finally:
        set_option("attn_depth", 1)
    _same_bits("attn_context_pooled", one, zero, "attn_depth = 0 changed the result")


# ==== attn_dalpha, bf16 ==================================================================================================
DALPHA16 = [
    # rows, P, E, dalpha_in, mis (bf16 elements)
    (2, 64, 2048, 0, 0),      # attn_dalpha_kernel<true,8,2,bf16_t>: E >= 2048 and P <= 128 (production, un-pooled map)
    (2, 128, 2048, 1, 0),     # <true,8,2,bf16_t>: P at the boundary
    (1, 100, 2052, 1, 0),     # <true,8,2,bf16_t>: 4 columns beyond the first 2048-wide batch, the rest clamped to E - 4
    (1, 129, 2048, 0, 0),     # attn_dalpha_kernel<true,4,4,bf16_t>: P just over the boundary; pixel tail 1 of 16
    (3, 17, 4, 1, 0),         # <true,4,4,bf16_t>: every lane clamped (the fp32 launcher takes <2,4>)
    (2, 196, 1024, 0, 0),     # <true,4,4,bf16_t>: exactly one batch
    (2, 33, 1028, 1, 0),      # <true,4,4,bf16_t>: second batch holds 4 columns
    (3, 15, 6, 1, 0),         # attn_dalpha_kernel<false,2,4,bf16_t>: E % 4
    (2, 196, 256, 0, 1),      # enc one element off: <false,2,4,bf16_t>
    (2, 196, 256, 1, 2),      # enc two elements off (4-byte, not 8-byte aligned): <false,2,4,bf16_t>
]


@pytest.mark.parametrize("rows,P,E,has_in,mis", DALPHA16)
def test_attn_dalpha_bf16(dev, rows, P, E, has_in, mis):
    g = _gen(24000 + P + E)
    enc, dawe = _rand16(g, rows, P, E), torch.randn(rows, E, generator=g)
    din = torch.randn(rows, P, generator=g) if has_in else None
    ref = K.attn_dalpha(_f64(enc), _f64(dawe), _f64(din))
    ld = P + 3

    def run(bf):
        _, p_enc = _streamed(dev, enc, bf, mis)
        b_dawe = GBuf(dev, dawe.shape, None, dawe)
        b_in = GBuf(dev, (rows, P), (ld, 1), din) if has_in else None
        b_out = GBuf(dev, (rows, P), None, out=True)
        _call("scnattn_attn_dalpha_bf16" if bf else "scnattn_attn_dalpha", dev, rows, P, E, p_enc, b_dawe.ptr, _ptr(b_in), ld,
              b_out.ptr)
        return {"dalpha": b_out.read("dalpha")}
    got = run(1)
    _sum_ok("attn_dalpha bf16", "dalpha", got["dalpha"], ref)
    _same_bits("attn_dalpha", got, run(0))
    if E >= 1024 and mis == 0:          # attn_depth = 0 moves the fp32 launcher to <2,4>; the bf16 launcher ignores it
        from scnattn.functional import set_option
        set_option("attn_depth", 0)
        try:
            _same_bits("attn_dalpha bf16", got, run(1), "attn_depth = 0 changed the result")
        finally:
            set_option("attn_depth", 1)


# ==== attn_softmax_bwd, bf16 dense and pooled ============================================================================
def _run_softmax_bwd(dev, kernel, bf, pool, rows, P, A, att1, att2, w, alpha, dal, din, has_de, mis, ref):
    """dal: dalpha [rows,P] (dense) or dalphaq [rows,Q] (pooled, + din [rows,P] or None behind an ld gap)"""
    ld, dld = A + 7, P + 3
    _, p_att1 = _streamed(dev, att1, bf, mis)
    b_att2, b_w, b_al, b_dal = (GBuf(dev, v.shape, None, v) for v in (att2, w, alpha, dal))
    b_din = GBuf(dev, (rows, P), (dld, 1), din) if din is not None else None
    b_de = GBuf(dev, (rows, P), None, out=True) if has_de else None
    b_d2 = GBuf(dev, (rows, A), (ld, 1), out=True)
    if pool is None:
        _call("scnattn_attn_softmax_bwd_bf16" if bf else "scnattn_attn_softmax_bwd", dev, rows, P, A, p_att1, b_att2.ptr, b_w.ptr,
              b_al.ptr, b_dal.ptr, _ptr(b_de), b_d2.ptr, ld)
    else:
        _call("scnattn_attn_softmax_bwd_pooled", dev, rows, P, A, p_att1, bf, b_att2.ptr, b_w.ptr, b_al.ptr,
              C.byref(pool.cstruct), b_dal.ptr, _ptr(b_din), dld, _ptr(b_de), b_d2.ptr, ld)
    out = {"de": b_de.read("de") if has_de else None, "datt2": b_d2.read("datt2")}
    if has_de:
        _sum_ok(kernel, "de", out["de"], ref)
    _sum_ok(kernel, "datt2", out["datt2"], ref)
    return out


def _softmax_bwd_case(rows, P, A, seed):
    g = _gen(seed + P + A)
    att1, att2 = _grid16(g, rows, P, A), _grid16(g, rows, A, half=True)
    w = torch.randn(A, generator=g)
    alpha = torch.softmax(torch.randn(rows, P, generator=g) * 2, dim=1)
    return g, att1, att2, w, alpha


SOFTMAX_BWD16 = [
    # rows, P, A, de, mis (bf16 elements)
    (2, 1, 4, 1, 0),          # attn_softmax_bwd_kernel<true, bf16_t>: one pixel (de == 0 exactly), every load clamped
    (1, 16, 64, 0, 0),        # <true, bf16_t>: one row of the 4 x 16-row batch per thread group, de NULL
    (2, 63, 68, 1, 0),        # <true, bf16_t>: P one short of the batch; second workgroup holds 4 columns
    (2, 64, 512, 0, 0),       # <true, bf16_t>: exactly one row batch
    (1, 65, 64, 1, 0),        # <true, bf16_t>: first prefetch of a next batch (one row, the rest clamped to P - 1)
    (2, 196, 512, 1, 0),      # <true, bf16_t>: production size
    (2, 15, 5, 0, 0),         # attn_softmax_bwd_kernel<false, bf16_t>: A % 4
    (2, 196, 512, 1, 1),      # att1 one element off: <false, bf16_t> although A % 4 == 0
    (1, 64, 68, 0, 2),        # att1 two elements off (4-byte, not 8-byte aligned): <false, bf16_t>
]


@pytest.mark.parametrize("rows,P,A,has_de,mis", SOFTMAX_BWD16)
def test_attn_softmax_bwd_bf16(dev, rows, P, A, has_de, mis):
    g, att1, att2, w, alpha = _softmax_bwd_case(rows, P, A, 25000)
    dalpha = torch.randn(rows, P, generator=g)
    ref = K.attn_softmax_bwd(_f64(att1), _f64(att2), _f64(w), _f64(alpha), _f64(dalpha))
    assert float(ref["pre"].abs().min()) >= 1.0 / 128
    args = (rows, P, A, att1, att2, w, alpha, dalpha, None, has_de, mis, ref)
    got = _run_softmax_bwd(dev, "attn_softmax_bwd bf16", 1, None, *args)
    _same_bits("attn_softmax_bwd", got, _run_softmax_bwd(dev, "attn_softmax_bwd (fp32, bf16 values)", 0, None, *args))


SOFTMAX_BWD_POOLED = [
    # pool, rows, A, de, dalpha_in, mis (elements); each row runs attn_softmax_bwd_kernel<VEC, float> and <VEC, bf16_t> with
    # DalphaTaps (dalphaq staged in `part`, which later holds the partial sums)
    (P11, 2, 4, 1, 1, 0),        # Q = 1, P = 4: every tap reads dalphaq[0]
    (P35, 2, 68, 0, 0, 0),       # rectangular, Q = 15, P = 28; de NULL, dalpha_in NULL
    (P88, 2, 512, 1, 1, 0),      # production: Q = 64, P = 196
    (P1010, 1, 64, 1, 0, 0),     # Q = 100
    (P1111, 2, 4, 0, 1, 0),      # Q = 121
    (P1212, 1, 68, 1, 1, 0),     # Q = 144
    (P1414, 2, 64, 1, 0, 0),     # identity: one live tap per pixel, Q = P = 196
    (P88, 2, 5, 1, 1, 0),        # <false, ..> with taps: A % 4
    (P88, 2, 64, 0, 0, 1),       # att1 one element off: the scalar forms
    (P1010, 1, 64, 1, 1, 2),     # att1 two elements off
]


@pytest.mark.parametrize("shape,rows,A,has_de,has_in,mis", SOFTMAX_BWD_POOLED)
def test_attn_softmax_bwd_pooled(dev, shape, rows, A, has_de, has_in, mis):
    pool = _pool(dev, shape)
    P = pool.P
    g, att1, att2, w, alpha = _softmax_bwd_case(rows, P, A, 26000 + pool.Q)
    dq = torch.randn(rows, pool.Q, generator=g)
    din = torch.randn(rows, P, generator=g) if has_in else None
    ref = K.attn_softmax_bwd_pooled(_f64(att1), _f64(att2), _f64(w), _f64(alpha), pool, _f64(dq), _f64(din))
    assert float(ref["pre"].abs().min()) >= 1.0 / 128
    args = (rows, P, A, att1, att2, w, alpha, dq, din, has_de, mis, ref)
    f32 = _run_softmax_bwd(dev, "attn_softmax_bwd_pooled", 0, pool, *args)
    b16 = _run_softmax_bwd(dev, "attn_softmax_bwd_pooled bf16", 1, pool, *args)
    _same_bits("attn_softmax_bwd_pooled", b16, f32)


# ==== attn_datt1_post, bf16 ==============================================================================================
@pytest.mark.parametrize("B,P,A,T,dl", DATT1_POST)
def test_attn_datt1_post_bf16(dev, B, P, A, T, dl):
    """attn_datt1_post_kernel<bf16_t> at the cases of the fp32 table"""
    from scnattn._lib import lib
    g = _gen(27000 + P + A + T)
    att1, att2 = _grid16(g, B, P, A), _grid16(g, T, B, A, half=True)
    de, w = torch.randn(T, B, P, generator=g), torch.randn(A, generator=g)
    for b in range(B):                       # steps a caption never decoded hold NaN: they must not be read
        att2[min(dl[b], T):, b], de[min(dl[b], T):, b] = float("nan"), float("nan")
    ref = K.attn_datt1_post(dl, _f64(att1), _f64(att2), _f64(de), _f64(w))
    assert ref["pre_min"] >= 1.0 / 128
    nblk = lib().scnattn_attn_datt1_post_blocks(B, P)
    b_dl = torch.tensor(dl, dtype=torch.int32, device=dev)

    def run(bf):
        _, p_att1 = _streamed(dev, att1, bf, 0)
        b_att2, b_de, b_w = (GBuf(dev, v.shape, None, v) for v in (att2, de, w))
        b_d1, b_dw = GBuf(dev, (B, P, A), None, out=True), GBuf(dev, (nblk, A + 1), None, out=True)
        _call("scnattn_attn_datt1_post_bf16" if bf else "scnattn_attn_datt1_post", dev, B, P, A, T, C.c_void_p(b_dl.data_ptr()),
              p_att1, b_att2.ptr, b_de.ptr, b_w.ptr, b_d1.ptr, b_dw.ptr)
        return {"datt1": b_d1.read("datt1"), "dwpart": b_dw.read("dwpart")}
    got = run(1)
    _sum_ok("attn_datt1_post bf16", "datt1", got["datt1"], ref)
    part = got["dwpart"].double().sum(0)          # the partial rows are summed in fp64: only their own rounding is judged
    _sum_ok("attn_datt1_post bf16", "dw", part[:A], ref)
    _sum_ok("attn_datt1_post bf16", "db0", part[A], ref)
    _same_bits("attn_datt1_post", got, run(0))


# ==== pool_expand / pool_transpose / add_bcast_rows_w / weighted_rows ====================================================
POOL_MAPS = [
    # B, pool, A, bias: the f32x4 count B * rows * A / 4 below and above one 256-thread workgroup
    (1, P11, 4, 1),           # expand: 4 threads, transpose: 1; every pooled pixel reads source pixel 0
    (2, P35, 8, 0),           # rectangular pool, 112 / 60 threads, bias NULL
    (1, P88, 4, 0),           # 196 / 64 threads: one partial workgroup; source rows padded with -1 taps
    (2, P88, 260, 1),         # many workgroups, the last one partial; A not a multiple of 256
    (1, P1010, 8, 1),         # 10x10: a mix of 1- and 2-wide windows
]


@pytest.mark.parametrize("B,shape,A,has_bias", POOL_MAPS)
def test_pool_expand(dev, B, shape, A, has_bias):
    pool = _pool(dev, shape)
    g = _gen(28000 + pool.Q + A)
    y, bias = torch.randn(B, pool.Q, A, generator=g), (torch.randn(A, generator=g) if has_bias else None)
    ref = K.pool_expand(_f64(y), pool, _f64(bias))
    b_y, b_bias = GBuf(dev, y.shape, None, y), (GBuf(dev, (A,), None, bias) if has_bias else None)
    b_out = GBuf(dev, (B, pool.P, A), None, out=True)
    _call("scnattn_pool_expand", dev, B, pool.P, A, C.byref(pool.cstruct), b_y.ptr, _ptr(b_bias), b_out.ptr)
    _sum_ok("pool_expand", "out", b_out.read("out"), ref)


@pytest.mark.parametrize("B,shape,A,has_bias", POOL_MAPS)
def test_pool_transpose(dev, B, shape, A, has_bias):
    pool = _pool(dev, shape)
    assert shape != P88 or bool((pool.qtap_idx < 0).any())          # the 8x8 -> 14x14 table has rows padded with -1
    gr = torch.randn(B, pool.P, A, generator=_gen(29000 + pool.Q + A))
    ref = K.pool_transpose(_f64(gr), pool)
    b_in, b_out = GBuf(dev, gr.shape, None, gr), GBuf(dev, (B, pool.Q, A), None, out=True)
    _call("scnattn_pool_transpose", dev, B, pool.P, A, C.byref(pool.cstruct), b_in.ptr, b_out.ptr)
    bound = (ref["out_n"].double() + 8) * U * ref["out_abs"]          # n = the live taps of each source pixel
    _bound_ok("pool_transpose", "out", b_out.read("out"), ref["out"], bound)


@pytest.mark.parametrize("B,Q,E", [(1, 1, 4), (3, 15, 260), (2, 64, 2048)])     # 1 thread; partial last workgroup; production
def test_add_bcast_rows_w(dev, B, Q, E):
    g = _gen(30000 + Q + E)
    out0, wts, v = torch.randn(B, Q, E, generator=g), torch.randn(Q, generator=g), torch.randn(B, E, generator=g)
    ref = K.add_bcast_rows_w(_f64(out0), _f64(wts), _f64(v))
    b_w, b_v = GBuf(dev, wts.shape, None, wts), GBuf(dev, v.shape, None, v)
    b_out = GBuf(dev, out0.shape, None, out0, out=True)              # accumulated into: the old values are given
    _call("scnattn_add_bcast_rows_w", dev, B, Q, E, b_w.ptr, b_v.ptr, b_out.ptr)
    _sum_ok("add_bcast_rows_w", "out", b_out.read("out"), ref)


WEIGHTED_ROWS = [
    # rows, Q, E, mis
    (2, 1, 4, 0),             # attn_context_kernel<true,2,8,false>: one row, every load clamped
    (3, 64, 260, 0),          # <true,2,8,false>: the production Q; 4 columns in the second workgroup
    (2, 100, 2048, 0),        # <true,2,8,false>: two batches of 8 x 8 rows
    (2, 15, 6, 0),            # attn_context_kernel<false,2,8,false>: E % 4
    (3, 64, 260, 1),          # x one float off: <false,2,8,false> although E % 4 == 0
]


@pytest.mark.parametrize("rows,Q,E,mis", WEIGHTED_ROWS)
def test_weighted_rows(dev, rows, Q, E, mis):
    g = _gen(31000 + Q + E)
    x, wts = torch.randn(rows, Q, E, generator=g), torch.randn(Q, generator=g)
    ref = K.weighted_rows(_f64(x), _f64(wts))
    b_x, b_w, b_out = GBuf(dev, x.shape, None, x, mis=mis), GBuf(dev, wts.shape, None, wts), GBuf(dev, (rows, E), None, out=True)
    _call("scnattn_weighted_rows", dev, rows, Q, E, b_x.ptr, b_w.ptr, b_out.ptr)
    _sum_ok("weighted_rows", "out", b_out.read("out"), ref)
