"""Every decode-step primitive of the C ABI (include/scnattn.h:196-233) against the fp64 references of
tests/decoder_kernel_refs.py, one kernel per call, at the sizes where csrc/attention.hip picks another template instance.

How a case is judged:
  * guard bands -- every buffer is a window inside a larger allocation (margin before and after, gaps between the width and
    the leading dimension, between the slabs, rows after `rows`).  Output windows sit in a sentinel bit pattern that must be
    unchanged after the call (compared as int32); input windows sit in NaN, so a stray read shows up as a NaN in a checked
    result.  The margins belong to the same allocation: neither a correct nor a slightly wrong kernel leaves it.
  * per element -- a result that is a sum of n terms must be within (n + 8) * 2^-24 * S of fp64, S = the fp64 sum of the
    absolute terms of that element: the forward bound of a summation in any order.  A result that goes through expf /
    sigmoid / tanh / a division (softmax rows, LSTM gates and states and what is multiplied by them) must be within
    4 x the worst element error of the SAME formula evaluated by torch on the CPU in fp32 (the references called with
    fp32 tensors), and never more than TOL_OUT / TOL_GRAD of its row's maximum.
  * ReLU masks -- att1 and att2 live on a grid (multiples of 1/256, att2 shifted by half a step), so |att1 + att2| >= 1/512
    everywhere and exactly representable: asserted on the fp64 side, and then ALL elements are compared.
The worst error / bound ratio per kernel and result is appended to the run's parity report (test_gpu_parity._report);
profiles/r05_parity_report_decoder_kernels.txt keeps a copy.

The case tables mirror the dispatch of csrc/attention.hip: attn_scores (early / loop / scalar);
attn_context (CU by ceil(P/8): <= 8 -> 8, 9..13 -> 13, 14..16 -> 8, > 16 -> 13; VEC by E % 4 and alignment);
mean_pixels; attn_dalpha (<8,2>: E >= 2048 and P <= 128; <4,4>: E >= 1024; <2,4>; scalar);
attn_softmax_bwd; attn_datt1_post (8 pixel rows per workgroup).  Picking: every value the sizes can take
appears at least once, and every (instance x optional pointer given / NULL) pair; sizes and options are otherwise paired
round-robin instead of as a cross product.  Each row's comment names the instance or edge it is there for.
"""
import ctypes as C

import pytest
import torch

import decoder_kernel_refs as K
from kernel_harness import GBuf, NAN, SENT, _call, _note, _slab_buf, _sum_ok, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
TOL_GRAD = 2e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


def _ptr(b):
    return None if b is None else b.ptr


# ---- judging ------------------------------------------------------------------------------------------------------------
def _yard_ok(kernel, name, got, ref64, ref32, tol):
    """|got - ref| <= min(4 x worst CPU-fp32 element error, tol x row max) per element"""
    want = ref64.double()
    got = got.double().reshape(want.shape)
    yard = float((ref32.double() - want).abs().max()) if want.numel() else 0.0
    bound = torch.minimum(torch.full_like(want, 4 * yard), tol * want.abs().amax(dim=-1, keepdim=True).expand_as(want))
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s %s: worst err/bound %.3f (CPU-fp32 yardstick %.3e, worst err %.3e)" % (kernel, name, worst, yard, float(err.max())))
    assert bool((err <= bound).all()), "%s %s: worst err/bound %.3f (yardstick %.3e, err %.3e), %d NaN" % (
        kernel, name, worst, yard, float(err.nan_to_num(1e30).max()), int(got.isnan().sum()))
    _note(kernel, name, worst, "%.0e" % tol, yard)


def _f32(x):
    return None if x is None else x.to(torch.float32)


def _f64(x):
    return None if x is None else x.to(torch.float64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(g, *shape, half=False):
    """multiples of 1/256 in [-2, 2) (+ half a step): sums of such att1 / att2 are exact and >= 1/512 away from 0"""
    k = torch.randint(-512, 512, shape, generator=g).to(torch.float32)
    return (k + (0.5 if half else 0.0)) / 256.0


# ==== attn_scores ========================================================================================================
SCORES = [
    # rows, P, A, nslab, dec_bias, b0, att2_out, mis
    (1, 1, 4, 1, 0, 0, 0, 0),        # <true>: early, every lane clamped to a = A - 4 = 0; 3 of a wave's 4 rows clamp to P - 1
    (5, 15, 5, 3, 1, 1, 1, 0),       # <false>: A % 4; pixel tail 15 of 16
    (1, 16, 252, 1, 1, 0, 1, 0),     # <true> early, first batch of 256 columns not full (:87)
    (5, 17, 256, 8, 0, 1, 0, 0),     # <true> early, one full batch; second workgroup holds 1 pixel row
    (1, 64, 260, 3, 1, 1, 0, 0),     # <true> early, second batch clamped by min(.., A - 4) (:66)
    (5, 196, 511, 1, 0, 0, 1, 0),    # <false> at the production pixel count, A just below 512
    (1, 196, 512, 8, 1, 1, 1, 0),    # <true> early, production size
    (5, 64, 516, 1, 1, 0, 0, 0),     # <true> loop form A > 512 (:96), 3 trips, last one 4 columns
    (1, 17, 1030, 3, 0, 1, 1, 0),    # <false>, A > 1024, two att2 staging trips per thread
    (5, 15, 512, 3, 1, 1, 1, 1),     # att1 off by one float: must take <false> although A % 4 == 0
    (1, 196, 516, 8, 0, 0, 0, 1),    # misaligned, loop-sized A
]


@pytest.mark.parametrize("rows,P,A,nslab,has_bd,has_b0,has_out,mis", SCORES)
def test_attn_scores(dev, rows, P, A, nslab, has_bd, has_b0, has_out, mis):
    g = _gen(1000 + A + P)
    att1 = _grid(g, rows, P, A)
    slabs = _grid(g, nslab, rows, A)
    bd = _grid(g, A) if has_bd else None
    (bd if has_bd else slabs[0]).add_(0.5 / 256.0)            # the half step that keeps att1 + att2 off 0
    w, b0 = torch.randn(A, generator=g), (torch.randn(1, generator=g) if has_b0 else None)
    ref = K.attn_scores(_f64(att1), _f64(slabs), _f64(bd), _f64(w), _f64(b0))
    assert float(ref["pre"].abs().min()) >= 1e-3            # mask-unambiguous: nothing is excluded below
    b_att1 = GBuf(dev, att1.shape, None, att1, mis=mis)
    b_att2, stride, ld = _slab_buf(dev, slabs)
    b_bd, b_w, b_b0 = (None if bd is None else GBuf(dev, (A,), None, bd)), GBuf(dev, (A,), None, w), \
        (None if b0 is None else GBuf(dev, (1,), None, b0))
    b_e = GBuf(dev, (rows, P), None, out=True)
    b_out = GBuf(dev, (rows, A), None, out=True) if has_out else None
    _call("scnattn_attn_scores", dev, rows, P, A, b_att1.ptr, b_att2.ptr, nslab, stride, ld, _ptr(b_bd), b_w.ptr, _ptr(b_b0),
          b_e.ptr, _ptr(b_out))
    _sum_ok("attn_scores", "e", b_e.read("e"), ref)
    if has_out:
        _sum_ok("attn_scores", "att2", b_out.read("att2_out"), ref)


# ==== attn_context / mean_pixels ========================================================================================
CONTEXT = [
    # rows, P, E, gpre slabs (0: none), gate_bias, alpha_out, alpha_save, gate, z, mis, scores
    (16, 1, 4, 0, 0, 1, 0, 0, 0, 0, "rand"),        # <true,0,8>: one pixel, softmax == 1; every load clamped
    (12, 8, 6, 1, 1, 1, 1, 1, 1, 0, "rand"),        # <false,0,8>: E % 4
    (2, 64, 256, 2, 0, 1, 1, 1, 1, 0, "spread"),    # <true,0,8>: ceil(P/8) = 8, exactly one 256-column workgroup
    (2, 65, 260, 8, 1, 0, 1, 0, 1, 0, "rand"),      # <true,0,13>: ceil(P/8) = 9; 4 columns in the second workgroup
    (1, 100, 255, 1, 1, 1, 0, 1, 0, 0, "equal"),    # <false,0,8>: 255 columns
    (2, 100, 2048, 2, 1, 1, 1, 1, 1, 0, "rand"),    # <true,0,13>: ceil(P/8) = 13, one batch
    (2, 105, 256, 0, 0, 1, 1, 0, 1, 0, "rand"),     # <true,0,8>: ceil(P/8) = 14; z without gpre (z = awe)
    (1, 128, 513, 2, 1, 1, 1, 1, 1, 0, "spread"),   # <false,0,8>: third workgroup holds one column
    (2, 129, 260, 1, 0, 1, 0, 1, 1, 0, "rand"),     # <true,0,13>: ceil(P/8) = 17
    (2, 196, 2048, 8, 1, 1, 1, 1, 1, 0, "spread"),  # <true,0,13>: production size
    (16, 197, 4, 1, 1, 1, 1, 1, 1, 0, "equal"),     # <true,0,13>: two batches, second one pixel row; tiny E
    (2, 196, 256, 2, 1, 1, 1, 1, 1, 1, "rand"),     # enc off by one float: <false> although E % 4 == 0
    (1, 64, 2048, 0, 0, 0, 0, 0, 0, 0, "rand"),     # every optional pointer NULL
    (2, 8, 513, 8, 0, 0, 1, 1, 0, 0, "rand"),       # <false>, gate without z, gpre without bias
]
_CTX_VEC = [c for c in CONTEXT if c[2] % 4 == 0 and c[9] == 0]


def _scores(g, rows, P, kind):
    if kind == "equal":
        return torch.full((rows, P), 0.375)
    e = torch.randn(rows, P, generator=g) * 2
    if kind == "spread" and P > 1:          # largest - smallest = 80: without the max subtraction expf overflows or all underflow
        e[:, 0], e[:, P - 1] = 45.0, -35.0
        e[:, 1:P - 1].clamp_(-30.0, 40.0)
    return e


def _run_context(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind):
    g = _gen(2000 + P + E)
    enc, e = torch.randn(rows, P, E, generator=g), _scores(g, rows, P, kind)
    gp = torch.randn(nslab, rows, E, generator=g) * 2 if nslab else None
    bb = torch.randn(E, generator=g) if has_bb else None
    ref = K.attn_context(_f64(enc), _f64(e), _f64(gp), _f64(bb))
    r32 = K.attn_context(enc, e, gp, bb)
    b_enc, b_e = GBuf(dev, enc.shape, None, enc, mis=mis), GBuf(dev, e.shape, None, e)
    b_gp, stride, ld = _slab_buf(dev, gp) if nslab else (None, 0, 0)
    b_bb = GBuf(dev, (E,), None, bb) if has_bb else None
    ald = P + 5
    b_aout = GBuf(dev, (rows, P), (ald, 1), out=True) if has_aout else None
    b_asave = GBuf(dev, (rows, P), None, out=True) if has_asave else None
    b_awe = GBuf(dev, (rows, E), None, out=True)
    b_gate = GBuf(dev, (rows, E), None, out=True) if has_gate else None
    b_z = GBuf(dev, (rows, E), None, out=True) if has_z else None
    _call("scnattn_attn_context", dev, rows, P, E, b_enc.ptr, b_e.ptr, _ptr(b_gp), nslab, stride, ld, _ptr(b_bb), _ptr(b_aout),
          ald, _ptr(b_asave), b_awe.ptr, _ptr(b_gate), _ptr(b_z))
    alphas = [b.read("alpha") for b in (b_aout, b_asave) if b is not None]
    for al in alphas:
        _yard_ok("attn_context", "alpha", al, ref["alpha"], r32["alpha"], TOL_OUT)
        assert bool((al >= 0).all()) and float((al.double().sum(1) - 1).abs().max()) <= P * 2.0 ** -23
    if len(alphas) == 2:
        assert torch.equal(alphas[0].view(torch.int32), alphas[1].view(torch.int32)), "alpha_out != alpha_save"
    _yard_ok("attn_context", "awe", b_awe.read("awe"), ref["awe"], r32["awe"], TOL_OUT)
    if has_gate and nslab:
        _yard_ok("attn_context", "gate", b_gate.read("gate"), ref["gate"], r32["gate"], TOL_OUT)
    elif has_gate:          # no gpre: the gate is not computed and must not be written
        b_gate.read("gate (no gpre)")
        assert bool((b_gate.flat.cpu().view(torch.int32) == SENT).all())
    if has_z:
        _yard_ok("attn_context", "z", b_z.read("z"), ref["z"], r32["z"], TOL_OUT)


@pytest.mark.parametrize("rows,P,E,nslab,has_bb,has_aout,has_asave,has_gate,has_z,mis,kind", CONTEXT)
def test_attn_context(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind):
    _run_context(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind)


@pytest.mark.parametrize("rows,P,E,nslab,has_bb,has_aout,has_asave,has_gate,has_z,mis,kind", _CTX_VEC)
def test_attn_context_attn_depth_0(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind):
    """option attn_depth = 0: every vector case on <true,0,8> whatever ceil(P/8) is"""
    from scnattn.functional import set_option
    set_option("attn_depth", 0)
    try:
        _run_context(dev, rows, P, E, nslab, has_bb, has_aout, has_asave, has_gate, has_z, mis, kind)
    finally:
        set_option("attn_depth", 1)


@pytest.mark.parametrize("rows,P,E,mis", sorted({(c[0], c[1], c[2], c[9]) for c in CONTEXT}))
def test_mean_pixels(dev, rows, P, E, mis):
    """attn_context_kernel<VEC,1,8,false> at the P, E set of CONTEXT (no softmax: a plain sum bound)"""
    enc = torch.randn(rows, P, E, generator=_gen(3000 + P + E))
    ref = K.mean_pixels(_f64(enc))
    b_enc, b_out = GBuf(dev, enc.shape, None, enc, mis=mis), GBuf(dev, (rows, E), None, out=True)
    _call("scnattn_mean_pixels", dev, rows, P, E, b_enc.ptr, b_out.ptr)
    _sum_ok("mean_pixels", "out", b_out.read("out"), ref)


# ==== attn_dalpha ========================================================================================================
DALPHA = [
    # rows, P, E, dalpha_in, mis
    (2, 196, 2048, 1, 0),     # <true,4,4>: E >= 1024 and P > 128 (production, dense map)
    (2, 64, 2048, 0, 0),      # <true,8,2>: E >= 2048 and P <= 128 (production, un-pooled map)
    (1, 128, 2048, 1, 0),     # <true,8,2>: P at the boundary
    (2, 129, 2048, 0, 0),     # <true,4,4>: P just above it; pixel tail 1 of 16
    (2, 196, 1024, 1, 0),     # <true,4,4>: E at the boundary, exactly one batch
    (2, 196, 512, 0, 0),      # <true,2,4>: E < 1024
    (3, 7, 6, 1, 0),          # <false,2,4>: E % 4; one partial workgroup
    (2, 33, 1023, 0, 0),      # <false,2,4>: 1023 columns, no dalpha_in
    (1, 196, 2052, 1, 0),     # <true,4,4>: third batch holds 4 columns, rest clamped to E - 4
    (2, 64, 2048, 1, 1),      # enc off by one float: <false> although E % 4 == 0
]


def _run_dalpha(dev, rows, P, E, has_in, mis):
    g = _gen(4000 + P + E)
    enc, dawe = torch.randn(rows, P, E, generator=g), torch.randn(rows, E, generator=g)
    din = torch.randn(rows, P, generator=g) if has_in else None
    ref = K.attn_dalpha(_f64(enc), _f64(dawe), _f64(din))
    ld = P + 3
    b_enc, b_dawe = GBuf(dev, enc.shape, None, enc, mis=mis), GBuf(dev, dawe.shape, None, dawe)
    b_in = GBuf(dev, (rows, P), (ld, 1), din) if has_in else None
    b_out = GBuf(dev, (rows, P), None, out=True)
    _call("scnattn_attn_dalpha", dev, rows, P, E, b_enc.ptr, b_dawe.ptr, _ptr(b_in), ld, b_out.ptr)
    _sum_ok("attn_dalpha", "dalpha", b_out.read("dalpha"), ref)


@pytest.mark.parametrize("rows,P,E,has_in,mis", DALPHA)
def test_attn_dalpha(dev, rows, P, E, has_in, mis):
    _run_dalpha(dev, rows, P, E, has_in, mis)


@pytest.mark.parametrize("rows,P,E,has_in,mis", [c for c in DALPHA if c[2] % 4 == 0 and c[4] == 0])
def test_attn_dalpha_attn_depth_0(dev, rows, P, E, has_in, mis):
    """option attn_depth = 0: every vector case on <true,2,4>"""
    from scnattn.functional import set_option
    set_option("attn_depth", 0)
    try:
        _run_dalpha(dev, rows, P, E, has_in, mis)
    finally:
        set_option("attn_depth", 1)


# ==== attn_softmax_bwd ===================================================================================================
SOFTMAX_BWD = [
    # rows, P, A, de, mis
    (2, 1, 4, 1, 0),          # <true>: one pixel (de == 0 exactly), one column group
    (2, 15, 5, 0, 0),         # <false>: A % 4, de NULL
    (1, 16, 60, 1, 0),        # <true>: 60 of a workgroup's 64 columns
    (2, 63, 64, 0, 0),        # <true>: one full column workgroup, P one short of the 64-row batch
    (2, 64, 68, 1, 0),        # <true>: second workgroup holds 4 columns; exactly one row batch
    (1, 65, 511, 1, 0),       # <false>: 511 columns
    (2, 196, 512, 1, 0),      # <true>: production size
    (1, 257, 64, 0, 0),       # <true>: P > 256, second trip of the per-thread softmax loops
    (2, 257, 5, 1, 0),        # <false> with P > 256
    (2, 196, 512, 0, 1),      # att1 off by one float: <false> although A % 4 == 0
]


@pytest.mark.parametrize("rows,P,A,has_de,mis", SOFTMAX_BWD)
def test_attn_softmax_bwd(dev, rows, P, A, has_de, mis):
    g = _gen(5000 + P + A)
    att1, att2 = _grid(g, rows, P, A), _grid(g, rows, A, half=True)
    w = torch.randn(A, generator=g)
    alpha = torch.softmax(torch.randn(rows, P, generator=g) * 2, dim=1)
    dalpha = torch.randn(rows, P, generator=g)
    ref = K.attn_softmax_bwd(_f64(att1), _f64(att2), _f64(w), _f64(alpha), _f64(dalpha))
    assert float(ref["pre"].abs().min()) >= 1e-3
    ld = A + 7
    b_att1 = GBuf(dev, att1.shape, None, att1, mis=mis)
    b_att2, b_w, b_al, b_dal = (GBuf(dev, x.shape, None, x) for x in (att2, w, alpha, dalpha))
    b_de = GBuf(dev, (rows, P), None, out=True) if has_de else None
    b_d2 = GBuf(dev, (rows, A), (ld, 1), out=True)
    _call("scnattn_attn_softmax_bwd", dev, rows, P, A, b_att1.ptr, b_att2.ptr, b_w.ptr, b_al.ptr, b_dal.ptr, _ptr(b_de),
          b_d2.ptr, ld)
    if has_de:
        _sum_ok("attn_softmax_bwd", "de", b_de.read("de"), ref)
    _sum_ok("attn_softmax_bwd", "datt2", b_d2.read("datt2"), ref)


# ==== attn_datt1_post ====================================================================================================
DATT1_POST = [
    # B, P, A, T, dl
    (1, 1, 3, 1, [1]),                        # smallest: A < 4, one pixel of a workgroup's 8
    (5, 7, 256, 5, [5, 9, 3, 1, 2]),          # dl > T is clamped, dl == 1; 7 of 8 pixel rows; one column trip
    (1, 8, 300, 51, [51]),                    # exactly one pixel workgroup; second column trip of 44; longest T
    (5, 9, 3, 51, [51, 60, 20, 1, 7]),        # second workgroup holds one pixel row
    (5, 196, 256, 5, [4, 5, 1, 7, 2]),        # production pixel count
    (1, 196, 300, 1, [3]),                    # T == 1 (the stand-alone module's call), dl > T
]


@pytest.mark.parametrize("B,P,A,T,dl", DATT1_POST)
def test_attn_datt1_post(dev, B, P, A, T, dl):
    from scnattn._lib import lib
    g = _gen(6000 + P + A + T)
    att1, att2 = _grid(g, B, P, A), _grid(g, T, B, A, half=True)
    de, w = torch.randn(T, B, P, generator=g), torch.randn(A, generator=g)
    for b in range(B):                       # steps a caption never decoded hold NaN: they must not be read
        att2[min(dl[b], T):, b], de[min(dl[b], T):, b] = NAN, NAN
    ref = K.attn_datt1_post(dl, _f64(att1), _f64(att2), _f64(de), _f64(w))
    assert ref["pre_min"] >= 1e-3
    nblk = lib().scnattn_attn_datt1_post_blocks(B, P)
    b_dl = torch.tensor(dl, dtype=torch.int32, device=dev)
    b_att1, b_att2, b_de, b_w = (GBuf(dev, x.shape, None, x) for x in (att1, att2, de, w))
    b_d1, b_dw = GBuf(dev, (B, P, A), None, out=True), GBuf(dev, (nblk, A + 1), None, out=True)
    _call("scnattn_attn_datt1_post", dev, B, P, A, T, C.c_void_p(b_dl.data_ptr()), b_att1.ptr, b_att2.ptr, b_de.ptr, b_w.ptr,
          b_d1.ptr, b_dw.ptr)
    _sum_ok("attn_datt1_post", "datt1", b_d1.read("datt1"), ref)
    part = b_dw.read("dwpart").double().sum(0)          # the partial rows are summed in fp64: only their own rounding is judged
    _sum_ok("attn_datt1_post", "dw", part[:A], ref)
    _sum_ok("attn_datt1_post", "db0", part[A], ref)


# ==== scn_mix_fwd / scn_mix_bwd ==========================================================================================
MIX_FWD = [
    # rows, F, pz slabs (0: NULL), ex, ph slabs
    (32, 1, 0, 1, 1),         # F = 1: every column its own gate block; pz NULL
    (7, 9, 2, 0, 8),          # odd F, ex NULL, 8 ph slabs
    (1, 512, 8, 1, 2),        # production F, one row, 8 pz slabs on top of ex
    (7, 512, 1, 1, 1),        # production F, single slabs
    (32, 9, 0, 0, 1),         # neither pz nor ex: pa == 0
]


@pytest.mark.parametrize("rows,F,npz,has_ex,nph", MIX_FWD)
def test_scn_mix_fwd(dev, rows, F, npz, has_ex, nph):
    g = _gen(7000 + rows + F)
    F4 = 4 * F
    pz = torch.randn(npz, rows, F4, generator=g) if npz else None
    ex = torch.randn(rows, F4, generator=g) if has_ex else None
    ph, qx, qh = torch.randn(nph, rows, F4, generator=g), torch.randn(rows, F4, generator=g), torch.randn(rows, F4, generator=g)
    ref = K.scn_mix_fwd(_f64(pz), _f64(ex), _f64(ph), _f64(qx), _f64(qh))
    b_pz, pz_s, pz_ld = _slab_buf(dev, pz) if npz else (None, 0, 0)
    b_ph, ph_s, ph_ld = _slab_buf(dev, ph, 6, 9)
    b_ex = GBuf(dev, ex.shape, None, ex) if has_ex else None
    b_qx, b_qh = GBuf(dev, qx.shape, None, qx), GBuf(dev, qh.shape, None, qh)
    b_pa, b_phs, b_xc = (GBuf(dev, s, None, out=True) for s in ((rows, F4), (rows, F4), (rows, 4, 2 * F)))
    _call("scnattn_scn_mix_fwd", dev, rows, F4, _ptr(b_pz), npz, pz_s, pz_ld, _ptr(b_ex), b_ph.ptr, nph, ph_s, ph_ld, b_qx.ptr,
          b_qh.ptr, b_pa.ptr, b_phs.ptr, b_xc.ptr)
    for name, b in (("pa", b_pa), ("phs", b_phs), ("xcat", b_xc)):
        _sum_ok("scn_mix_fwd", name, b.read(name), ref)


MIX_BWD = [
    # rows, F, slabs, layout of dxcat: "driver" = [slab][gate][row][2F] packed (csrc/sequence.cpp sDb), "wide" = gaps everywhere
    (32, 1, 1, "driver"),
    (7, 9, 2, "wide"),
    (1, 512, 8, "driver"),
    (32, 512, 2, "wide"),
]


@pytest.mark.parametrize("rows,F,n,layout", MIX_BWD)
def test_scn_mix_bwd(dev, rows, F, n, layout):
    g = _gen(8000 + rows + F)
    F4 = 4 * F
    dx = torch.randn(n, 4, rows, 2 * F, generator=g)
    qx, qh, pa, phs, ax, ah = (torch.randn(rows, F4, generator=g) for _ in range(6))     # accumulators start non-zero
    ref = K.scn_mix_bwd(_f64(dx), _f64(qx), _f64(qh), _f64(pa), _f64(phs), _f64(ax), _f64(ah))
    ld = 2 * F if layout == "driver" else 2 * F + 3
    gs = rows * ld if layout == "driver" else rows * ld + 7
    ss = 4 * gs if layout == "driver" else 4 * gs + 11
    b_dx = GBuf(dev, dx.shape, (ss, gs, ld, 1), dx, tail=ss + 64)
    b_qx, b_qh, b_pa, b_phs = (GBuf(dev, x.shape, None, x) for x in (qx, qh, pa, phs))
    dph_ld = F4 + 5
    b_dpx, b_dph = GBuf(dev, (rows, F4), None, out=True), GBuf(dev, (rows, F4), (dph_ld, 1), out=True)
    b_ax, b_ah = GBuf(dev, ax.shape, None, ax, out=True), GBuf(dev, ah.shape, None, ah, out=True)
    _call("scnattn_scn_mix_bwd", dev, rows, F4, b_dx.ptr, n, ss, ld, gs, b_qx.ptr, b_qh.ptr, b_pa.ptr, b_phs.ptr, b_dpx.ptr,
          b_dph.ptr, dph_ld, b_ax.ptr, b_ah.ptr)
    for name, b in (("dpx", b_dpx), ("dph", b_dph), ("dqx_acc", b_ax), ("dqh_acc", b_ah)):
        _sum_ok("scn_mix_bwd", name, b.read(name), ref)


# ==== lstm_fwd / lstm_bwd ================================================================================================
LSTM_FWD = [
    # rows, H, slabs, bih, bhh, tanhc, spread of the pre-activations
    (200, 1, 1, 1, 0, 1, 30.0),       # H = 1 (many rows so that the fp32 yardstick is a sample, not one number); saturated gates
    (9, 7, 2, 0, 1, 0, 1.0),          # odd H, tanhc NULL
    (3, 512, 8, 1, 1, 1, 30.0),       # production H, 8 slabs, both biases, saturated
    (5, 512, 1, 0, 0, 1, 0.01),       # no bias, pre-activations near 0
]


def _lstm_inputs(g, rows, H, n, has_bih, has_bhh, spread):
    r = (torch.rand(n, 4, rows, H, generator=g) * 2 - 1) * (spread / n)
    bih = torch.randn(4 * H, generator=g) * 0.1 if has_bih else None
    bhh = torch.randn(4 * H, generator=g) * 0.1 if has_bhh else None
    return r, bih, bhh, torch.randn(rows, H, generator=g)


@pytest.mark.parametrize("rows,H,n,has_bih,has_bhh,has_tc,spread", LSTM_FWD)
def test_lstm_fwd(dev, rows, H, n, has_bih, has_bhh, has_tc, spread):
    g = _gen(9000 + rows + H)
    r, bih, bhh, cp = _lstm_inputs(g, rows, H, n, has_bih, has_bhh, spread)
    ref, r32 = K.lstm_fwd(_f64(r), _f64(bih), _f64(bhh), _f64(cp)), K.lstm_fwd(r, bih, bhh, cp)
    ld = H + 3
    gs = rows * ld + 7
    ss = 4 * gs + 11
    b_r = GBuf(dev, r.shape, (ss, gs, ld, 1), r, tail=ss + 64)
    b_bih, b_bhh = (None if x is None else GBuf(dev, x.shape, None, x) for x in (bih, bhh))
    b_cp = GBuf(dev, cp.shape, None, cp)
    b_g, b_c, b_h = (GBuf(dev, s, None, out=True) for s in ((rows, 4 * H), (rows, H), (rows, H)))
    b_tc = GBuf(dev, (rows, H), None, out=True) if has_tc else None
    _call("scnattn_lstm_fwd", dev, rows, H, b_r.ptr, n, ss, ld, gs, _ptr(b_bih), _ptr(b_bhh), b_cp.ptr, b_g.ptr, b_c.ptr, b_h.ptr,
          _ptr(b_tc))
    for name, b in (("gates", b_g), ("c", b_c), ("h", b_h)) + ((("tanhc", b_tc),) if has_tc else ()):
        _yard_ok("lstm_fwd", name, b.read(name), ref[name], r32[name], TOL_OUT)


LSTM_BWD = [
    # rows, H, slabs of dh_next (0: NULL), dh_fc, rows_next, spread
    (200, 1, 1, 1, 198, 30.0),        # rows_next = rows - 2; saturated gates
    (9, 7, 2, 0, 9, 1.0),             # dh_fc NULL, rows_next = rows
    (3, 512, 0, 1, 0, 30.0),          # last step: rows_next = 0, dh_next NULL
    (5, 512, 8, 1, 3, 1.0),           # rows_next = rows - 2, 8 slabs
    (9, 7, 0, 0, 9, 1.0),             # neither dh_fc nor dh_next: only the cell-state path
]


@pytest.mark.parametrize("rows,H,n,has_fc,rows_next,spread", LSTM_BWD)
def test_lstm_bwd(dev, rows, H, n, has_fc, rows_next, spread):
    g = _gen(10000 + rows + H + n)
    r, _, _, cp = _lstm_inputs(g, rows, H, 1, False, False, spread)
    f = K.lstm_fwd(_f64(r), None, None, _f64(cp))
    gates, tanhc = f["gates"].float(), f["tanhc"].float()
    dh_fc = torch.randn(rows, H, generator=g) if has_fc else None
    dhn = torch.randn(n, rows, H, generator=g) if n else None
    dc = torch.randn(rows, H, generator=g)
    if n:
        dhn[:, rows_next:] = NAN          # rows that stopped decoding: nothing to read from the next step
    dc[rows_next:] = NAN
    ref = K.lstm_bwd(rows_next, _f64(dh_fc), _f64(dhn), _f64(dc), _f64(gates), _f64(cp), _f64(tanhc))
    r32 = K.lstm_bwd(rows_next, dh_fc, dhn, dc, gates, cp, tanhc)
    b_fc = GBuf(dev, dh_fc.shape, None, dh_fc) if has_fc else None
    b_dhn, ss, ld = _slab_buf(dev, dhn) if n else (None, 0, 0)
    b_dc = GBuf(dev, dc.shape, None, dc, out=True)
    b_g, b_cp, b_tc = (GBuf(dev, x.shape, None, x) for x in (gates, cp, tanhc))
    b_dr = GBuf(dev, (rows, 4 * H), None, out=True)
    _call("scnattn_lstm_bwd", dev, rows, rows_next, H, _ptr(b_fc), _ptr(b_dhn), n, ss, ld, b_dc.ptr, b_g.ptr, b_cp.ptr, b_tc.ptr,
          b_dr.ptr)
    _yard_ok("lstm_bwd", "dr", b_dr.read("dr"), ref["dr"], r32["dr"], TOL_GRAD)
    _yard_ok("lstm_bwd", "dc", b_dc.read("dc"), ref["dc"], r32["dc"], TOL_GRAD)


# ==== gate_bwd, transpose2d, colsum, mul_bcast ===========================================================================
@pytest.mark.parametrize("rows,E,n", [(4, 256, 2), (3, 7, 1), (1, 5, 8), (6, 1, 2)])     # aligned, odd, one row, one column
def test_gate_bwd(dev, rows, E, n):
    g = _gen(11000 + rows + E)
    dz, awe = torch.randn(n, rows, E, generator=g), torch.randn(rows, E, generator=g)
    gate = torch.sigmoid(torch.randn(rows, E, generator=g) * 3)
    ref = K.gate_bwd(_f64(dz), _f64(awe), _f64(gate))
    b_dz, ss, ld = _slab_buf(dev, dz)
    b_awe, b_gate = GBuf(dev, awe.shape, None, awe), GBuf(dev, gate.shape, None, gate)
    gld = E + 3
    b_dawe, b_dg = GBuf(dev, (rows, E), None, out=True), GBuf(dev, (rows, E), (gld, 1), out=True)
    _call("scnattn_gate_bwd", dev, rows, E, b_dz.ptr, n, ss, ld, b_awe.ptr, b_gate.ptr, b_dawe.ptr, b_dg.ptr, gld)
    _sum_ok("gate_bwd", "dawe", b_dawe.read("dawe"), ref)
    _sum_ok("gate_bwd", "dgpre", b_dg.read("dgpre"), ref)


@pytest.mark.parametrize("R,Cn", [(64, 32), (33, 7), (1, 40), (37, 1)])
def test_transpose2d(dev, R, Cn):
    x = torch.randn(R, Cn, generator=_gen(12000 + R))
    ldi, ldo = Cn + 3, R + 5
    b_in, b_out = GBuf(dev, x.shape, (ldi, 1), x), GBuf(dev, (Cn, R), (ldo, 1), out=True)
    _call("scnattn_transpose2d", dev, R, Cn, b_in.ptr, ldi, b_out.ptr, ldo)
    assert torch.equal(b_out.read("out").view(torch.int32), x.t().contiguous().view(torch.int32))     # a copy: bit-equal


@pytest.mark.parametrize("R,N,beta", [(128, 32, 0.0), (67, 5, 1.0), (1, 19, 1.0), (130, 1, 0.0)])
def test_colsum(dev, R, N, beta):
    g = _gen(13000 + R)
    x, out0 = torch.randn(R, N, generator=g), torch.randn(N, generator=g)
    ref = K.colsum(_f64(x), _f64(out0), beta)
    ld = N + 3
    b_x = GBuf(dev, x.shape, (ld, 1), x)
    b_out = GBuf(dev, (N,), None, out0 if beta != 0 else None, out=True)     # beta == 0: the output is not read
    _call("scnattn_colsum", dev, R, N, b_x.ptr, ld, b_out.ptr, C.c_float(beta))
    _sum_ok("colsum", "out", b_out.read("out"), ref)


@pytest.mark.parametrize("T,B,N", [(3, 4, 8), (2, 3, 5), (1, 1, 7), (4, 5, 1)])
def test_mul_bcast(dev, T, B, N):
    g = _gen(14000 + T + N)
    x, q = torch.randn(T, B, N, generator=g), torch.randn(B, N, generator=g)
    ref = K.mul_bcast(_f64(x), _f64(q))
    b_x, b_q, b_out = GBuf(dev, x.shape, None, x), GBuf(dev, q.shape, None, q), GBuf(dev, x.shape, None, out=True)
    _call("scnattn_mul_bcast", dev, T, B, N, b_x.ptr, b_q.ptr, b_out.ptr)
    _sum_ok("mul_bcast", "out", b_out.read("out"), ref)


# ==== the sequence drivers and the stand-alone modules at sizes that are not multiples of 4 ==============================
# The drivers carve `saved` / `scratch` in 256-byte granules (seq_workspace of csrc/sequence.cpp), so every sub-buffer starts aligned,
# but with such sizes its rows and per-step slices do not: every kernel behind them has to take its scalar instance.  Construction of test_decoder_edge_batches
# (fp64 oracle, TOL_OUT / TOL_GRAD, every parameter gradient, d encoder_out, d tags), no floors: the full-width case, where
# a ReLU pre-activation within rounding of 0 is likely, uses the mask-unambiguous weights of
# test_attention_gradients_meet_2e4_when_relu_mask_is_unambiguous instead.
def _ok(a, b, tol, what):
    from helpers import rel_err
    e = rel_err(a, b)
    print("%s rel_err %.3e" % (what, e))
    assert e <= tol, "%s rel_err %.3e > %.1e" % (what, e, tol)


def _rig_attention(sd, enc, g, pre="attention."):
    """channel 0 of the map is 0 or 3, encoder_att.weight[:, 0] = +-4 (alternating per unit), bias = -(+-4), other columns
    x 0.25: att1 + att2 = +-4 * (x0 - 1) + (a small part) stays away from 0 while the mask still varies over pixels and
    units.  Here x0 takes only two values (no pooling in between), so the large part would add one constant per pixel
    class to the scores, the softmax would keep one class only and d att2 would be left with rounding noise (the fp32 CPU
    oracle is then 20 % off): full_att.weight is centred over the even and over the odd units, which removes exactly that
    constant.  The margin that results is asserted by the caller."""
    A = sd[pre + "encoder_att.bias"].numel()
    sign = torch.where(torch.arange(A) % 2 == 0, 1.0, -1.0)
    W = sd[pre + "encoder_att.weight"].clone() * 0.25
    W[:, 0] = 4.0 * sign
    sd[pre + "encoder_att.weight"], sd[pre + "encoder_att.bias"] = W, -4.0 * sign
    wf = sd[pre + "full_att.weight"].clone()
    for par in (0, 1):
        wf[0, par::2] -= wf[0, par::2].mean()
    sd[pre + "full_att.weight"] = wf
    enc = enc.clone()
    enc[..., 0] = 3.0 * (torch.rand(enc.shape[:-1], generator=g) > 0.5).float()
    return enc


def _check_all_grads(m, P):
    bad = []
    for k, p in m.named_parameters():
        from helpers import rel_err
        if k.endswith("full_att.bias"):       # exactly 0 in exact arithmetic: absolute
            err, lim = (p.grad.double().cpu() - P[k].grad).abs().max().item(), 1e-4
        else:
            err, lim = rel_err(p.grad, P[k].grad), TOL_GRAD
        if not err <= lim:
            bad.append("%s err %.3e > %.1e" % (k, err, lim))
    assert not bad, "; ".join(bad)


def _decoder_vs_oracle(dev, kind, m, E, S, B, hw, L, V, seed, rig=False):
    from oracle import scnattn_ref as R
    g = _gen(seed)
    enc = torch.rand(B, hw, hw, E, generator=g)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    if rig:
        enc = _rig_attention(sd, enc, g)
        m.load_state_dict(sd)
    tags = torch.rand(B, S, generator=g)
    ln = torch.randint(2, L + 1, (B,), generator=g)           # ragged; B == 1 decodes whatever it draws
    caps = torch.randint(1, V - 3, (B, L), generator=g)
    caplens = ln.unsqueeze(1)
    si = torch.sort(ln, descending=True, stable=True)[1]
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in sd.items()}
    e1, t1 = enc.double().requires_grad_(True), tags.double().requires_grad_(True)
    R.RELU_PROBE = []
    try:
        if kind == "attention_scn":
            pr, cs, dl, al, _ = R.attention_scn_forward(P, e1, t1, caps, caplens, sort_ind=si)
        elif kind == "pure_scn":
            (pr, cs, dl, _), al = R.pure_scn_forward(P, e1, t1, caps, caplens, sort_ind=si), None
        else:
            pr, cs, dl, al, _ = R.pure_attention_forward(P, e1, caps, caplens, sort_ind=si)
        margin = min(R.RELU_PROBE) if R.RELU_PROBE else None
    finally:
        R.RELU_PROBE = None
    print("ReLU margin", margin)
    assert not rig or margin >= 1e-3, "ReLU margin %.3e" % margin
    R.caption_loss(pr, cs, dl, al, 1.0)[0].backward()
    m = m.to(dev).train()
    e2, t2 = enc.to(dev).requires_grad_(True), tags.to(dev).requires_grad_(True)
    args = (e2, caps.to(dev), caplens.to(dev)) if kind == "pure_attention" else (e2, t2, caps.to(dev), caplens.to(dev))
    out = m(*args, sort_ind=si.to(dev))
    preds, caps_s, dl2 = out[0], out[1], out[2]
    alphas = None if kind == "pure_scn" else out[3]
    assert list(dl2) == list(dl)
    _ok(preds, pr, TOL_OUT, "preds")
    if alphas is not None:
        _ok(alphas, al, TOL_OUT, "alphas")
    R.caption_loss(preds, caps_s, dl2, alphas, 1.0)[0].backward()
    _check_all_grads(m, P)
    _ok(e2.grad, e1.grad, TOL_GRAD, "denc")
    if kind != "pure_attention":
        _ok(t2.grad, t1.grad, TOL_GRAD, "dtags")
    return preds.detach(), (None if alphas is None else alphas.detach()), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("B,hw", [(1, 3), (6, 3), (33, 3), (1, 14), (6, 14), (33, 14)])
def test_attention_scn_driver_all_sizes_odd(dev, B, hw):
    """nothing is a multiple of 4: A = 26, M = 21, D = 30, F = 37, S = 13, V = 51, E = 42; P = 9 and P = 196"""
    from models.decoders.attention_scn import AttentionSCN
    torch.manual_seed(100 + B)
    m = AttentionSCN(26, 21, 30, 37, 13, 51, encoder_dim=42, dropout=0.0)
    _decoder_vs_oracle(dev, "attention_scn", m, 42, 13, B, hw, 9, 51, 200 + B + hw)


@pytest.mark.parametrize("A,M,D,F,S,E", [(25, 20, 28, 36, 14, 40), (24, 21, 28, 36, 14, 40), (24, 20, 29, 36, 14, 40),
                                         (24, 20, 28, 35, 14, 40), (24, 20, 28, 36, 13, 40), (24, 20, 28, 36, 14, 41)])
def test_attention_scn_driver_one_odd_size_at_a_time(dev, A, M, D, F, S, E):
    """test_decoder_edge_batches' model with exactly one of A, M, D, F, S, E off the multiple of 4"""
    from models.decoders.attention_scn import AttentionSCN
    torch.manual_seed(A + M + D + F + S + E)
    m = AttentionSCN(A, M, D, F, S, 50, encoder_dim=E, dropout=0.0)
    _decoder_vs_oracle(dev, "attention_scn", m, E, S, 6, 3, 9, 50, 300 + A + M + D + F + S + E)


def test_attention_scn_driver_full_width_with_attention_dim_513(dev):
    """VEC = false beside production-sized operands: A = 513, everything else at full width (E = 2048, D = M = F = 512,
    P = 196)"""
    from models.decoders.attention_scn import AttentionSCN
    torch.manual_seed(513)
    m = AttentionSCN(513, 512, 512, 512, 1000, 60, encoder_dim=2048, dropout=0.0)
    _decoder_vs_oracle(dev, "attention_scn", m, 2048, 1000, 6, 14, 7, 60, 513, rig=True)


def test_pure_scn_and_pure_attention_drivers_at_odd_sizes(dev):
    from models.decoders.pure_scn import PureSCN
    from models.decoders.pure_attention import PureAttention
    torch.manual_seed(77)
    _decoder_vs_oracle(dev, "pure_scn", PureSCN(21, 30, 37, 13, 51, encoder_dim=42, dropout=0.0), 42, 13, 6, 3, 9, 51, 401)
    _decoder_vs_oracle(dev, "pure_attention", PureAttention(26, 21, 30, 51, encoder_dim=42, dropout=0.0), 42, 13, 6, 3, 9, 51, 402)


def test_standalone_attention_and_scn_cell_modules_at_odd_sizes(dev):
    """scnattn/functional.py::attention / scn_input / scn_recurrent (the beam search's path) at P = 9 / 196, A = 26, E = 42,
    D = 30, F = 37, S = 13 against the fp64 oracle"""
    from helpers import rel_err
    from models.attention import Attention
    from models.scn_cell import SCNCell
    from oracle import scnattn_ref as R
    torch.manual_seed(31)
    for B, Pn in ((5, 9), (3, 196)):
        g = _gen(500 + Pn)
        m = Attention(42, 30, 26)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        enc = torch.rand(B, Pn, 42, generator=g)
        h, wa, wl = torch.randn(B, 30, generator=g) * 0.5, torch.randn(B, 42, generator=g), torch.randn(B, Pn, generator=g)
        P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        e1, h1 = enc.double().requires_grad_(True), h.double().requires_grad_(True)
        awe_r, al_r = R.attention_forward(P, "", e1, h1)
        ((awe_r * wa.double()).sum() + (al_r * wl.double()).sum()).backward()
        m = m.to(dev)
        e2, h2 = enc.to(dev).requires_grad_(True), h.to(dev).requires_grad_(True)
        awe, al = m(e2, h2)
        _ok(awe, awe_r, TOL_OUT, "awe"); _ok(al, al_r, TOL_OUT, "alpha")
        ((awe * wa.to(dev)).sum() + (al * wl.to(dev)).sum()).backward()
        _ok(e2.grad, e1.grad, TOL_GRAD, "denc"); _ok(h2.grad, h1.grad, TOL_GRAD, "dh")
        _check_all_grads(m, P)
    g = _gen(600)
    I, H, S, F, B = 63, 30, 13, 37, 5
    m = SCNCell(I, H, S, F)
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    ins = [torch.randn(B, n, generator=g) for n in (I, S, H, H)]
    wh, wc = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    u1, s1, h1, c1 = (x.double().requires_grad_(True) for x in ins)
    h_r, c_r = R.scn_cell_forward(P, "", u1, s1, (h1, c1))
    ((h_r * wh.double()).sum() + (c_r * wc.double()).sum()).backward()
    m = m.to(dev)
    u2, s2, h2, c2 = (x.to(dev).requires_grad_(True) for x in ins)
    hh, cc = m(u2, s2, (h2, c2))
    _ok(hh, h_r, TOL_OUT, "h"); _ok(cc, c_r, TOL_OUT, "c")
    ((hh * wh.to(dev)).sum() + (cc * wc.to(dev)).sum()).backward()
    for a, b, what in ((u2, u1, "du"), (s2, s1, "ds"), (h2, h1, "dh0"), (c2, c1, "dc0")):
        _ok(a.grad, b.grad, TOL_GRAD, what)
    _check_all_grads(m, P)


def test_pool_descriptor_with_odd_sizes_is_refused_or_takes_the_dense_path(dev):
    """The pooled path needs A % 4 == 0 and E % 4 == 0: the driver refuses such a descriptor with its message
    (csrc/sequence.cpp check_pool; a host-side argument check, nothing is launched), and the module layer
    (models/decoders/_common.py resolve_prepool) never builds one: it decodes the pooled encoder_out densely, and
    with no encoder_out to fall back on it raises."""
    from models.decoders.attention_scn import AttentionSCN
    from scnattn import _lib
    from scnattn.functional import pool_taps
    pool = pool_taps(8, 8, 14, 14, dev)
    sv, sc = C.c_size_t(), C.c_size_t()
    for A, E in ((26, 40), (24, 42)):
        d = _lib.Dims(4, 196, E, A, 28, 36, 20, 14, 50, 5, 6, 1)
        with pytest.raises(RuntimeError, match="attention_dim and encoder_dim must be multiples of 4"):
            _lib.call("scnattn_seq_workspace", C.byref(d), C.byref(pool.cstruct), C.byref(sv), C.byref(sc))
    torch.manual_seed(8)
    m = AttentionSCN(26, 20, 28, 36, 14, 50, encoder_dim=40, dropout=0.0).to(dev).train()
    x = torch.rand(4, 8, 8, 40, device=dev)
    tags, caps = torch.rand(4, 14, device=dev), torch.randint(1, 47, (4, 6), device=dev)
    caplens = torch.tensor([[6], [5], [3], [2]], device=dev)
    with pytest.raises(RuntimeError, match="no usable prepool map"):
        m(None, tags, caps, caplens, prepool=x, pool_size=14)
    enc = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 14).permute(0, 2, 3, 1).contiguous()
    dense, with_map = m(enc, tags, caps, caplens), m(enc, tags, caps, caplens, prepool=x, pool_size=14)
    assert torch.equal(dense[0], with_map[0]) and torch.equal(dense[3], with_map[3])      # the same (dense) path, bit for bit


@pytest.mark.parametrize("mode", [1, 2])
def test_decoder_bf16_option_at_odd_sizes_runs_fp32(dev, mode):
    """option decoder_bf16 = 1 / 2 needs D, F, E (and A) to be multiples of 4 (csrc/sequence.cpp bf16_mode); otherwise the
    drivers run fp32 without saying so.  Pinned: bit-equal predictions, alphas and gradients to the decoder_bf16 = 0 run."""
    from models.decoders.attention_scn import AttentionSCN
    from scnattn.functional import set_option
    torch.manual_seed(90)
    m = AttentionSCN(26, 21, 30, 37, 13, 51, encoder_dim=42, dropout=0.0).to(dev).train()
    g = _gen(91)
    enc, tags = torch.rand(6, 3, 3, 42, generator=g).to(dev), torch.rand(6, 13, generator=g).to(dev)
    caps = torch.randint(1, 48, (6, 9), generator=g).to(dev)
    caplens = torch.tensor([[9], [7], [7], [4], [3], [2]], device=dev)
    runs = []
    for opt in (0, mode):
        set_option("decoder_bf16", opt)
        try:
            m.zero_grad(set_to_none=True)
            e = enc.clone().requires_grad_(True)
            out = m(e, tags, caps, caplens)
            ((out[0] ** 2).sum() + (out[3] ** 2).sum()).backward()
            runs.append([out[0].detach(), out[3].detach(), e.grad] + [p.grad.clone() for p in m.parameters()])
        finally:
            set_option("decoder_bf16", 0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hin,mis", [(8, 0), (10, 0), (8, 1), (10, 1)])
def test_pooled_driver_instances_vs_oracle(dev, hin, mis, monkeypatch):
    """The pooled instances -- attn_context_kernel<.., POOLED = true> (CU = 8 for the 8x8 map, Q = 64; CU = 13 for a
    10x10 map, Q = 100), attn_softmax_bwd with taps, weighted_rows (MODE 2), pool_expand / pool_transpose /
    add_bcast_rows_w -- chained by the pooled sequence driver, against the fp64 oracle fed with AdaptiveAvgPool2d(14)(x).
    (Each of them alone, per element, through its own entry: tests/test_gpu_attn_variant_kernels.py.)
    mis = 1: the driver is handed the un-pooled map one float off 16-byte alignment (the module layer always passes a
    fresh, aligned tensor, so the map is re-homed on the way in): the scalar forms of the same instances."""
    import torch.nn.functional as F
    import scnattn.functional as SF
    from models.decoders.attention_scn import AttentionSCN
    from oracle import scnattn_ref as R
    if mis:
        inner = SF.decoder_sequence

        def shifted(dims, bt_host, enc, *rest, **kw):
            store = torch.zeros(enc.numel() + 1, device=enc.device)
            view = store[1:].view_as(enc)
            view.copy_(enc)                       # differentiable: d x flows back through the copy
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            return inner(dims, bt_host, view, *rest, **kw)
        monkeypatch.setattr(SF, "decoder_sequence", shifted)
    torch.manual_seed(40 + hin)
    B, V, L, E = 5, 50, 9, 64
    m = AttentionSCN(32, 24, 32, 40, 12, V, encoder_dim=E, dropout=0.0)
    g = _gen(41 + hin)
    x, tags = torch.rand(B, hin, hin, E, generator=g), torch.rand(B, 12, generator=g)
    ln = torch.tensor([9, 7, 7, 4, 2])
    caps, caplens = torch.randint(1, V - 3, (B, L), generator=g), ln.unsqueeze(1)
    si = torch.sort(ln, descending=True, stable=True)[1]
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    x1 = x.double().requires_grad_(True)
    enc1 = F.adaptive_avg_pool2d(x1.permute(0, 3, 1, 2), 14).permute(0, 2, 3, 1)
    pr, cs, dl, al, _ = R.attention_scn_forward(P, enc1, tags.double(), caps, caplens, sort_ind=si)
    R.caption_loss(pr, cs, dl, al, 1.0)[0].backward()
    m = m.to(dev).train()
    x2 = x.to(dev).requires_grad_(True)
    preds, caps_s, dl2, alphas, _ = m(None, tags.to(dev), caps.to(dev), caplens.to(dev), sort_ind=si.to(dev), prepool=x2,
                                      pool_size=14)
    _ok(preds, pr, TOL_OUT, "preds"); _ok(alphas, al, TOL_OUT, "alphas")
    R.caption_loss(preds, caps_s, dl2, alphas, 1.0)[0].backward()
    _check_all_grads(m, P)
    _ok(x2.grad, x1.grad, TOL_GRAD, "d x")
