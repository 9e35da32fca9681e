"""The three GEMM families of the C ABI -- scnattn_skinny_gemm / _bf16w / _bf16 (csrc/skinny.hip), scnattn_sgemm / _sgemm_ws
(csrc/sgemm.hip) and the plain-epilogue scnattn_cgemm that _sgemm_ws reaches (csrc/cgemm.hip) -- per element against the
fp64 references of tests/gemm_refs.py, one product per call, at every template instance and at the operand layouts the
drivers of csrc/sequence.cpp pass (sub-blocks of wider buffers, gaps between groups / slabs / batches).

How a case is judged (the harness of tests/kernel_harness.py):
  * every operand is a GBuf window: inputs in NaN, outputs in the sentinel, margins in front and behind, ld > width, gaps
    between groups, slabs and batches; an output starts as the sentinel unless beta != 0 (a kernel that reads C without
    being asked poisons its result); every guard word is checked after the call; the split-K workspace starts as NaN;
  * per element |got - ref| <= (n + 8) * 2^-24 * S, n = the number of terms of the element (K products, + beta*C0, + bias;
    for a skinny slab the length of its K-slice), S = the fp64 sum of their magnitudes: the forward bound of a sum of n
    rounded terms in any order.  v_mfma_f32_32x32x2_f32 is a k-ordered fp32 fma chain, split-K partials, the cross-wave
    LDS reduction and the slab sum are further additions of the same terms.  The bf16 forms are judged on the operands
    they multiply (weights / activations rounded with torch's round-to-nearest-even conversion; bf16 x bf16 is exact in
    fp32).  All elements are compared.  Rows with rowmask == 0 must be +0.0 bit for bit (C0 holds NaN there when
    beta != 0), empty K-slices of a skinny product must be written as zeros, slabs past ksplit_out must be untouched.
The worst err / bound per (instance, result) goes to the run's parity report; profiles/parity_report_gemm_kernels.txt keeps
a copy, profiles/gemm_kernel_tests_kernel_coverage.txt the kernels a trace of this file saw launched (all 75 the dispatch
below can pick).  Wall time of the module on an MI355X: under 4 s.

Which instance a row reaches is asked of the library: the row's own call, built once (_skinny_call / _dense_call), goes
through scnattn_plan_next on host windows of the same alignment and leading dimensions (kernel_harness._call with the CPU
device) and gemm_refs.skinny_name / dense_name render the plan.  tests/test_gemm_refs.py asserts, without a GPU, that every
row's `inst` is that name and that every instance below is reached:
  skinny   the slice policy of the entry point (ksplit <= 0), skinny_plan: per / nb = 1..8 / chunks / kslice (the bf16 matrix instruction: whole
           16-k blocks, nb even); XVEC = X 16-byte aligned, ldx % 4 == 0, xg % 4 == 0, K % 4 == 0, K >= 4; grid =
           (ceil(N/32) * groups, ksplit, ceil(rows/32)); <NB, XVEC, WBF, BFM>.
           inst = "nb<NB> c<chunks> v<XVEC> e<empty slices> z<grid.z>"
  sgemm_ws cgemm when use_cgemm and cgemm_supported (A, B 16-byte aligned, lda, ldb, sA, sB % 4 == 0, the contiguous extents
           % 4 == 0); sgemm_plan: S (tiles < 256 and K >= 2 * kmin, kmin = 128 for <= 16 tiles else 256; target 512 workgroups;
           at most K / kmin, 16, and what fits ws), kper in whole 16s, VEC, splitk_reduce_kernel when S > 1.
           inst = "sgemm v<VEC> S<S>"
  cgemm    cgemm_plan: vector C store = N % 4 == 0, ldc % 4 == 0, sC % 4 == 0, C 16-byte aligned; row tile mi (2: 128 rows;
           1: 64 rows when the 128-row grid has < 256 tiles and M > 64; 4: 128 x 64 when N <= 64 and M >= 128; option cgemm_mi,
           ex->force_mi); S (tiles < 224 and K >= 256: 512 / tiles, at most K / 128 and what fits ws), ex->force_split, kper in
           whole 16s; in-launch combine (finish_block) when S <= 8, vector store and option cgemm_combine, else
           creduce_kernel<vector store>.  inst = "cgemm mi<mi> S<S> <-|comb|red> <vst|sst>"
Picking: every value the sizes can take at an edge appears at least once and every instance; sizes and options are otherwise
paired round-robin instead of as a cross product.  Each row's `why` names the instance or edge it is there for.
"""
import ctypes as C
from collections import namedtuple

import pytest
import torch

import gemm_refs as R
from kernel_harness import CPU, GBuf, NAN, SENT, _call, _sum_ok, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "GEMM kernels vs fp64: worst |got - ref| / ((n+8) * 2^-24 * sum|terms|) over all cases"
OPTION_DEFAULTS = {"use_cgemm": 1, "cgemm_combine": 1, "cgemm_mi": 0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _untouched(buf):
    return bool((buf.flat.cpu().view(torch.int32) == SENT).all())


# ==== skinny =============================================================================================================
SK = namedtuple("SK", "form rows N K groups ks x inst why")
SK_ENTRY = {"f32": "scnattn_skinny_gemm", "bf16w": "scnattn_skinny_gemm_bf16w", "bf16": "scnattn_skinny_gemm_bf16"}
# x: what makes XVEC false ("" = nothing: 16-byte activation loads): "mis" X one float off 16 bytes, "ldx" ldx % 4 != 0,
# "xg" xg % 4 != 0, "K" K % 4 != 0 (or K < 4)
SKINNY = [
    # ---- nb = 1..8 (ksplit = 1) on the fp32 and the bf16-weight form
    SK("f32", 1, 33, 9, 1, 1, "K", "nb1 c1 v0 e0 z1", "nb = 1; the old test's smallest case"),
    SK("f32", 31, 31, 33, 1, 1, "K", "nb2 c1 v0 e0 z1", "nb = 2; 31 rows, 31 columns"),
    SK("f32", 7, 45, 77, 4, 1, "K", "nb3 c1 v0 e0 z1", "nb = 3; 4 groups, second column tile holds 13"),
    SK("f32", 32, 32, 128, 1, 1, "", "nb4 c1 v1 e0 z1", "nb = 4; exactly one full tile"),
    SK("f32", 33, 1, 132, 1, 1, "", "nb5 c1 v1 e0 z2", "nb = 5; N = 1; second row block holds 1 row"),
    SK("f32", 40, 33, 192, 4, 1, "", "nb6 c1 v1 e0 z2", "nb = 6; 40 rows, second column tile holds 1"),
    SK("f32", 5, 45, 200, 1, 1, "", "nb7 c1 v1 e0 z1", "nb = 7"),
    SK("f32", 32, 128, 256, 1, 1, "", "nb8 c1 v1 e0 z1", "nb = 8: one full chunk per wave"),
    SK("bf16w", 33, 45, 9, 4, 1, "K", "nb1 c1 v0 e0 z2", "nb = 1, bf16 weights, grid.z = 2"),
    SK("bf16w", 1, 1, 33, 1, 1, "K", "nb2 c1 v0 e0 z1", "nb = 2; one row, one column"),
    SK("bf16w", 32, 33, 77, 1, 1, "K", "nb3 c1 v0 e0 z1", "nb = 3"),
    SK("bf16w", 31, 32, 128, 4, 1, "", "nb4 c1 v1 e0 z1", "nb = 4"),
    SK("bf16w", 40, 31, 132, 1, 1, "", "nb5 c1 v1 e0 z2", "nb = 5; second row block partial"),
    SK("bf16w", 5, 33, 192, 1, 1, "", "nb6 c1 v1 e0 z1", "nb = 6"),
    SK("bf16w", 33, 45, 200, 4, 1, "", "nb7 c1 v1 e0 z2", "nb = 7; 4 groups x 2 row blocks"),
    SK("bf16w", 7, 32, 256, 1, 1, "", "nb8 c1 v1 e0 z1", "nb = 8"),
    # ---- nb = 2, 4, 6, 8 on the bf16 matrix instruction (k per wave in whole 16s)
    SK("bf16", 31, 45, 9, 1, 1, "K", "nb2 c1 v0 e0 z1", "K = 9 -> 16 k per wave, 7 of them past K"),
    SK("bf16", 33, 33, 77, 4, 1, "K", "nb4 c1 v0 e0 z2", "K = 77 -> nb 3 rounded to 4; grid.z = 2 on the bf16 form"),
    SK("bf16", 1, 31, 132, 1, 1, "", "nb6 c1 v1 e0 z1", "K = 132 -> nb 5 rounded to 6"),
    SK("bf16", 40, 1, 200, 1, 1, "", "nb8 c1 v1 e0 z2", "K = 200 -> nb 7 rounded to 8; N = 1"),
    # ---- several chunks per wave
    SK("f32", 7, 45, 260, 1, 1, "", "nb8 c2 v1 e0 z1", "two chunks; wave 2 holds the last 4 k, wave 3 nothing"),
    SK("bf16w", 5, 33, 260, 4, 1, "", "nb8 c2 v1 e0 z1", "two chunks, bf16 weights"),
    SK("bf16", 32, 32, 260, 1, 1, "", "nb8 c2 v1 e0 z1", "two chunks, bf16 matrix instruction"),
    SK("f32", 31, 33, 1024, 1, 1, "", "nb8 c4 v1 e0 z1", "four full chunks"),
    SK("bf16", 7, 45, 1024, 4, 1, "", "nb8 c4 v1 e0 z1", "four full chunks, bf16 matrix instruction"),
    # ---- XVEC = false, one cause at a time (K % 4 is in the rows above on every form)
    SK("f32", 32, 45, 128, 1, 1, "mis", "nb4 c1 v0 e0 z1", "X one float off 16 bytes"),
    SK("bf16", 5, 33, 128, 1, 2, "mis", "nb2 c1 v0 e0 z1", "X one float off 16 bytes, bf16 matrix instruction"),
    SK("bf16w", 7, 31, 128, 1, 1, "ldx", "nb4 c1 v0 e0 z1", "ldx % 4 != 0"),
    SK("f32", 31, 32, 64, 1, 1, "ldx", "nb2 c1 v0 e0 z1", "ldx % 4 != 0"),
    SK("bf16", 32, 45, 64, 4, 1, "xg", "nb2 c1 v0 e0 z1", "xg % 4 != 0"),
    SK("bf16w", 1, 33, 64, 4, 1, "xg", "nb2 c1 v0 e0 z1", "xg % 4 != 0"),
    SK("f32", 5, 33, 260, 1, 1, "mis", "nb8 c2 v0 e0 z1", "scalar activation loads through two chunks"),
    SK("f32", 7, 31, 132, 4, 1, "xg", "nb5 c1 v0 e0 z1", "scalar activation loads at nb = 5"),
    SK("bf16w", 7, 31, 200, 1, 1, "ldx", "nb7 c1 v0 e0 z1", "scalar activation loads at nb = 7"),
    SK("bf16w", 5, 33, 192, 4, 1, "xg", "nb6 c1 v0 e0 z1", "scalar activation loads at nb = 6"),
    SK("bf16", 5, 32, 132, 1, 1, "mis", "nb6 c1 v0 e0 z1", "scalar activation loads at nb = 6, bf16 matrix instruction"),
    SK("bf16", 7, 45, 260, 1, 1, "ldx", "nb8 c2 v0 e0 z1", "scalar activation loads through two chunks, bf16 matrix instruction"),
    SK("bf16w", 5, 33, 132, 1, 1, "mis", "nb5 c1 v0 e0 z1", "scalar activation loads at nb = 5, bf16 weights"),
    SK("f32", 7, 45, 192, 1, 1, "ldx", "nb6 c1 v0 e0 z1", "scalar activation loads at nb = 6"),
    SK("f32", 31, 33, 200, 1, 1, "mis", "nb7 c1 v0 e0 z1", "scalar activation loads at nb = 7"),
    SK("bf16w", 7, 31, 256, 4, 1, "xg", "nb8 c1 v0 e0 z1", "scalar activation loads at nb = 8, bf16 weights"),
    SK("f32", 31, 45, 96, 1, 1, "", "nb3 c1 v1 e0 z1", "16-byte activation loads at nb = 3 (K = 96)"),
    SK("bf16", 33, 32, 64, 1, 1, "", "nb2 c1 v1 e0 z2", "16-byte activation loads at nb = 2 on the bf16 matrix instruction"),
    SK("bf16w", 5, 32, 3, 1, 1, "K", "nb1 c1 v0 e0 z1", "K < 4"),
    SK("f32", 33, 31, 1, 4, 1, "K", "nb1 c1 v0 e0 z2", "K = 1"),
    SK("bf16", 7, 33, 2, 1, 1, "K", "nb2 c1 v0 e0 z1", "K < 4 on the bf16 matrix instruction"),
    # ---- ksplit: 3, 16 (empty slices), 2 with a short last slice, 0 = the policy
    SK("f32", 7, 45, 77, 1, 3, "K", "nb1 c1 v0 e0 z1", "old test; slices of 32, 32, 13"),
    SK("f32", 5, 36, 40, 4, 2, "", "nb1 c1 v1 e0 z1", "old test; last slice 8 k"),
    SK("f32", 40, 64, 128, 1, 2, "", "nb2 c1 v1 e0 z2", "old test; 40 rows"),
    SK("f32", 5, 33, 33, 1, 16, "K", "nb1 c1 v0 e14 z1", "14 empty slices: their slabs are zeros"),
    SK("bf16w", 33, 45, 40, 1, 16, "", "nb1 c1 v1 e14 z2", "14 empty slices, bf16 weights, second slice 8 k"),
    SK("bf16", 7, 31, 33, 4, 16, "K", "nb2 c1 v0 e15 z1", "whole 16s: kslice = 64, 15 empty slices"),
    SK("bf16w", 31, 33, 200, 1, 3, "", "nb3 c1 v1 e0 z1", "ksplit = 3: slices of 96, 96, 8"),
    SK("bf16", 32, 32, 200, 4, 3, "", "nb4 c1 v1 e1 z1", "ksplit = 3 in whole 16s: slices of 128, 72 and an empty one"),
    SK("f32", 1, 45, 9, 1, 0, "K", "nb1 c1 v0 e0 z1", "policy: K < 32 -> one slice"),
    SK("bf16w", 40, 33, 132, 4, 0, "", "nb2 c1 v1 e1 z2", "policy picks 4 slices; kslice = 64: 64, 64, 4 k and an empty slice"),
    # ---- the production shapes of the old tests
    SK("f32", 32, 128, 512, 1, 0, "", "nb1 c1 v1 e0 z1", "h -> att2 slice, policy split"),
    SK("f32", 32, 2048, 2048, 1, 0, "", "nb8 c1 v1 e0 z1", "h -> gate pre-activation, policy split"),
    SK("bf16w", 32, 512, 1024, 4, 0, "", "nb8 c1 v1 e0 z1", "four gate blocks, policy split (4 slices of 256)"),
    SK("bf16", 32, 4608, 512, 1, 4, "", "nb4 c1 v1 e0 z1", "N = 4608"),
    SK("f32", 32, 512, 4608, 1, 16, "", "nb8 c2 v1 e7 z1", "old test: 16 slices asked, k per wave 72 -> two chunks, kslice = 512: 9 slices hold k, 7 are empty"),
    SK("bf16", 32, 512, 1024, 4, 0, "", "nb8 c1 v1 e0 z1", "four gate blocks on the bf16 matrix instruction"),
]


def sk_layout(r):
    """leading dimensions and strides of a SKINNY row: xg > K, ldx > groups * xg, ldw > N, wg > K * ldw, ldy > N,
    yg > rows * ldy, yslab > groups * yg; everything the 16-byte activation loads need is a multiple of 4 unless r.x says not"""
    xg = (r.K + 3) // 4 * 4 + 4 + (1 if r.x == "xg" else 0)
    ldx = (r.groups * xg + 3) // 4 * 4 + 4 + (1 if r.x == "ldx" else 0)
    ldw, ldy = r.N + 3, r.N + 5
    wg, yg = r.K * ldw + 7, r.rows * ldy + 6
    return dict(xg=xg, ldx=ldx, mis=1 if r.x == "mis" else 0, ldw=ldw, wg=wg, ldy=ldy, yg=yg, yslab=r.groups * yg + 9)


def _bf16_window(dev, W, wg, ldw):
    """the bf16 copy of W [groups, K, N] as a window of 16-bit elements inside bf16 NaNs"""
    G, K, N = W.shape
    total = 16 + (G - 1) * wg + (K - 1) * ldw + N + 64
    host = torch.full((total,), 0x7FC0, dtype=torch.int16)
    pos = 16 + torch.arange(G).view(G, 1, 1) * wg + torch.arange(K).view(1, K, 1) * ldw + torch.arange(N)
    host[pos] = R.bf16_bits(W)
    flat = host.to(dev)
    return flat, C.c_void_p(flat.data_ptr() + 2 * 16)


def _skinny_inputs(r):
    g = _gen(20000 + 7 * r.rows + 3 * r.N + r.K + r.groups)
    return torch.randn(r.rows, r.groups, r.K, generator=g), torch.randn(r.groups, r.K, r.N, generator=g)


def _skinny_call(dev, r, X, W, ksplit=None):
    """-> (Y [16, groups, rows, N] as read back, guards checked; ksplit_out); on the CPU device (the launch plan, ksplit_out)"""
    L = sk_layout(r)
    b_x = GBuf(dev, X.shape, (L["ldx"], L["xg"], 1), X, mis=L["mis"])
    if r.form == "f32":
        b_w = GBuf(dev, W.shape, (L["wg"], L["ldw"], 1), W)
        wptr = b_w.ptr
    else:
        b_w, wptr = _bf16_window(dev, W, L["wg"], L["ldw"])
    b_y = GBuf(dev, (R_MAX_KSPLIT, r.groups, r.rows, r.N), (L["yslab"], L["yg"], L["ldy"], 1), out=True)
    used = C.c_int(-1)
    plan = _call(SK_ENTRY[r.form], dev, r.rows, r.N, r.K, r.groups, b_x.ptr, L["ldx"], L["xg"], wptr, L["ldw"], L["wg"], b_y.ptr,
                 L["ldy"], L["yg"], L["yslab"], r.ks if ksplit is None else ksplit, C.byref(used))
    return (plan if dev.type == "cpu" else b_y.read("Y")), used.value


def skinny_plan(r):
    """-> (the launch plan of the row's call, the ksplit it runs with)"""
    X, W = _skinny_inputs(r)
    return _skinny_call(CPU, r, X, W)


R_MAX_KSPLIT = 16       # SCN_MAX_KSPLIT (csrc/kernels.h)


@pytest.mark.parametrize("r", SKINNY, ids=lambda r: "%s-%dx%dx%d-g%d-ks%d%s" % (r.form, r.rows, r.N, r.K, r.groups, r.ks,
                                                                                 "-" + r.x if r.x else ""))
def test_skinny_gemm_per_element(dev, r):
    X, W = _skinny_inputs(r)
    Y, ks = _skinny_call(dev, r, X, W)
    assert 1 <= ks <= R_MAX_KSPLIT and (r.ks == 0 or ks == r.ks)
    assert bool((_bits(Y[ks:]) == SENT).all()), "a slab past ksplit_out = %d was written" % ks
    Xo, Wo = R.skinny_operands(X, W, r.form)
    slices = R.skinny_slices(r.K, ks, r.form)
    ref = R.skinny(Xo.double(), Wo.double(), slices)
    kern = "skinny_%s %s" % (r.form, r.inst[:r.inst.index(" e")])
    for s, (kb, ke) in enumerate(slices):                   # every slab on its own: n = its slice length
        if ke == kb:
            assert bool((Y[s] == 0).all()), "empty K-slice %d of %d is not zero" % (s, ks)
        else:
            _sum_ok(kern, "y", Y[s], R.slab(ref, s))
    _sum_ok(kern, "sum", R.slab_sum_f32(Y[:ks]), ref)
    # what the policy picked is known only through what the slabs hold: each judged above against ITS slice of K


# ==== dense ==============================================================================================================
DG = namedtuple("DG", "api ta tb M N K batch epi lay ws opts inst why")
# api: "ws" scnattn_sgemm_ws, "sgemm" scnattn_sgemm (no workspace), "cgemm" scnattn_cgemm
# epi: a alpha = 2; b beta = 0.5 onto non-zero C; 1 beta = 1; B bias; m rowmask (zeros in the first row, the last row and the
#      rows around the 64- and 128-row tile boundaries; C0 holds NaN there when beta != 0)
# lay: A1 / B1 / C1 base one float off 16 bytes; lda1 / ldb1 / ldc1 leading dimension % 4 != 0; tn the drivers' batched TN
#      product (csrc/sequence.cpp: lda = batch * M, ldb = batch * N, sA = M, sB = N); colblk a column block of
#      matrices four times as wide (lda = 4 * D with N = F)
# ws:  "full" room for every split the policy may pick; "null"; an int = room for that many slabs
# opts: scnattn_set_option values, and force_mi / force_split of scnattn_conv_extra (api "cgemm")
DENSE = [
    # ---- sgemm_kernel<VEC = false>, all four layouts
    DG("ws", 0, 0, 37, 53, 29, 1, "", "", "full", {}, "sgemm v0 S1", "old test's odd shape, nothing a multiple of 4"),
    DG("ws", 0, 1, 65, 68, 20, 1, "aB", "A1", "full", {}, "sgemm v0 S1", "aligned sizes, A one float off"),
    DG("ws", 1, 0, 129, 132, 15, 1, "b", "", "full", {}, "sgemm v0 S1", "M = 129: one row in the second tile; K = 15"),
    DG("ws", 1, 1, 64, 60, 252, 1, "m", "lda1", "full", {}, "sgemm v0 S1", "lda % 4 != 0"),
    DG("ws", 0, 0, 300, 130, 257, 1, "abBm", "", "full", {}, "sgemm v0 S2", "old test's shape; <= 16 tiles, K >= 256: two slices, the last 113 k"),
    DG("ws", 0, 0, 127, 1, 256, 1, "B", "", "full", {}, "sgemm v0 S2", "tiles <= 16 with K = 256 (kmin 128); N = 1"),
    DG("ws", 1, 0, 196, 132, 512, 5, "ab", "B1", "full", {}, "sgemm v0 S2", "tiles = 20 > 16 with K = 512 (kmin 256); batch 5 with split-K"),
    DG("ws", 1, 1, 63, 4, 2048, 1, "abBm", "C1", 3, {}, "sgemm v0 S3", "workspace for 3 of the policy's 16 slices: kper 688, last slice 672"),
    DG("ws", 0, 1, 1, 700, 96, 1, "B", "ldb1", "full", {}, "sgemm v0 S1", "old test's one-row shape, ldb % 4 != 0"),
    DG("sgemm", 0, 0, 128, 129, 2048, 1, "m", "", "null", {}, "sgemm v0 S1", "no workspace: K = 2048 un-split; N = 129"),
    DG("ws", 1, 0, 9, 12, 7, 5, "1", "tn", "full", {}, "sgemm v0 S1", "old batched test: the drivers' TN form at odd P, beta = 1"),
    # ---- sgemm_kernel<VEC = true>: option use_cgemm = 0
    DG("ws", 0, 0, 128, 128, 64, 1, "", "", "full", {"use_cgemm": 0}, "sgemm v1 S1", "old test's aligned shape"),
    DG("ws", 0, 1, 196, 512, 2048, 1, "abBm", "", "full", {"use_cgemm": 0}, "sgemm v1 S16", "old test's deep shape: 16 slices, splitk_reduce_kernel"),
    DG("ws", 1, 0, 64, 4, 16, 1, "a", "", "full", {"use_cgemm": 0}, "sgemm v1 S1", "N = 4, K = 16"),
    DG("ws", 1, 1, 128, 64, 252, 1, "B", "", "full", {"use_cgemm": 0}, "sgemm v1 S1", "K = 252"),
    DG("ws", 1, 0, 196, 64, 7, 5, "1", "tn", "full", {"use_cgemm": 0}, "sgemm v1 S1", "the drivers' batched TN form, beta = 1"),
    DG("ws", 0, 0, 32, 4608, 512, 1, "b", "", "full", {"use_cgemm": 0}, "sgemm v1 S2", "N = 4608: 36 tiles > 16, K = 512 (kmin 256): two slices"),
    DG("sgemm", 0, 1, 65, 128, 256, 1, "m", "", "null", {"use_cgemm": 0}, "sgemm v1 S1", "scnattn_sgemm: no workspace"),
    # ---- cgemm, 128-row tile (mi = 2), all four layouts
    DG("ws", 0, 0, 64, 64, 16, 1, "", "", "full", {}, "cgemm mi2 S1 - vst", "one k-step"),
    DG("ws", 0, 1, 1, 700, 96, 1, "B", "", "full", {}, "cgemm mi2 S1 - vst", "old test's one-row shape"),
    DG("ws", 1, 0, 4, 128, 252, 1, "b", "", "full", {}, "cgemm mi2 S1 - vst", "M = 4"),
    DG("ws", 1, 1, 64, 132, 20, 1, "abBm", "", "full", {}, "cgemm mi2 S1 - vst", "every epilogue term on the un-split vector epilogue"),
    DG("ws", 0, 1, 63, 128, 2048, 1, "abBm", "", "full", {}, "cgemm mi2 S16 red vst", "16 slices: deeper than cgemm_combine_max -> creduce_kernel<true>"),
    DG("ws", 0, 1, 196, 700, 256, 1, "m", "", "full", {"cgemm_mi": 2}, "cgemm mi2 S2 comb vst", "option cgemm_mi = 2 on a shape that picks 64 rows"),
    DG("cgemm", 0, 0, 196, 128, 64, 1, "B", "", "full", {"force_mi": 2}, "cgemm mi2 S1 - vst", "force_mi = 2"),
    # ---- cgemm, 64-row tile (mi = 1)
    DG("ws", 0, 0, 196, 512, 2048, 1, "abBm", "", "full", {}, "cgemm mi1 S16 red vst", "old test's deep shape: 16 slices -> the reduce launch"),
    DG("ws", 0, 1, 196, 512, 2048, 1, "abBm", "", "full", {}, "cgemm mi1 S16 red vst", "the same call as the sgemm v1 S16 row, on cgemm (use_cgemm 0 vs 1)"),
    DG("ws", 0, 1, 129, 128, 512, 1, "abBm", "", "full", {}, "cgemm mi1 S4 comb vst", "finish_block with bias, beta, rowmask and alpha together"),
    DG("ws", 1, 0, 128, 68, 257, 1, "B", "", "full", {}, "cgemm mi1 S2 comb vst", "K = 257: kper 144, last slice 113"),
    DG("ws", 1, 1, 68, 128, 2048, 1, "b", "", "full", {}, "cgemm mi1 S16 red vst", "TT, 16 slices"),
    DG("ws", 0, 1, 129, 128, 512, 1, "abBm", "", 3, {}, "cgemm mi1 S3 comb vst", "workspace for 3 of the policy's 4 slices: kper 176, last slice 160"),
    DG("ws", 0, 1, 129, 128, 512, 1, "abBm", "", "full", {"cgemm_combine": 0}, "cgemm mi1 S4 red vst", "option cgemm_combine = 0: creduce_kernel<true> at S <= 8"),
    DG("ws", 0, 1, 129, 63, 512, 1, "abBm", "", "full", {}, "cgemm mi4 S4 red sst", "N % 4 != 0 on a tB product (N <= 64: the 128 x 64 tile), split: creduce_kernel<false>"),
    DG("ws", 0, 0, 65, 132, 16, 1, "abBm", "ldc1", "full", {}, "cgemm mi1 S1 - sst", "ldc % 4 != 0: the scalar-store epilogue"),
    DG("ws", 1, 0, 132, 128, 4, 1, "b", "C1", "full", {}, "cgemm mi1 S1 - sst", "C one float off; K = 4"),
    DG("ws", 0, 1, 65, 128, 256, 5, "abBm", "", "full", {}, "cgemm mi1 S2 comb vst", "batch 5 with split-K, gaps between the batches"),
    DG("ws", 1, 0, 128, 68, 100, 1, "a", "colblk", "full", {}, "cgemm mi1 S1 - vst", "the drivers' column-block form: lda = 4 * M, ldb = ldc = 4 * N"),
    DG("sgemm", 0, 1, 196, 512, 2048, 1, "B", "", "null", {}, "cgemm mi1 S1 - vst", "no workspace: K = 2048 un-split"),
    DG("ws", 0, 0, 32, 4608, 512, 1, "b", "", "full", {}, "cgemm mi2 S4 comb vst", "N = 4608, 32 rows"),
    DG("cgemm", 1, 1, 64, 128, 512, 1, "m", "", "full", {"force_mi": 1, "force_split": 2}, "cgemm mi1 S2 comb vst", "force_mi = 1, force_split = 2"),
    DG("ws", 0, 0, 127, 128, 16, 1, "m", "", "full", {"cgemm_mi": 1}, "cgemm mi1 S1 - vst", "option cgemm_mi = 1; M = 127"),
    DG("ws", 0, 1, 65, 63, 16, 1, "B", "", "full", {}, "cgemm mi1 S1 - sst", "scalar store on the NT layout, N = 63"),
    DG("ws", 1, 1, 68, 4, 20, 1, "m", "ldc1", "full", {}, "cgemm mi1 S1 - sst", "scalar store on the TT layout"),
    # ---- scalar stores on the 128-row tile
    DG("ws", 0, 1, 64, 63, 20, 1, "abBm", "", "full", {}, "cgemm mi2 S1 - sst", "scalar store, every epilogue term, N = 63"),
    DG("ws", 1, 0, 4, 132, 16, 1, "B", "C1", "full", {}, "cgemm mi2 S1 - sst", "scalar store on the TN layout, C one float off"),
    DG("ws", 0, 0, 63, 60, 252, 1, "b", "ldc1", "full", {}, "cgemm mi2 S1 - sst", "scalar store on the NN layout"),
    DG("ws", 1, 1, 64, 68, 20, 1, "a", "C1", "full", {}, "cgemm mi2 S1 - sst", "scalar store on the TT layout"),
    # ---- cgemm, 128 x 64 tile (mi = 4)
    DG("ws", 0, 0, 128, 64, 16, 1, "B", "", "full", {}, "cgemm mi4 S1 - vst", "exactly one tile, bias"),
    DG("ws", 0, 1, 196, 60, 256, 1, "abBm", "", "full", {}, "cgemm mi4 S2 comb vst", "bias and rowmask through the combine"),
    DG("ws", 1, 0, 128, 4, 1, 1, "m", "", "full", {}, "cgemm mi4 S1 - vst", "K = 1, N = 4, rowmask"),
    DG("ws", 1, 1, 132, 64, 252, 1, "abBm", "ldc1", "full", {}, "cgemm mi4 S1 - sst", "scalar store, one row block of 4"),
    DG("ws", 1, 0, 196, 64, 7, 5, "1", "tn", "full", {}, "cgemm mi4 S1 - vst", "the drivers' batched TN product: lda = B * P, ldb = B * E, sA = P, sB = E, beta = 1"),
    DG("ws", 0, 0, 128, 64, 16, 1, "b", "C1", "full", {}, "cgemm mi4 S1 - sst", "128 x 64 tile, scalar store on the NN layout"),
    DG("ws", 1, 0, 128, 60, 15, 1, "abBm", "ldc1", "full", {}, "cgemm mi4 S1 - sst", "128 x 64 tile, scalar store on the TN layout"),
    DG("ws", 1, 1, 128, 64, 20, 1, "b", "", "full", {}, "cgemm mi4 S1 - vst", "128 x 64 tile, vector store on the TT layout"),
    DG("cgemm", 0, 1, 129, 128, 20, 1, "aB", "", "full", {"force_mi": 4}, "cgemm mi4 S1 - vst", "force_mi = 4 at N = 128: two column tiles"),
]


def dg_layout(r):
    """leading dimensions, batch strides and base offsets of a DENSE row (elements): ld > width, batch stride > one operand"""
    wA, hA = (r.M, r.K) if r.ta else (r.K, r.M)          # contiguous extent, rows of the stored operand
    wB, hB = (r.K, r.N) if r.tb else (r.N, r.K)
    lay = r.lay.split()
    lda = wA + 4 + (1 if "lda1" in lay else 0)
    ldb = wB + 8 + (1 if "ldb1" in lay else 0)
    ldc = r.N + 4 + (1 if "ldc1" in lay else 0)
    if "colblk" in lay:
        lda, ldb, ldc = 4 * wA, 4 * wB, 4 * r.N
    sA, sB, sC = hA * lda + 8, hB * ldb + 12, r.M * ldc + 8
    if "tn" in lay:
        assert r.ta and not r.tb
        lda, ldb, sA, sB = r.batch * r.M, r.batch * r.N, r.M, r.N
    return dict(lda=lda, ldb=ldb, ldc=ldc, sA=sA, sB=sB, sC=sC, hA=hA, wA=wA, hB=hB, wB=wB,
                misA=int("A1" in lay), misB=int("B1" in lay), misC=int("C1" in lay))


def dg_mask(M):
    m = torch.ones(M)
    for i in (0, 63, 64, 127, 128, M - 1):
        if 0 <= i < M:
            m[i] = 0.0
    return m


def dg_ws_floats(r):
    return 0 if r.ws == "null" else (R_MAX_KSPLIT if r.ws == "full" else r.ws) * r.batch * r.M * r.N


def dg_inputs(r):
    """logical operands and epilogue terms of a DENSE row (fp32 on the CPU)"""
    g = _gen(30000 + 7 * r.M + 3 * r.N + r.K + 2 * r.ta + r.tb + r.batch)
    L = dg_layout(r)
    a = torch.randn(r.batch, L["hA"], L["wA"], generator=g)
    b = torch.randn(r.batch, L["hB"], L["wB"], generator=g)
    alpha = 2.0 if "a" in r.epi else 1.0
    beta = 0.5 if "b" in r.epi else (1.0 if "1" in r.epi else 0.0)
    bias = torch.randn(r.N, generator=g) if "B" in r.epi else None
    mask = dg_mask(r.M) if "m" in r.epi else None
    c0 = torch.randn(r.batch, r.M, r.N, generator=g) if beta != 0.0 else None
    if c0 is not None and mask is not None:
        c0[:, mask == 0] = NAN              # a masked row is 0 whatever C held
    return a, b, alpha, beta, c0, bias, mask


class _Options:
    """scnattn_set_option values of a row, restored to the defaults whatever happens"""

    def __init__(self, opts):
        self.opts = {k: v for k, v in opts.items() if k in OPTION_DEFAULTS}

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
        for k, v in OPTION_DEFAULTS.items():
            set_option(k, v)


def _dense_call(dev, r, opts=None):
    """-> (C [batch, M, N] as read back, guards checked; the fp64 reference; the mask); on the CPU device the launch plan"""
    from scnattn._lib import ConvExtra
    a, b, alpha, beta, c0, bias, mask = dg_inputs(r)
    L = dg_layout(r)
    b_a = GBuf(dev, a.shape, (L["sA"], L["lda"], 1), a, mis=L["misA"])
    b_b = GBuf(dev, b.shape, (L["sB"], L["ldb"], 1), b, mis=L["misB"])
    b_c = GBuf(dev, (r.batch, r.M, r.N), (L["sC"], L["ldc"], 1), c0, out=True, mis=L["misC"])
    b_bias = None if bias is None else GBuf(dev, bias.shape, None, bias)
    b_mask = None if mask is None else GBuf(dev, mask.shape, None, mask)
    nws = dg_ws_floats(r)
    # NaN: a slab read before it is written shows (a plan query touches no memory)
    ws = (torch.empty(nws + 4) if dev.type == "cpu" else torch.full((nws + 4,), NAN, device=dev)) if nws else None
    opts = r.opts if opts is None else opts
    args = [int(r.ta), int(r.tb), r.M, r.N, r.K, C.c_float(alpha), b_a.ptr, L["lda"], b_b.ptr, L["ldb"], C.c_float(beta),
            b_c.ptr, L["ldc"], None if b_bias is None else b_bias.ptr, None if b_mask is None else b_mask.ptr, r.batch,
            L["sA"], L["sB"], L["sC"]]
    if r.api != "sgemm":
        args += [None if ws is None else C.c_void_p(ws.data_ptr()), nws]
    if r.api == "cgemm":
        ex = ConvExtra()
        ex.stride, ex.force_mi, ex.force_split = 1, opts.get("force_mi", 0), opts.get("force_split", 0)
        args.append(C.byref(ex))
    with _Options(opts):
        plan = _call({"ws": "scnattn_sgemm_ws", "sgemm": "scnattn_sgemm", "cgemm": "scnattn_cgemm"}[r.api], dev, *args)
    if dev.type == "cpu":
        return plan
    ref = R.gemm(a.double(), b.double(), bool(r.ta), bool(r.tb), alpha, beta, None if c0 is None else c0.double(),
                 None if bias is None else bias.double(), mask)
    return b_c.read("C"), ref, mask


def dense_plan(r, opts=None):
    return _dense_call(CPU, r, opts)


def _dense_id(r):
    return "%s-%s%s-%dx%dx%d-b%d-%s-%s" % (r.api, "T" if r.ta else "N", "T" if r.tb else "N", r.M, r.N, r.K, r.batch,
                                          r.epi or "plain", r.inst.replace(" ", "_"))


@pytest.mark.parametrize("r", DENSE, ids=_dense_id)
def test_dense_gemm_per_element(dev, r):
    got, ref, mask = _dense_call(dev, r)
    _sum_ok(r.inst, "c", got, ref)
    if mask is not None:
        assert bool((_bits(got[:, mask == 0]) == 0).all()), "a masked row is not +0.0"


# ==== across instances ===================================================================================================
_COMBINE_ROWS = [r for r in DENSE if " comb " in r.inst and not r.opts and ("abBm" in r.epi or r.batch > 1)]


@pytest.mark.parametrize("r", _COMBINE_ROWS, ids=_dense_id)
def test_cgemm_combine_modes_are_bit_identical(dev, r):
    """the reduce launch (cgemm_combine = 0), the write-through combine (1) and the release combine (2) sum the slabs in
    slab order and apply the same epilogue: the same bits"""
    outs = [_bits(_dense_call(dev, r, {"cgemm_combine": mode})[0]) for mode in (0, 1, 2)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


_TWICE_DENSE = [next(r for r in DENSE if r.inst == inst) for inst in
                ("sgemm v0 S2", "sgemm v1 S16", "cgemm mi1 S4 comb vst", "cgemm mi1 S16 red vst", "cgemm mi4 S2 comb vst")]
_TWICE_SKINNY = [next(r for r in SKINNY if r.form == form and r.ks != 1 and "e0" in r.inst) for form in ("f32", "bf16w", "bf16")]


@pytest.mark.parametrize("r", _TWICE_DENSE, ids=_dense_id)
def test_dense_gemm_twice_is_bit_identical(dev, r):
    first, second = _dense_call(dev, r)[0], _dense_call(dev, r)[0]
    assert torch.equal(_bits(first), _bits(second))


@pytest.mark.parametrize("r", _TWICE_SKINNY, ids=lambda r: "%s-%dx%dx%d-ks%d" % (r.form, r.rows, r.N, r.K, r.ks))
def test_skinny_gemm_twice_is_bit_identical(dev, r):
    X, W = _skinny_inputs(r)
    (y1, k1), (y2, k2) = _skinny_call(dev, r, X, W), _skinny_call(dev, r, X, W)
    assert k1 == k2 and torch.equal(_bits(y1), _bits(y2))


def test_use_cgemm_0_and_1_both_meet_the_bound(dev):
    """the deep NT shape on sgemm_kernel<VEC = true> and on cgemm: both within the bound of fp64 (test_dense_gemm_per_element
    judges each); here only that the table holds the pair"""
    pair = [r for r in DENSE if (r.api, r.ta, r.tb, r.M, r.N, r.K, r.epi) == ("ws", 0, 1, 196, 512, 2048, "abBm")]
    assert sorted(r.opts.get("use_cgemm", 1) for r in pair) == [0, 1]
    for r in pair:
        got, ref, _ = _dense_call(dev, r)
        _sum_ok(r.inst, "c", got, ref)


# ==== refusals: host-side argument checks, nothing is launched ===========================================================
def _small_skinny_buffers(dev):
    return (GBuf(dev, (2, 8), None, torch.ones(2, 8)), GBuf(dev, (8, 4), None, torch.ones(8, 4)),
            GBuf(dev, (R_MAX_KSPLIT, 2, 4), None, out=True))


@pytest.mark.parametrize("entry", sorted(SK_ENTRY.values()))
@pytest.mark.parametrize("what,K,ldx,ldw,ks,msg", [
    ("K = 0", 0, 8, 4, 1, "K must be >= 1"),
    ("ksplit = 17", 8, 8, 4, 17, "ksplit out of range"),
    ("K * ldw * 4 >= 2 GiB", 8, 8, 1 << 27, 1, "exceeds the 2 GiB buffer-descriptor range"),
    ("rows * ldx * 4 >= 2 GiB", 8, 1 << 28, 4, 1, "exceeds the 2 GiB buffer-descriptor range"),
])
def test_skinny_gemm_refusals(dev, entry, what, K, ldx, ldw, ks, msg):
    if entry != "scnattn_skinny_gemm" and what.startswith("K * ldw"):
        ldw *= 2                                        # 2-byte weights
    b_x, b_w, b_y = _small_skinny_buffers(dev)
    used = C.c_int(-1)
    with pytest.raises(RuntimeError, match=msg):
        _call(entry, dev, 2, 4, K, 1, b_x.ptr, ldx, 8, b_w.ptr, ldw, 32, b_y.ptr, 4, 8, 8, ks, C.byref(used))
    b_y.read("Y")
    assert _untouched(b_y), what


def test_dense_gemm_refusals(dev):
    from scnattn._lib import ConvExtra
    one = torch.ones(8, 8)
    b_a, b_b, b_a1 = GBuf(dev, (8, 8), None, one), GBuf(dev, (8, 8), None, one), GBuf(dev, (8, 8), None, one, mis=1)
    b_c = GBuf(dev, (8, 8), None, out=True)
    ws = torch.full((8 * 8 * 2,), NAN, device=dev)
    wsp = C.c_void_p(ws.data_ptr())
    one_f, zero_f = C.c_float(1.0), C.c_float(0.0)

    def dense(name, M, K, A, lda, *more):
        _call(name, dev, 0, 0, M, 8, K, one_f, A.ptr, lda, b_b.ptr, 8, zero_f, b_c.ptr, 8, None, None, 1, 0, 0, 0, *more)

    with pytest.raises(RuntimeError, match="sgemm: K must be >= 1"):
        dense("scnattn_sgemm_ws", 8, 0, b_a, 8, wsp, ws.numel())
    with pytest.raises(RuntimeError, match="sgemm: operand exceeds the 2 GiB buffer-descriptor range"):
        dense("scnattn_sgemm", 8, 8, b_a, 1 << 27)      # (M - 1) * lda * 4 >= 2 GiB
    with pytest.raises(RuntimeError, match="cgemm: operand alignment / size not supported"):
        dense("scnattn_cgemm", 8, 8, b_a1, 8, wsp, ws.numel(), None)
    ex = ConvExtra()
    ex.stride, ex.force_split = 1, 4                    # 4 slabs of 8 x 8 do not fit 128 floats
    with pytest.raises(RuntimeError, match="cgemm: forced split does not fit"):
        dense("scnattn_cgemm", 8, 8, b_a, 8, wsp, ws.numel(), C.byref(ex))
    b_c.read("C")
    assert _untouched(b_c) and bool(ws.isnan().all())
