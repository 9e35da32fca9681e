"""fp64 references, case table, inputs, judges and instance names of the bf16 TRAINING convolution kernels:
csrc/cgemm16.hip (cgemm16_kernel EPI 0 / 1 / 2, creduce16_kernel; through scnattn_cgemm16, scnattn_conv3x3_fwd16 and
scnattn_conv3x3_dgrad16), csrc/wgrad16.hip (scnattn_wgrad16_3x3 = w9, scnattn_wgrad16_rows = w1) and scnattn_bf16_weights.
Shared by tests/test_conv16_refs.py (CPU) and tests/test_gpu_conv16_kernels.py; tests/eval16_refs.py (EPI 3) reads plans
through `names` too.

References: the index-arithmetic products of tests/conv_refs.py (conv1x1_* / conv3_* on gather_rows / fwd_taps /
dgrad_taps) on the bf16 operands widened exactly to fp64.  The operands are generated as bf16, so every product term is
exact in fp32 and in fp64; weights are scaled by K^-1/2; BatchNorm vectors are fp32.

Bounds, per element, all derived (none is fitted to a kernel; no element is excluded).  U = 2^-24.

  b = (n + 8) * U * sum|terms|       conv_refs.bound_of: any order of rounded fp32 additions of n exact products (DESIGN.md
                                     3), so it covers split-K slabs summed in slab order and the four-wave meet of the
                                     weight gradients.  With beta = 1 the old C (bf16 widened, or fp32) is one more exact
                                     term: n + 1, its magnitude added to sum|terms|.
  fp32 output (out_bf16 = 0, every weight gradient):      |got - ref| <= b
  bf16 output:                                            |got - ref| <= b + 2^-8 * (|ref| + b)
      the stored value is ONE round-to-nearest-even (8 significant bits, unit roundoff 2^-8) of an fp32 value within b of ref.
  EPI 2 (masked gradient): the mask is decided exactly on the CPU from the widened bf16 z (conv_refs.bn_mask: the sign of
      the fused multiply-add is the sign of its exact argument).  A masked element must be +0.0 bit for bit, an unmasked
      one meets the bf16-output bound.  Partials: every slot against the fp64 sums of the kernel's OWN stored (rounded) g --
      that is what the kernel sums -- with conv_refs.mask_stats_ref / bound_of (n = rows of the slot).
  EPI 1, fp32 output: every slot against the fp64 sums of the kernel's own stored output (conv_refs.stats_ref; un-split the
      stored value is the accumulator, split it is the slab sum the reducer took its statistics from).
  EPI 1, bf16 output: the kernel sums its fp32 accumulators a_i, which the stored bf16 map does not show, so each slot is
      judged against the fp64 sums of the exact d_i = p_i - s (p the exact product, s the shift).  |a_i - p_i| <= b_i, the
      kernel's difference fl(a_i - s) is within b'_i = b_i + U |d_i| of d_i (one more rounding; U |a_i - s| <= U |d_i| + U b_i
      and the second-order U b_i is covered by the + 8 of b_i), and r such terms are then added in fp32:
          slot 1:  |got - sum d_i|   <= sum b_i + (r + 8) U sum |d_i|
          slot 2:  |got - sum d_i^2| <= sum (2 |d_i| b'_i + b'_i^2) + (r + 8) U sum d_i^2
      (in slot 1 the r roundings of the differences, U sum |d_i|, are one of the 8 spare units of (r + 8) U sum |d_i|: r - 1
      additions use r - 1 of them);
      r = rows of the slot.
  Statistics and mask cases: slots [row_tiles(M), stat_ld(M)) of every channel must keep the sentinel (only row_tiles(M)
      slots are live; nothing may write zeros there).
  scnattn_bf16_weights: both copies bit-equal to torch's .to(torch.bfloat16) of the master, plain [Cout][taps][Cin] and
      transposed [Cin][taps][Cout].  No tolerance.

The matrix instruction.  The guides describe the fp32 matrix instruction as a k-ordered fmaf chain and say nothing of how
v_mfma_f32_32x32x16_bf16 rounds its inner 16-term sum.  b assumes round-to-nearest additions (unit roundoff 2^-24).
MFMA_WIDEN is the one admissible widening, the derived factor for TRUNCATING additions (unit roundoff 2^-23): 2, applied to
the matrix-instruction products alone.  It is 1 unless a measurement on the GPU shows an fp32-output instance above b; an
error above 2 b is a kernel bug.  DESIGN.md 3 states which value holds and why.

`names` renders the launch plan of a case's own call (scnattn_plan_next; test_gpu_conv16_kernels.dispatch) as the kernel
instances of the parity report: the launched cgemm16 instance (MI, EPI, GATHER, OBF, C3) and the creduce16<OBF, STATS>
that follows, or the wave-split weight gradient with its Q, ntiles and S.  The policy itself is stated once, in
cgemm16_plan (csrc/cgemm16.hip) and wgrad_split (csrc/tile.h)."""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_refs as CR
from scnattn import _lib as L

BF = torch.bfloat16
U = CR.U
U8 = 2.0 ** -8
MFMA_WIDEN = 1.0
WS_FLOATS = 4 << 20         # the split workspace the GPU test passes
SENT32 = 0x7FC5A5A5         # kernel_harness.SENT
SENT16 = 0x7FC5

cdiv = CR.cdiv


# ==== instance names, rendered from the launch plan of the real call (scnattn_plan_next) ===============================
def names(p):
    """launch plan -> dict(names = the kernel instances in launch order, S, and per family: cgemm16 mi, kper, tiles, inst =
    (MI, EPI, GATHER, OBF, C3) of the product launch, reduce = (OBF, STATS) of the creduce16 that follows | 'eval' | None;
    wave-split weight gradients kernel = 'w9' | 'w1', Q, ntiles)"""
    if p.family in (L.PLAN_WGRAD16_W9, L.PLAN_WGRAD16_W1):
        kernel = "w9" if p.family == L.PLAN_WGRAD16_W9 else "w1"
        assert (p.second == L.SECOND_CGEMM_REDUCE) == (p.S > 1)
        return dict(kernel=kernel, Q=p.Q, ntiles=p.ntiles, S=p.S, names=["wgrad16_%s (S %s 1)" % (kernel, ">" if p.S > 1 else "=")])
    assert p.family == L.PLAN_CGEMM16 and (p.second == L.SECOND_CREDUCE16) == (p.S > 1)
    obf = bool(p.out_bf16)
    d = dict(mi=p.mi, S=p.S, kper=p.kper, tiles=p.tiles, inst=(p.mi, p.epi, bool(p.gather), obf, p.c3), reduce=None,
             names=["cgemm16<MI %d, EPI %d, %s, %s, C3 %d>" % (p.mi, p.epi, "gather" if p.gather else "plain",
                                                               "bf16" if obf else "fp32", p.c3)])
    if p.second:
        d["reduce"] = "eval" if p.second_mode == 2 else (obf, p.second_mode == 1)
        if p.second_mode != 2:
            d["names"].append("creduce16<%s, %s>" % ("bf16" if obf else "fp32", "stats" if p.second_mode == 1 else "plain"))
    return d


# ==== cases ==============================================================================================================
# op:  f1 1x1 forward (s > 1: rows gathered from the N x Hi x Wi map) / d1 1x1 d input (B = the transposed weight copy) through
#      scnattn_cgemm16 with lda = K + 8, ldb = K + 8, ldc = N + 8 (bf16) / N + 4 (fp32), ldz = N + 8;
#      f3 / d3 / s3: scnattn_conv3x3_fwd16 / _dgrad16 stride 1 (`flip`) / _dgrad16 stride 2 (C3 4);
#      w9 scnattn_wgrad16_3x3;  w1 scnattn_wgrad16_rows: plain (s = 1), the gathered downsample (s = 2), var "t": the nine
#      taps of a stride-2 3x3 written into one [Cout][9][Cin] window.
# N, Hi, Wi: the INPUT map; an un-gathered product of R rows is N = R maps of 1 x 1.  epi: 0 / 1 / 2.
# var: s stat_shift given, b beta = 1.  mi / split: force_mi / force_split (w9, w1: k_slices).  obf: bf16 output.
Case = namedtuple("Case", "op N Hi Wi Cin Cout s epi var mi split obf")


def case(op, N, Hi, Wi, Cin, Cout, s=1, epi=0, var="", mi=0, split=0, obf=1):
    return Case(op, N, Hi, Wi, Cin, Cout, s, epi, var, mi, split, obf)


def case_id(c):
    return "%s-%dx%dx%d-%dto%d-s%d-e%d%s-mi%d-S%d-%s" % (c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, c.epi, c.var, c.mi, c.split,
                                                         "bf16" if c.obf else "fp32")


def out_hw(c):
    return (c.Hi - 1) // c.s + 1, (c.Wi - 1) // c.s + 1


def rows_in(c):
    return c.N * c.Hi * c.Wi


def rows_out(c):
    Ho, Wo = out_hw(c)
    return c.N * Ho * Wo


def gemm_of(c):
    """the product a cgemm16 case launches -> dict(M, N, K, c3, gather)"""
    Ri, Ro = rows_in(c), rows_out(c)
    return {"f1": dict(M=Ro, N=c.Cout, K=c.Cin, c3=0, gather=c.s > 1), "d1": dict(M=Ri, N=c.Cin, K=c.Cout, c3=0, gather=False),
            "f3": dict(M=Ro, N=c.Cout, K=9 * c.Cin, c3=1, gather=False), "d3": dict(M=Ri, N=c.Cin, K=9 * c.Cout, c3=1, gather=False),
            "s3": dict(M=Ro, N=c.Cin, K=9 * c.Cout, c3=4, gather=False)}[c.op]


def out_shape(c):
    if c.op in ("f1", "f3"):
        return rows_out(c), c.Cout
    if c.op in ("d1", "d3", "s3"):
        return rows_in(c), c.Cin
    return c.Cout, (9 if c.op == "w9" or "t" in c.var else 1) * c.Cin


# ---- the table: the smallest shapes at which a path can go wrong ----------------------------------------------------------
MS, NS, KS = (16, 64, 65, 129, 200), (8, 72, 136, 256), (8, 40, 64, 1024)
MODES = (("", 0), ("b", 0), ("", 1), ("s", 1))         # (var, epi): plain, beta = 1, statistics without / with a shift


def _variants(op, M, Nn, K, t, split_of):
    """the eight (mode x output type) forms of one product, the row tile cycling 1 / 2 / policy"""
    rows = []
    for v in range(8):
        var, epi = MODES[v % 4]
        Cin, Cout = (K, Nn) if op == "f1" else (Nn, K)
        rows.append(case(op, M, 1, 1, Cin, Cout, epi=epi, var=var, mi=(1, 2, 0)[(v + t) % 3], split=split_of(v), obf=1 - v // 4))
    return rows


def _gemm_cases():
    rows, t = [], 0
    for i, M in enumerate(MS):            # every (M, N), (M, K) and (N, K) pair occurs
        for j, Nn in enumerate(NS):
            K = KS[(i + j) % 4]
            # K = 1024 with a workspace is split by the policy: force_split = 1 keeps every second form in one launch
            rows += _variants("f1" if t % 2 == 0 else "d1", M, Nn, K, t, lambda v: 1 if (K >= 512 and (v + t) % 2 == 0) else 0)
            t += 1
    for (M, Nn) in ((200, 256), (65, 72), (16, 136), (129, 8), (64, 72)):       # forced 2 / 4 at K = 1024
        for S in (2, 4):
            rows += _variants("f1", M, Nn, 1024, t, lambda v: S)
            t += 1
    for (M, Nn, K) in ((65, 72, 40), (200, 136, 40), (65, 72, 72), (129, 256, 72)):    # the second slab 8 deep; kper 64
        rows += _variants("d1" if K == 72 else "f1", M, Nn, K, t, lambda v: 2)
        t += 1
    return rows


def _gather_cases():
    rows = []
    G = dict(N=3, Hi=7, Wi=5, s=2)              # odd maps: 3 x 7 x 5 -> 4 x 3, 36 rows
    k = 0
    for (Cin, Cout) in ((40, 72), (64, 136), (1024, 8), (8, 256)):
        for v in range(8):
            var, epi = MODES[v % 4]
            split = (1, 2, 0)[k % 3] if Cin == 1024 else 0
            rows.append(case("f1", Cin=Cin, Cout=Cout, epi=epi, var=var, mi=(1, 2, 0)[k % 3], split=split, obf=1 - v // 4, **G))
            k += 1
    return rows


def _mask_cases():
    rows, k = [], 0
    for i, M in enumerate(MS):
        for j, Nn in enumerate(NS):
            K = KS[(i + j + 1) % 4]
            rows.append(case("d1", M, 1, 1, Nn, K, epi=2, mi=(1, 2, 0)[k % 3]))
            rows.append(case("d1", M, 1, 1, Nn, K, epi=2, mi=(2, 0, 1)[k % 3]))
            k += 1
    for (N, H, W) in ((2, 3, 5), (3, 7, 7), (1, 1, 1)):
        for (Cin, Cout) in ((8, 32), (72, 64), (136, 32)):
            for mi in (1, 2):
                rows.append(case("d3", N, H, W, Cin, Cout, epi=2, mi=mi))
            rows.append(case("d3", N, H, W, Cin, Cout, epi=0, mi=(1, 2)[k % 2], split=(0, 2)[(k // 2) % 2]))     # the plain stride-1 d input
            k += 1
    return rows


def _f3_cases():
    rows, k = [], 0
    for (N, H, W, s) in ((1, 1, 1, 1), (2, 3, 5, 1), (2, 5, 4, 2), (3, 7, 7, 1)):
        for Cin in (32, 64, 96):                # K = 288 / 576 / 864: the policy splits the last two
            for Cout in (8, 72):
                for epi, var in ((0, ""), (1, "s" if k % 2 else "")):
                    rows.append(case("f3", N, H, W, Cin, Cout, s=s, epi=epi, var=var, mi=(1, 2, 0)[k % 3], split=(0, 1, 2, 3)[k % 4]))
                    k += 1
    return rows


def _s3_cases():
    rows = []
    for (N, H, W) in ((1, 2, 2), (2, 4, 6), (3, 8, 4)):
        for Cout in (32, 64):
            for Cin in (8, 72):
                rows += [case("s3", N, H, W, Cin, Cout, s=2, mi=mi) for mi in (1, 2)]
    rows.append(case("s3", 3, 8, 4, 72, 64, s=2))
    return rows


W9_MAPS = ((1, 1, 3), (1, 5, 1), (2, 3, 16), (2, 2, 17), (2, 2, 32), (2, 9, 20), (4, 8, 16))
CH32 = ((32, 64), (64, 32), (96, 32), (32, 96), (64, 96), (96, 64))


def _w9_cases():
    rows = []
    for i, (N, H, W) in enumerate(W9_MAPS):
        smax = max((N * cdiv(W, 16) * H) // 16, 1)          # every k_slices the clamp allows
        for ksl in [0, 1] + list(range(2, smax + 1)):
            Cin, Cout = CH32[(i + ksl) % len(CH32)]
            rows.append(case("w9", N, H, W, Cin, Cout, split=ksl, obf=0))
    return rows


def _w1_cases():
    rows = []
    chans = ((64, 64), (128, 64), (64, 192), (192, 128), (128, 128))
    # rows 16 ... 257 hold fewer than 32 lines, so the clamp allows no split there; 500 rows (32 lines, the last one 4 deep) is
    # the smallest table entry at which k_slices = 2 survives it
    for i, R in enumerate((16, 17, 37, 100, 257, 500)):
        smax = max(cdiv(R, 16) // 16, 1)
        for ksl in [0, 1] + list(range(2, min(smax, 2) + 1)):
            Cin, Cout = chans[(i + ksl) % len(chans)]
            rows.append(case("w1", R, 1, 1, Cin, Cout, split=ksl, obf=0))
    G = dict(N=3, Hi=7, Wi=5, s=2)
    rows += [case("w1", Cin=64, Cout=128, obf=0, **G), case("w1", Cin=192, Cout=64, split=1, obf=0, **G),
             case("w1", Cin=64, Cout=64, var="t", obf=0, **G), case("w1", Cin=128, Cout=64, var="t", split=1, obf=0, **G)]
    return rows


CASES = list({case_id(c): c for c in _gemm_cases() + _gather_cases() + _mask_cases() + _f3_cases() + _s3_cases() + _w9_cases() +
              _w1_cases()}.values())


# ==== inputs =============================================================================================================
def _bf16_neighbour(v, up):
    """the bf16 value next to the bf16-representable v (non-zero), above (up) or below"""
    bits = int(torch.tensor(float(v)).to(BF).view(torch.int16))
    bits += 1 if (float(v) > 0) == bool(up) else -1
    return float(torch.tensor(bits, dtype=torch.int16).view(BF).float())


def is_bf16(t):
    return bool((t.to(BF).float() == t).all())


def _plant_bf16(z32, mean, invstd, gamma, beta):
    """conv_refs._plant_mask_edges on the widened z (an expression that is exactly 0 -> masked, one step either side of it,
    the fused-versus-unfused residual in channel 4); every planted z that bf16 cannot hold -- the fp32 neighbours of the zero
    -- moves to the bf16 neighbour of the zero on the same side."""
    zero_at = mean.clone()
    CR._plant_mask_edges(z32, gamma, beta, lambda zz: CR.bn_mask(zz, mean, invstd, gamma, beta, False)[1], zero_at)
    bad = (z32.to(BF).float() != z32).nonzero()
    for r, ch in bad.tolist():
        z32[r, ch] = _bf16_neighbour(zero_at[ch], bool(z32[r, ch] > zero_at[ch]))
    assert is_bf16(z32), "a planted z is not representable in bf16"
    return z32.to(BF)


_INPUTS = {}


def inputs(c):
    """seeded bf16 operands of a case (shared by every form of the same op and shape) and the fp32 vectors"""
    key = (c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s)
    if key in _INPUTS:
        return _INPUTS[key]
    g = torch.Generator().manual_seed(70000 + zlib.crc32(repr(key).encode()) % 100000)
    Ri, Ro = rows_in(c), rows_out(c)
    I = {"x": torch.randn(Ri, c.Cin, generator=g).to(BF), "dy": torch.randn(Ro, c.Cout, generator=g).to(BF)}
    taps = 9 if c.op in ("f3", "d3", "s3") else 1
    if c.op in ("f1", "d1", "f3", "d3", "s3"):
        K = taps * (c.Cin if c.op in ("f1", "f3") else c.Cout)
        I["w"] = (torch.randn(c.Cout, taps, c.Cin, generator=g) * K ** -0.5).to(BF)      # [Cout][taps][Cin]
        I["wt"] = I["w"].permute(2, 1, 0).contiguous()                                    # [Cin][taps][Cout]
        M, Nc = out_shape(c)
        I["c0"] = torch.randn(M, Nc, generator=g).to(BF)                                  # the old C of beta = 1 (bf16; fp32: below)
        I["c0f"] = torch.randn(M, Nc, generator=g)
        I["shift"] = 0.1 * torch.randn(Nc, generator=g)
    if c.op in ("d1", "d3"):                    # the consumer BatchNorm of the mask epilogue (channel = Cin of the d input)
        z32 = torch.randn(Ri, c.Cin, generator=g).to(BF).float()
        mean = (0.1 * torch.randn(c.Cin, generator=g) + 0.3).to(BF).float()             # bf16 values: z = mean is representable
        I["invstd"] = 1 + 0.2 * torch.rand(c.Cin, generator=g)
        gamma = 1 + 0.3 * torch.randn(c.Cin, generator=g)
        gamma[1::2] *= -1                                                                 # both signs
        beta = 0.2 * torch.randn(c.Cin, generator=g)
        I["z"] = _plant_bf16(z32, mean, I["invstd"], gamma, beta)
        I["mean"], I["gamma"], I["beta"] = mean, gamma, beta
    _INPUTS[key] = I
    return I


# ==== references =========================================================================================================
def tap_rows(N, Hi, Wi, s, goh, gow, wrap=False):
    """source row of scnattn_wgrad16_rows for output row (n, ho, wo): pixel (ho * s + goh, wo * s + gow) of the Hi x Wi map, -1
    outside the image.  wrap plants the defect of a missing horizontal check: the linear index of the neighbouring line."""
    n, ho, wo = CR._grid(N, (Hi - 1) // s + 1, (Wi - 1) // s + 1)
    hi, wi = ho * s + goh, wo * s + gow
    ok = (hi >= 0) & (hi < Hi)
    lin = (n * Hi + hi) * Wi + wi
    ok = ok & ((lin >= 0) & (lin < N * Hi * Wi) if wrap else (wi >= 0) & (wi < Wi))
    return torch.where(ok, lin, torch.full_like(n, -1))


def _gather_idx(c, wrong_width=False):
    if c.s == 1:
        return None
    if not wrong_width:
        return CR.gather_rows(c.N, c.Hi, c.Wi, c.s)
    Ho, Wo = out_hw(c)                           # the defect: Wo used for Wi
    n, ho, wo = CR._grid(c.N, Ho, Wo)
    return (n * c.Hi + ho * c.s) * Wo + wo * c.s


def product(c, I, dt=torch.float64):
    """the product of a case in dtype dt from the index tables -> out / out_abs / out_n (without beta)"""
    x, dy = I["x"].to(dt), I["dy"].to(dt)
    if c.op == "f1":
        return CR.conv1x1_fwd(x, I["w"][:, 0].to(dt), _gather_idx(c))
    if c.op == "d1":
        return CR.conv1x1_dgrad(dy, I["w"][:, 0].to(dt))
    if c.op == "f3":
        return CR.conv3_fwd(x, I["w"].to(dt), CR.fwd_taps(c.N, c.Hi, c.Wi, c.s))
    if c.op in ("d3", "s3"):
        return CR.conv3_dgrad(dy, I["w"].to(dt), CR.dgrad_taps(c.N, c.Hi, c.Wi, c.s))
    if c.op == "w9":
        return CR.conv3_wgrad(dy, x, CR.fwd_taps(c.N, c.Hi, c.Wi, 1), per_tap=True)
    if "t" in c.var:                              # nine launches, tap t = (dh, dw): goh = dh - 1, gow = dw - 1
        idx = torch.stack([tap_rows(c.N, c.Hi, c.Wi, c.s, t // 3 - 1, t % 3 - 1) for t in range(9)], 1)
        return CR.conv3_wgrad(dy, x, idx, per_tap=True)
    return CR.conv1x1_wgrad(dy, x, _gather_idx(c))


_REFS = {}


def reference(c, I=None):
    """fp64 reference of the stored product (with the old C of beta = 1): out / out_abs / out_n, computed once per product"""
    key = (c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, "t" in c.var)
    I = inputs(c) if I is None else I
    if key not in _REFS:
        _REFS[key] = product(c, I)
    r = dict(_REFS[key])
    if "b" in c.var:
        c0 = (I["c0"] if c.obf else I["c0f"]).double()
        r = {"out": r["out"] + c0, "out_abs": r["out_abs"] + c0.abs(), "out_n": r["out_n"] + 1}
    return r


def torch_product(c, I, dt):
    """The same products from torch's own operators (F.conv2d, conv_transpose2d, aten.convolution_backward, strided views)
    in dtype dt: fp64 checks the index references, fp32 is the CPU evaluation the judges must accept."""
    x, dy = I["x"].to(dt), I["dy"].to(dt)
    Ho, Wo = out_hw(c)
    nhwc = lambda t, H, W: t.view(c.N, H, W, -1).permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    if c.op == "f1":
        xs = x if c.s == 1 else x.view(c.N, c.Hi, c.Wi, -1)[:, ::c.s, ::c.s].reshape(-1, c.Cin)
        return xs @ I["w"][:, 0].to(dt).t()
    if c.op == "d1":
        return dy @ I["w"][:, 0].to(dt)
    w4 = None if "w" not in I else I["w"].to(dt).view(c.Cout, 3, 3, c.Cin).permute(0, 3, 1, 2) if I["w"].shape[1] == 9 else None
    if c.op == "f3":
        return rows(F.conv2d(nhwc(x, c.Hi, c.Wi), w4, stride=c.s, padding=1))
    if c.op in ("d3", "s3"):
        op = (c.Hi - ((Ho - 1) * c.s + 1), c.Wi - ((Wo - 1) * c.s + 1))
        return rows(F.conv_transpose2d(nhwc(dy, Ho, Wo), w4, stride=c.s, padding=1, output_padding=op))
    if c.op == "w9" or "t" in c.var:
        s = 1 if c.op == "w9" else c.s
        gw = torch.ops.aten.convolution_backward(nhwc(dy, Ho, Wo).contiguous(), nhwc(x, c.Hi, c.Wi).contiguous(),
                                                 torch.zeros(c.Cout, c.Cin, 3, 3, dtype=dt), None, [s, s], [1, 1], [1, 1], False,
                                                 [0, 0], 1, [False, True, False])[1]
        return gw.permute(0, 2, 3, 1).reshape(c.Cout, 9 * c.Cin)
    xs = x if c.s == 1 else x.view(c.N, c.Hi, c.Wi, -1)[:, ::c.s, ::c.s].reshape(-1, c.Cin)
    return dy.t() @ xs


# ==== judging ============================================================================================================
def _ratio(err, bound):
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30).nan_to_num(1e30)


def stats_bf16_ref(ref, shift, b):
    """EPI 1 under a bf16 output: fp64 sums of the exact d = p - s per 64-row slot and the bound propagated through the sums
    (module docstring) -> (want [2][C][mt], bound [2][C][mt])"""
    d = ref["out"] - (0.0 if shift is None else shift.double())
    r = CR.block_rows(d.shape[0])[0]                               # [1][mt]
    bp = b + U * d.abs()
    want = torch.stack([CR.block_sums(d), CR.block_sums(d * d)])
    bound = torch.stack([CR.block_sums(b) + (r + 8) * U * CR.block_sums(d.abs()),
                         CR.block_sums(2 * d.abs() * bp + bp * bp) + (r + 8) * U * CR.block_sums(d * d)])
    return want, bound


def judge(c, I, got):
    """got = dict(out = the stored [rows][cols] map (bf16 or fp32), part = the whole [2][C][stat_ld] partial array or None)
    of the kernel or of any other evaluation -> (ok, {result: worst err / bound}, [what failed]).  No element is excluded."""
    ref = reference(c, I)
    b = CR.bound_of(ref) * MFMA_WIDEN
    out = got["out"]
    want = ref["out"]
    bound = b + U8 * (want.abs() + b) if c.obf else b
    fails, ratios = [], {}
    on = xhat = None
    if c.epi == 2:
        on, xhat = CR.bn_mask(I["z"].float(), I["mean"], I["invstd"], I["gamma"], I["beta"], False)
        zero = torch.zeros((), dtype=torch.float64)
        want, bound = torch.where(on, want, zero), torch.where(on, bound, zero)
        if not bool((out.contiguous().view(torch.int16)[~on] == 0).all()):
            fails.append("a masked element is not +0.0")
    err = (out.double() - want).abs()
    ratios["out"] = float(_ratio(err, bound).max())
    if not bool((err <= bound).all()):
        fails.append("out: worst err/bound %.3f, %d NaN" % (ratios["out"], int(out.float().isnan().sum())))
    if c.epi in (1, 2):
        part = got["part"]
        M = out.shape[0]
        mt, ld = CR.row_tiles(M), CR.stat_ld(M)
        assert tuple(part.shape) == (2, out.shape[1], ld)
        live = part[:, :, :mt]
        if not bool((part[:, :, mt:].contiguous().view(torch.int32) == SENT32).all()):
            fails.append("a partial slot in [row_tiles, stat_ld) lost the sentinel")
        shift = I["shift"] if "s" in c.var else None
        if c.epi == 2:
            s = CR.mask_stats_ref(out.float(), xhat)
            swant, sbound = s["out"], CR.bound_of(s)
        elif not c.obf:
            s = CR.stats_ref(out, shift)
            swant, sbound = s["out"], CR.bound_of(s)
        else:
            swant, sbound = stats_bf16_ref(ref, shift, b)
        serr = (live.double() - swant).abs()
        name = "sums" if c.epi == 2 else "stats"
        ratios[name] = float(_ratio(serr, sbound.expand(swant.shape)).max())
        if not bool((serr <= sbound).all()):
            fails.append("%s: worst err/bound %.3f, %d NaN" % (name, ratios[name], int(live.isnan().sum())))
    return not fails, ratios, fails


# ==== torch's own evaluation on the CPU, and the planted defects =========================================================
DEFECTS = ("k_granule", "truncate", "pad_row_stats", "slot_tm", "mask_ge", "mask_unfused", "sums_unrounded", "s3_class_missing",
           "gather_wo", "w1_tap_wrap", "w9_seg16")           # + "wt_swap" on the weight copies (cv_eval)


def applies(defect, c):
    M = out_shape(c)[0]
    if defect == "k_granule":                   # on a 1 x 1 map the last tap lies outside the image: its k multiply padding
        return not (c.op in ("f3", "d3") and c.Hi * c.Wi == 1)
    if defect == "truncate":
        return bool(c.obf)
    if defect == "pad_row_stats":
        return c.epi == 1 and "s" in c.var and M % 64 != 0
    if defect == "slot_tm":
        from test_gpu_conv16_kernels import dispatch        # the row tile and the split the library plans for the case
        return c.epi in (1, 2) and M > 64 and dispatch(c)["mi"] == 2 and dispatch(c)["S"] == 1
    if defect in ("mask_ge", "sums_unrounded"):
        return c.epi == 2 and c.Cin >= 8
    if defect == "mask_unfused":                # the residual is planted at a row past the first three
        return c.epi == 2 and c.Cin >= 8 and M > 3
    if defect == "s3_class_missing":
        return c.op == "s3"
    if defect == "gather_wo":
        return c.op in ("f1", "w1") and c.s > 1 and "t" not in c.var
    if defect == "w1_tap_wrap":
        return c.op == "w1" and "t" in c.var
    if defect == "w9_seg16":
        return c.op == "w9" and c.Wi % 16 != 0 and c.N * c.Hi > 1
    raise ValueError(defect)


def _sent_part(C, M):
    return torch.full((2, C, CR.stat_ld(M)), SENT32, dtype=torch.int32).view(torch.float32).clone()


def _truncate(y):
    return (y.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def cpu_eval(c, I, defect=None):
    """fp32 matmul / convolution of the widened operands by torch's own operators, the epilogue in fp32 steps, .bfloat16()
    where the kernel stores bf16 -> dict(out, part); `defect` plants one defect."""
    J = dict(I)
    if defect == "k_granule":                   # the last 8 k of the last slab never added
        if c.op in ("w9", "w1"):
            J["dy"] = I["dy"].clone()
            J["dy"][-8:] = 0
        elif c.op in ("f1", "f3"):
            J["w"] = I["w"].clone()
            J["w"][:, -1, -8:] = 0
        else:                                   # d input: k runs over (tap, Cout); the `flip` walks the taps backwards
            J["w"] = I["w"].clone()
            J["w"][-8:, 0 if c.op == "d3" else -1, :] = 0
    f32 = torch.float32
    if defect == "gather_wo":
        rows = _gather_idx(c, True).clamp_max(rows_in(c) - 1)
        xs = J["x"].float()[rows]
        P = xs @ J["w"][:, 0].float().t() if c.op == "f1" else J["dy"].float().t() @ xs
    elif defect == "w1_tap_wrap":
        idx = torch.stack([tap_rows(c.N, c.Hi, c.Wi, c.s, t // 3 - 1, t % 3 - 1, wrap=True) for t in range(9)], 1)
        P = CR.conv3_wgrad(J["dy"].float(), J["x"].float(), idx)["out"]
    else:
        P = torch_product(c, J, f32)
    if defect == "w9_seg16":                    # the last segment of every line summed over 16 pixels: the pixels past W are
        x, dy = J["x"].float(), J["dy"].float()  # the next line's (what lies there in memory)
        rows = rows_in(c)
        P = P.clone().view(c.Cout, 9, c.Cin)
        for n in range(c.N):
            for h in range(c.Hi):
                for w in range(c.Wi, cdiv(c.Wi, 16) * 16):
                    r = (n * c.Hi + h) * c.Wi + w
                    if r >= rows:
                        continue
                    for t in range(9):
                        hx, rx = h + t // 3 - 1, (n * c.Hi + h + t // 3 - 1) * c.Wi + w + t % 3 - 1
                        if 0 <= hx < c.Hi and 0 <= rx < rows:
                            P[:, t] += torch.outer(dy[r], x[rx])
        P = P.view(c.Cout, 9 * c.Cin)
    if "b" in c.var:
        P = P + (I["c0"] if c.obf else I["c0f"]).float()
    M, Nc = P.shape
    part = None
    if c.epi == 1:
        d = P - I["shift"] if "s" in c.var else P
        live = torch.stack([CR.block_sums(d), CR.block_sums(d * d)])
        if defect == "pad_row_stats":           # one padding row's (0 - s) in the last slot
            live[0, :, -1] -= I["shift"]
            live[1, :, -1] += I["shift"] * I["shift"]
    if c.epi == 2:
        on, xhat = CR.bn_mask(I["z"].float(), I["mean"], I["invstd"], I["gamma"], I["beta"], False)
        if defect == "mask_ge":
            on = xhat.double() * I["gamma"].double() + I["beta"].double() >= 0
        if defect == "mask_unfused":
            on = torch.from_numpy((xhat.numpy() * I["gamma"].numpy()).astype(np.float32) + I["beta"].numpy() > 0)
        P = torch.where(on, P, torch.zeros(()))
        gs = P if defect == "sums_unrounded" else (_truncate(P) if defect == "truncate" else P.to(BF)).float()
        live = torch.stack([CR.block_sums(gs), CR.block_sums(gs * xhat)])
    if c.epi in (1, 2):
        part = _sent_part(Nc, M)
        mt = CR.row_tiles(M)
        if defect == "slot_tm":                 # a 128-row tile's two wave rows both write slot tm
            for j in range(mt):
                part[:, :, j // 2] = live[:, :, j]
        else:
            part[:, :, :mt] = live
    out = (_truncate(P) if defect == "truncate" else P.to(BF)) if c.obf else P
    if defect == "s3_class_missing":            # parity class (1, 0) never stored: the sentinel stays
        Ho, Wo = out_hw(c)
        n, hi, wi = CR._grid(c.N, c.Hi, c.Wi)
        out = out.clone()
        out.view(torch.int16)[(hi % 2 == 1) & (wi % 2 == 0)] = SENT16
    return dict(out=out, part=part)


# ==== scnattn_bf16_weights ===============================================================================================
CV_WEIGHTS = ((32, 1, 96), (96, 9, 32), (64, 9, 64), (96, 1, 32))     # (cout, taps, cin)


def cv_masters():
    """fp32 masters [cout][taps][cin] holding, among random values: exact ties to even in both directions, the values one
    fp32 step either side of a tie, the largest finite value (rounds to infinity), subnormals, -0.0 and a NaN"""
    g = torch.Generator().manual_seed(9016)
    tie_down, tie_up = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8           # between 1 and 1 + 2^-7 -> 1; between 1 + 2^-7 and 1 + 2^-6 -> 1 + 2^-6
    f = lambda v: np.float32(v)
    special = [tie_down, tie_up, -tie_down, -tie_up,
               np.nextafter(f(tie_down), f(2)), np.nextafter(f(tie_down), f(0)), np.nextafter(f(tie_up), f(2)), np.nextafter(f(tie_up), f(0)),
               np.finfo(np.float32).max, -np.finfo(np.float32).max, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -133 + 2.0 ** -141, -0.0, 0.0,
               float("nan"), float("inf")]
    out = []
    for (co, taps, ci) in CV_WEIGHTS:
        w = torch.randn(co, taps, ci, generator=g) * 0.05
        sp = torch.tensor([float(v) for v in special], dtype=torch.float32)
        pos = torch.randperm(w.numel(), generator=g)[:4 * sp.numel()]
        w.view(-1)[pos] = sp.repeat(4)
        w[co - 1, taps - 1, ci - 4:] = sp[:4]                                # the last corner of the last tile too
        out.append(w)
    return out


def cv_expected(w):
    """((plain, transposed), (plain, transposed)): int16 bit patterns of torch's own .to(bfloat16) of the master, [cout][taps][cin]
    and [cin][taps][cout], taken twice: of the whole tensor, and with every NaN master converted as a 0-dim tensor.  torch
    leaves the pattern of a converted NaN to the route: on an AVX-512 CPU the vector loop gives 0xFFFF and the scalar route (a
    0-dim tensor, the tail of the loop) 0x7FC0 for the same 0x7FC00000, so at a NaN master either pattern is torch's.  On
    every number there is one conversion and no choice."""
    main = w.to(BF)
    alt = main.clone()
    for idx in w.isnan().nonzero().tolist():
        alt[tuple(idx)] = w[tuple(idx)].to(BF)
    return [(b.contiguous().view(torch.int16), b.permute(2, 1, 0).contiguous().view(torch.int16)) for b in (main, alt)]


def cv_eval(w, defect=None):
    b = _truncate(w) if defect == "truncate" else w.to(BF)
    t = b.permute(2, 0, 1) if defect == "wt_swap" else b.permute(2, 1, 0)      # wt_swap: [cin][cout][taps]
    return b.contiguous().view(torch.int16), t.contiguous().view(torch.int16).reshape(w.shape[2], w.shape[1], w.shape[0])


def cv_mismatch(w, got, which):
    """flat positions where copy `which` (0 plain, 1 transposed) is neither of torch's conversions"""
    a, b = (e[which].reshape(-1) for e in cv_expected(w))
    g = got.reshape(-1)
    return ((g != a) & (g != b)).nonzero().reshape(-1)


def cv_judge(w, got):
    return cv_mismatch(w, got[0], 0).numel() == 0 and cv_mismatch(w, got[1], 1).numel() == 0
