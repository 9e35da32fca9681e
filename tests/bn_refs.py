"""fp64 references of the BatchNorm kernels of csrc/batchnorm.hip (include/scnattn.h: scnattn_bn_stats / _stats_fold /
_apply / _bwd, the chunk-major family, and scnattn_bn_finalize / _apply_fin / _bwd_reduce / _bwd_dx_fin, the finalize-on-load
family), the case tables of tests/test_gpu_bn_kernels.py, their seeded inputs, the judges, and Python mirrors of the host
dispatch (row_chunks / pick_chunks / ew_chunks / ew_blocks, the variant choice of bn_bwd_t and of bn_bwd_reduce_t).

A judge takes what a kernel -- or any other evaluation, tests/test_bn_stem_refs.py uses torch's CPU fp32 -- stored, as fp32
tensors (a bf16 map widened), and a callback ok(kernel, name, got, want, bound, kind) (kernel_harness._bound_ok).  Nothing
is excluded; u = 2^-24.  The tiers:
  * partial slots: each slot against the fp64 sum over exactly the rows the mirror assigns to it, (n + 8) u sum|terms|;
  * finalize outputs: fp64 arithmetic on the partials actually summed (the kernel's own stored slots, or the input partials);
    n = chunk count, A1 / A2 = sum|slot|:  bm1 = (n + 8) u A1 / R, mean within bm1 + 2 u |mean|,
    bvar = (n + 8) u A2 / R + 2 |m1| bm1 + bm1^2 + 4 u m1^2, invstd inside
    [rsqrt(var + bvar + eps) (1 - k u), rsqrt(max(var - bvar, 0) + eps) (1 + k u)], k = RSQRT_ULP;
    running statistics, folded scale / shift, dbeta / dgamma as written at judge_finalize / judge_param_grads;
  * element-wise maps against fp64 on the STORED fp32 statistics: y within 4 u (|xhat gamma| + |beta| + |res|) (the ReLU,
    1-Lipschitz, applied to the reference), dz (train) within 8 u |gamma invstd| (|g| + |dbeta| / R + |xhat dgamma| / R),
    dz (eval) within 4 u |gamma invstd g|; a bf16 output b + 2^-8 (|ref| + b);
  * the masked gradient (dres, gout) bit for bit: dy where the mask is on, +0.0 where it is off.  The mask from y is y > 0;
    the mask from z is conv_refs.bn_mask.
"""
import re
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import conv16_refs as C16
import conv_refs as CR

U = 2.0 ** -24
U8 = 2.0 ** -8
RSQRT_ULP = 2               # error of the device rsqrtf in units of u; the one admissible widening is 4
EPS = 1e-5
MOM = 0.1
MAX_CHUNKS = 256            # bn_max_chunks()
BF = torch.bfloat16
F64 = torch.float64
INT_MAX = 2 ** 31 - 1
cdiv = CR.cdiv

K_SLOT = "=(n+8)*2^-24*sum|terms| of the slot's rows"
K_FIN = "=finalize tier: fp64 on the partials summed (bm1, bvar, RSQRT_ULP = %d)" % RSQRT_ULP
K_MAP = "=element tier: 4u / 8u of the term magnitudes on the stored statistics (bf16: + 2^-8)"
K_NOTE = "=measured, in units of 1e-6 relative; not a criterion"


# ==== the mirror of the host dispatch (csrc/batchnorm.hip) ===============================================================
def row_chunks(R, C, wg_aim, min_rows, max_chunks):
    """-> (chunks, rows per chunk): aim at wg_aim workgroups over cdiv(C, 64) column blocks, at least min_rows rows per
    chunk, at most max_chunks chunks, rows a multiple of 16"""
    n = min(wg_aim // cdiv(C, 64), cdiv(R, min_rows))
    n = min(max(n, 1), max_chunks)
    rpc = (cdiv(R, n) + 15) & ~15
    return cdiv(R, rpc), rpc


def pick_chunks(R, C):
    return row_chunks(R, C, 2048, 64, MAX_CHUNKS)


def ew_chunks(R, C):
    return row_chunks(R, C, 1024, 128, INT_MAX)


def ew_blocks(n4):
    return min(cdiv(n4, 256), 8192)


def workspace_floats(C):
    return MAX_CHUNKS * 2 * C


def chunk_facts(R, C, pick):
    """what a shape reaches: chunk count, rows per chunk, rows of the last chunk, column blocks, whether the cap bit"""
    n, rpc = pick(R, C)
    uncapped = max(min(2048 // cdiv(C, 64), cdiv(R, 64)), 1)
    return {"R": R, "C": C, "nchunk": n, "rpc": rpc, "last": R - (n - 1) * rpc, "colblocks": cdiv(C, 64),
            "cap": int(pick is pick_chunks and uncapped > MAX_CHUNKS), "laps": cdiv(min(rpc, R), 64),
            "dense": int(ew_blocks(R * C // 4) == 8192 and R * C // 4 > 8192 * 256)}


def tags_hold(tags, facts):
    """every tag `name<number>` of a row is what the mirror says: facts[name] == number (no number: truthy)"""
    for t in tags.split():
        m = re.fullmatch(r"([A-Za-z]+)(\d*)", t)
        v = facts[m.group(1)]
        if not (v == int(m.group(2)) if m.group(2) else bool(v)):
            return False
    return True


def T(bf16):
    return "bf16" if bf16 else "f32"


def bwd_variant(bf16, relu, y, dz, dres, train):
    """bn_bwd_t: maskz, gfirst, the reduce instance <T, RELU, MASKZ, GOUT> and the second pass <T, RELU, TRAIN, MASKZ>"""
    maskz = bool(relu and not y)
    gfirst = bool(relu and not maskz and dres and dz and not bf16)
    red = (1, int(maskz), int(gfirst)) if relu else (0, 0, 0)
    dx = None
    if dz or dres:
        dx = "bn_bwd_dx<%s,%d,%d,%d>" % (T(bf16), 1 if maskz else int(bool(relu) and not gfirst), int(bool(train)), int(maskz))
    return {"maskz": maskz, "gfirst": gfirst, "reduce": "bn_bwd_reduce<%s,%d,%d,%d>" % ((T(bf16),) + red), "dx": dx}


def reduce_variant(bf16, relu, gout):
    """bn_bwd_reduce_t (channel-major partials): <T, RELU, false, GOUT>; relu == 0 with gout is refused"""
    if not relu and gout:
        raise ValueError("bn_bwd_reduce_t: gout needs relu")
    return "bn_bwd_reduce_t<%s,%d,0,%d>" % (T(bf16), int(bool(relu)), int(bool(relu and gout)))


# ==== case tables ========================================================================================================
# (R, C, what the shape is there for -- tags_hold checks it against chunk_facts(pick_chunks))
REDUCE_SHAPES = [
    (1, 4, "R1 nchunk1 C4"), (3, 8, "R3 C8"), (17, 60, "R17 nchunk1 C60"), (65, 64, "nchunk2 last17 C64"),
    (193, 68, "last1 C68 colblocks2"), (207, 72, "last15 C72"), (208, 4, "last16"), (240, 8, "last48"), (241, 60, "last49"),
    (255, 64, "last63"), (961, 4, "nchunk16"), (1025, 8, "nchunk17"), (1100, 4, "nchunk18"), (4200, 8, "nchunk66"),
    (16400, 4, "cap rpc80"), (70, 2048, "colblocks32 nchunk2"), (300, 72, "nchunk5"),
]
# (R, C, tags against chunk_facts(ew_chunks)): a single chunk of fewer than 16 rows, 17 and 63 rows, a full chunk (two laps of
# r += 64), a ragged last chunk, C = 4 and C = 72 (the cq = min(c, C - 4) clamp)
EW_SHAPES = [
    (10, 4, "nchunk1 last10"), (17, 72, "nchunk1 last17"), (63, 8, "nchunk1 last63"), (128, 64, "nchunk1 laps2"),
    (129, 4, "nchunk2 last49"), (300, 72, "nchunk3 last76 laps2"), (700, 8, "nchunk6 last60"), (10, 72, "nchunk1 last10 colblocks2"),
]
PART_NCHUNK = [1, 3, 4, 5, 16, 17, 63, 64, 65, 130]        # chunks of an INPUT partial (second lap of i0 += 64 at 65 and 130)
DENSE = (2052, 4096, "dense")                             # R * C / 4 > 8192 * 256: the grid-stride loop's second lap

StatsCase = namedtuple("StatsCase", "R C bf16 fold rm rv outlier tags")
ApplyCase = namedtuple("ApplyCase", "R C bf16 relu res tags")
BwdCase = namedtuple("BwdCase", "R C bf16 relu y dz dres train tags")
FinCase = namedtuple("FinCase", "R C bf16 relu res nchunk ldp shift rm rv ss tags")
ReduceCase = namedtuple("ReduceCase", "R C bf16 relu gout alias cap tags")
DxFinCase = namedtuple("DxFinCase", "R C bf16 nchunk ldp alias tags")


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "-".join(
        "%s%s" % (k, v) for k, v in zip(c._fields, c) if k != "tags" and v not in (0, False, ""))


def ldp_of(nchunk):
    return (nchunk + 3) & ~3


def _stats_cases():
    opts = [(1, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1)]              # run_mean, run_var, ss_out: round-robin, no cross product
    rows = []
    for i, (R, C, tags) in enumerate(REDUCE_SHAPES):
        rm, rv, ss = opts[i % 4]
        bf16 = i % 2
        rows.append(StatsCase(R, C, bf16, int(ss and not bf16), rm, rv, 0, tags))
    rows += [StatsCase(1, 8, 1, 0, 1, 1, 0, "R1"), StatsCase(1100, 4, 1, 0, 1, 1, 0, "nchunk18"),
             StatsCase(300, 72, 0, 1, 1, 1, 1, "outlier"), StatsCase(300, 72, 1, 0, 1, 1, 1, "outlier")]
    return rows


def _apply_cases():
    shapes = [s for s in REDUCE_SHAPES if s[0] * s[1] <= 70 * 2048][:8]
    rows = [ApplyCase(R, C, i % 2, (i // 2) % 2, (i // 4) % 2, tags) for i, (R, C, tags) in enumerate(shapes)]
    return rows + [ApplyCase(DENSE[0], DENSE[1], 0, 1, 1, DENSE[2])]


def _bwd_cases():
    # relu, y given, dz, dres, train -- every combination bn_bwd_t can pick, each with both map types
    V = [(1, 0, 1, 1, 1), (1, 1, 1, 1, 1), (0, 0, 1, 1, 1), (1, 0, 1, 0, 0), (1, 1, 1, 0, 1), (1, 1, 0, 1, 1), (0, 0, 1, 0, 0),
         (1, 1, 1, 1, 0), (1, 0, 0, 1, 1), (0, 0, 0, 0, 1), (1, 1, 0, 0, 1), (1, 0, 1, 1, 0), (0, 0, 0, 1, 0), (1, 1, 0, 1, 0)]
    rows = []
    for i in range(2 * len(V)):
        R, C, tags = REDUCE_SHAPES[i % len(REDUCE_SHAPES)]
        rows.append(BwdCase(R, C, int(i >= len(V)), *V[i % len(V)], tags))
    return rows + [BwdCase(DENSE[0], DENSE[1], 0, 1, 0, 1, 1, 1, DENSE[2])]


def _fin_cases():
    opts = [(1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 1, 0)]       # shift, run_mean, run_var, ss_out
    rows = []
    for i in range(20):
        R, C, tags = EW_SHAPES[i % len(EW_SHAPES)]
        n = PART_NCHUNK[i % len(PART_NCHUNK)]
        ldp = n + 8 if i == 4 else ldp_of(n)
        rows.append(FinCase(R, C, i % 2, (i // 2) % 2, (i // 4) % 2, n, ldp, *opts[i % 5], tags))
    return rows


def _reduce_cases():
    V = [(1, 1, 0), (1, 0, 0), (0, 0, 0), (1, 1, 1)]                 # relu, gout, gout == dy
    rows = []
    for i, (R, C, tags) in enumerate(REDUCE_SHAPES + REDUCE_SHAPES[:7]):
        relu, gout, alias = V[i % 4]
        rows.append(ReduceCase(R, C, (i // 4) % 2, relu, gout, alias, 4 * (i % 3), tags))
    return rows


def _dxfin_cases():
    rows = []
    for i in range(12):
        R, C, tags = EW_SHAPES[i % len(EW_SHAPES)]
        n = PART_NCHUNK[(i + 3) % len(PART_NCHUNK)]
        rows.append(DxFinCase(R, C, i % 2, n, n + 8 if n == 64 else ldp_of(n), int(i in (2, 5)), tags))
    return rows


STATS_CASES, APPLY_CASES, BWD_CASES = _stats_cases(), _apply_cases(), _bwd_cases()
FIN_CASES, REDUCE_CASES, DXFIN_CASES = _fin_cases(), _reduce_cases(), _dxfin_cases()


def kernel_of(c):
    """the name of a case's row in the parity report: the entry point and the instance the mirror picks"""
    k = type(c).__name__
    if k == "StatsCase":
        return "bn_stats%s<%s>" % ("_fold" if c.fold else "", T(c.bf16))
    if k == "ApplyCase":
        return "bn_apply<%s,%d,%d>" % (T(c.bf16), c.relu, c.res)
    if k == "BwdCase":
        v = bwd_variant(c.bf16, c.relu, c.y, c.dz, c.dres, c.train)
        return v["reduce"] + (" + " + v["dx"] if v["dx"] else "")
    if k == "FinCase":
        return "bn_apply_fin<%s,%d,%d>" % (T(c.bf16), c.relu, c.res)
    if k == "ReduceCase":
        return reduce_variant(c.bf16, c.relu, c.gout)
    return "bn_bwd_dx_fin<%s>" % T(c.bf16)


# ==== inputs =============================================================================================================
def _gen(*key):
    return torch.Generator().manual_seed(50000 + zlib.crc32(repr(key).encode()) % 100000)


def _store(v, bf16):
    """the values a map of the case's type can hold"""
    return v.to(BF).float() if bf16 else v


def _vectors(g, C):
    return {"mean": 0.1 * torch.randn(C, generator=g), "invstd": 1 + 0.2 * torch.rand(C, generator=g),
            "gamma": (1 + 0.3 * torch.randn(C, generator=g)) * (1 - 2 * (torch.arange(C) % 3 == 1).float()),
            "beta": 0.2 * torch.randn(C, generator=g),
            "run_mean": 0.5 * torch.randn(C, generator=g), "run_var": 0.5 + torch.rand(C, generator=g)}


def _plant_y(y):
    """+0.0, -0.0, the smallest normal and a negative among the forward outputs (no subnormals: a mode setting)"""
    v = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, -1.5, 2.0 ** -126, 0.0, -0.0])
    flat = y.view(-1)
    n = min(flat.numel(), v.numel())
    flat[:n] = v[:n]
    if flat.numel() > 80:
        flat[-8:] = v


def _plant_z(I, bf16):
    """the mask edges of conv_refs._plant_mask_edges (on bf16 maps moved to representable neighbours, conv16_refs._plant_bf16)"""
    if bf16:
        I["mean"] = I["mean"].to(BF).float()          # z == mean, the zero of the expression, must be a bf16 value
        I["z"] = C16._plant_bf16(I["z"], I["mean"], I["invstd"], I["gamma"], I["beta"]).float()
    else:
        CR._plant_mask_edges(I["z"], I["gamma"], I["beta"],
                             lambda zz: CR.bn_mask(zz, I["mean"], I["invstd"], I["gamma"], I["beta"], False)[1], I["mean"].clone())


def split_partials(t1, t2, nchunk, ldp):
    """channel-major partials [2][C][ldp] of the fp64 terms t1, t2 [R][C]: the rows split into nchunk groups (tensor_split),
    each sum rounded to fp32, NaN in [nchunk, ldp)"""
    R, C = t1.shape
    part = torch.full((2, C, ldp), float("nan"))
    for w, t in enumerate((t1, t2)):
        for i, grp in enumerate(torch.tensor_split(t, nchunk)):
            part[w, :, i] = grp.sum(0).float()
    return part


@lru_cache(maxsize=16)
def inputs(c):
    """seeded fp32 operands of a case (CPU); a map of a bf16 case holds bf16 values.  Shared: never written to.  (A short
    cache: a case's tests follow each other, and the dense rows are ~100 MB each.)"""
    g = _gen(tuple(c))
    k, R, C = type(c).__name__, c.R, c.C
    I = _vectors(g, C)
    m = lambda scale=1.0: _store(scale * torch.randn(R, C, generator=g), c.bf16)
    if k == "StatsCase":
        x = torch.randn(R, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 2 * torch.randn(C, generator=g)
        if c.outlier and R > 1:      # row 0 -- the conditioning shift s = x[0][c] -- 64 standard deviations off the mean
            x[0] = x[1:].mean(0) + 64 * x[1:].std(0)
        I["x"] = _store(x, c.bf16)
    elif k == "ApplyCase":
        I["z"], I["res"] = m(), m()
    elif k == "BwdCase":
        I["dy"], I["z"], I["y"] = m(), m(), m()
        _plant_y(I["y"])
        if c.relu and not c.y:
            _plant_z(I, c.bf16)
    elif k == "FinCase":
        z = torch.randn(R, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        I["z"], I["res"] = _store(z, c.bf16), m()
        I["shift"] = I["z"].mean(0) + 0.05 * torch.randn(C, generator=g)
        d = I["z"].double() - (I["shift"].double() if c.shift else 0.0)
        I["partial"] = split_partials(d, d * d, c.nchunk, c.ldp)
    elif k == "ReduceCase":
        I["dy"], I["z"], I["y"] = m(), m(), m()
        _plant_y(I["y"])
    else:
        I["g"], I["z"] = m() * (torch.rand(R, C, generator=g) > 0.4), m()
        gg, xh = I["g"].double(), xhat64(I["z"], I)
        I["partial"] = split_partials(gg, gg * xh, c.nchunk, c.ldp)
    return I


# ==== the formulas, in fp64 from fp32 inputs =============================================================================
def xhat64(z, st):
    return (z.double() - st["mean"].double()) * st["invstd"].double()


def mom_pair(momentum=MOM):
    """(1 - momentum, momentum) as the kernel forms them: fl32(1 - fl32(momentum)) is not 0.9"""
    m = np.float32(momentum)
    return float(np.float32(np.float32(1.0) - m)), float(m)


def y_ref(z, res, st, relu):
    """-> (y, magnitude of the terms)"""
    t = xhat64(z, st) * st["gamma"].double()
    y, mag = t + st["beta"].double(), t.abs() + st["beta"].double().abs()
    if res is not None:
        y, mag = y + res.double(), mag + res.double().abs()
    return (torch.relu(y) if relu else y), mag


def dz_ref(g, xh, st, dbeta, dgamma, R, train):
    """-> (dz, bound)"""
    gi = st["gamma"].double() * st["invstd"].double()
    if not train:
        return gi * g, 4 * U * (gi * g).abs()
    db, dg = dbeta.double() / R, dgamma.double() / R
    return gi * (g - db - xh * dg), 8 * U * gi.abs() * (g.abs() + db.abs() + (xh * dg).abs())


def stats_of_partials(s1, s2, shift, R):
    """s1, s2 [C][n] -> dict(mean, var (clamped at 0 as the kernel does), m1, bm1, bvar) in fp64"""
    n = s1.shape[1]
    s1, s2 = s1.double(), s2.double()
    m1 = s1.sum(1) / R
    bm1 = (n + 8) * U * s1.abs().sum(1) / R
    var = s2.sum(1) / R - m1 * m1
    bvar = (n + 8) * U * s2.abs().sum(1) / R + 2 * m1.abs() * bm1 + bm1 * bm1 + 4 * U * m1 * m1
    return {"mean": (0.0 if shift is None else shift.double()) + m1, "var": var.clamp_min(0.0), "var_raw": var, "m1": m1,
            "bm1": bm1, "bvar": bvar}


def _bf(bound, want, bf16):
    return bound + U8 * (want.abs() + bound) if bf16 else bound


def _bits(t):
    return t.float().contiguous().view(torch.int32)


# ==== judges =============================================================================================================
def judge_slots(kernel, ok, got, t1, t2, slot, nslot):
    """got [2][nslot][C] against the fp64 sums of the terms t1, t2 [rows][C] over the rows with slot[row] == that slot"""
    def sums(t):
        return torch.zeros(nslot, t.shape[1], dtype=F64).index_add_(0, slot, t)
    cnt = torch.bincount(slot, minlength=nslot).double().view(1, nslot, 1)
    want = torch.stack([sums(t1), sums(t2)])
    ok(kernel, "slots", got, want, (cnt + 8) * U * torch.stack([sums(t1.abs()), sums(t2.abs())]), K_SLOT)


def judge_finalize(kernel, ok, s1, s2, shift, R, out, I, eps=EPS, k=None, momentum=MOM, s=None):
    """mean / invstd / run_mean / run_var / ss of `out` (None: not written) from the partials s1, s2 [C][n] that were summed.
    s: the dict of stats_of_partials from a caller whose partials are not stored (tests/block16_refs.py derives mean, var,
    m1, bm1, bvar from the exact product and the slot bounds); s1, s2 are not read then."""
    k = RSQRT_ULP if k is None else k
    s = stats_of_partials(s1, s2, shift, R) if s is None else s
    ok(kernel, "mean", out["mean"], s["mean"], s["bm1"] + 2 * U * s["mean"].abs(), K_FIN)
    e = float(np.float32(eps))
    lo = torch.rsqrt(s["var_raw"] + s["bvar"] + e) * (1 - k * U)
    hi = torch.rsqrt((s["var_raw"] - s["bvar"]).clamp_min(0.0) + e) * (1 + k * U)
    ok(kernel, "invstd", out["invstd"], (lo + hi) / 2, (hi - lo) / 2, K_FIN)
    om, m = mom_pair(momentum)
    mean, invstd = out["mean"].double(), out["invstd"].double()
    if out.get("run_mean") is not None:
        old = I["run_mean"].double()
        ok(kernel, "run_mean", out["run_mean"], om * old + m * mean, 4 * U * (old.abs() + mean.abs()), K_FIN)
    if out.get("run_var") is not None:
        old, f = I["run_var"].double(), (R / (R - 1.0) if R > 1 else 1.0)
        a, b = om * old, m * s["var"] * f
        ok(kernel, "run_var", out["run_var"], a + b, m * f * s["bvar"] + 4 * U * (a.abs() + b.abs()), K_FIN)
    if out.get("ss") is not None:
        scale = I["gamma"].double() * invstd
        ok(kernel, "scale", out["ss"][:, 0], scale, U * scale.abs(), K_FIN)
        ok(kernel, "shift", out["ss"][:, 1], I["beta"].double() - mean * scale,
           2 * U * ((mean * scale).abs() + I["beta"].double().abs()), K_FIN)


def judge_param_grads(kernel, ok, s1, s2, out):
    """dbeta / dgamma are the slot sums: s1, s2 [C][n]"""
    n = s1.shape[1]
    for name, s in (("dbeta", s1), ("dgamma", s2)):
        ok(kernel, name, out[name], s.double().sum(1), (n + 8) * U * s.double().abs().sum(1), K_FIN)


def judge_masked(kernel, name, got, dy, on):
    want = torch.where(on, dy, torch.zeros(()))
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, "%s %s: %d elements are not dy / +0.0 bit for bit (first at %s)" % (
        kernel, name, bad.shape[0], bad[0].tolist())


def judge_stats(c, I, out, kernel, ok, note=None):
    """out: partial [nchunk][2][C], mean, invstd, run_mean, run_var, ss [C][2] (None where the case passes NULL)"""
    x = I["x"].double()
    d = x - x[0]
    nchunk, rpc = pick_chunks(c.R, c.C)
    p = out["partial"]
    judge_slots(kernel, ok, p.permute(1, 0, 2), d, d * d, torch.arange(c.R) // rpc, nchunk)
    judge_finalize(kernel, ok, p[:, 0].t(), p[:, 1].t(), I["x"][0], c.R, out, I)
    if note is not None:
        var = x.var(0, unbiased=False)
        got = out["invstd"].double() ** -2 - float(np.float32(EPS))
        rel = float(((got - var).abs() / (var + 1e-30)).max()) if c.R > 1 else 0.0
        note("%s%s" % (kernel, " outlier shift" if c.outlier else ""), "var/data", rel * 1e6, K_NOTE)


def judge_y(kernel, ok, z, res, st, relu, y, bf16):
    want, mag = y_ref(z, res, st, relu)
    ok(kernel, "y", y, want, _bf(4 * U * mag, want, bf16), K_MAP)


def judge_apply(c, I, out, kernel, ok):
    judge_y(kernel, ok, I["z"], I["res"] if c.res else None, I, c.relu, out["y"], c.bf16)


def mask_of(I, relu, from_y):
    if not relu:
        return torch.ones_like(I["dy"], dtype=torch.bool)
    if from_y:
        return I["y"] > 0
    return CR.bn_mask(I["z"], I["mean"], I["invstd"], I["gamma"], I["beta"], False)[0]


def judge_bwd(c, I, out, kernel, ok):
    """out: partial [nchunk][2][C], dbeta, dgamma, dz, dres (None: NULL)"""
    on = mask_of(I, c.relu, c.y)
    g = torch.where(on, I["dy"], torch.zeros(())).double()
    xh = xhat64(I["z"], I)
    nchunk, rpc = pick_chunks(c.R, c.C)
    p = out["partial"]
    judge_slots(kernel, ok, p.permute(1, 0, 2), g, g * xh, torch.arange(c.R) // rpc, nchunk)
    judge_param_grads(kernel, ok, p[:, 0].t(), p[:, 1].t(), out)
    if out.get("dres") is not None:
        judge_masked(kernel, "dres", out["dres"], I["dy"], on)
    if out.get("dz") is not None:
        want, b = dz_ref(g, xh, I, out["dbeta"], out["dgamma"], c.R, c.train)
        ok(kernel, "dz", out["dz"], want, _bf(b, want, c.bf16), K_MAP)


def judge_fin(c, I, out, kernel, ok):
    """out: y, mean, invstd, run_mean, run_var, ss"""
    p = I["partial"]
    judge_finalize(kernel, ok, p[0, :, :c.nchunk], p[1, :, :c.nchunk], I["shift"] if c.shift else None, c.R, out, I)
    if out.get("y") is not None:
        judge_y(kernel, ok, I["z"], I["res"] if c.res else None, dict(I, mean=out["mean"], invstd=out["invstd"]), c.relu,
                out["y"], c.bf16)


def judge_reduce(c, I, out, kernel, ok):
    """out: partial [2][C][nchunk], gout, nchunk"""
    nchunk, rpc = pick_chunks(c.R, c.C)
    assert out["nchunk"] == nchunk, "%s: *nchunk_out %d, the mirror says %d" % (kernel, out["nchunk"], nchunk)
    on = mask_of(I, c.relu, True)
    g = torch.where(on, I["dy"], torch.zeros(())).double()
    judge_slots(kernel, ok, out["partial"].permute(0, 2, 1), g, g * xhat64(I["z"], I), torch.arange(c.R) // rpc, nchunk)
    if out.get("gout") is not None:
        judge_masked(kernel, "gout", out["gout"], I["dy"], on)


def judge_dxfin(c, I, out, kernel, ok):
    """out: dbeta, dgamma, dz"""
    p = I["partial"]
    judge_param_grads(kernel, ok, p[0, :, :c.nchunk], p[1, :, :c.nchunk], out)
    want, b = dz_ref(I["g"].double(), xhat64(I["z"], I), I, out["dbeta"], out["dgamma"], c.R, 1)
    ok(kernel, "dz", out["dz"], want, _bf(b, want, c.bf16), K_MAP)


# ==== what the tables must reach (tests/test_bn_stem_refs.py asserts it) =================================================
REQUIRED = sorted(
    ["bn_stats<f32>", "bn_stats<bf16>", "bn_stats_fold<f32>", "bn_bwd_dx_fin<f32>", "bn_bwd_dx_fin<bf16>"] +
    ["bn_apply<%s,%d,%d>" % (t, r, s) for t in ("f32", "bf16") for r in (0, 1) for s in (0, 1)] +
    ["bn_apply_fin<%s,%d,%d>" % (t, r, s) for t in ("f32", "bf16") for r in (0, 1) for s in (0, 1)] +
    ["bn_bwd_dx<%s,%d,%d,%d>" % (t, r, tr, mz) for t in ("f32", "bf16") for (r, mz) in ((1, 1), (1, 0), (0, 0)) for tr in (0, 1)] +
    ["bn_bwd_reduce<%s,%s>" % (t, v) for t in ("f32", "bf16") for v in ("1,1,0", "1,0,0", "0,0,0")] + ["bn_bwd_reduce<f32,1,0,1>"] +
    ["bn_bwd_reduce_t<%s,%s>" % (t, v) for t in ("f32", "bf16") for v in ("1,0,1", "1,0,0", "0,0,0")])


def reached():
    out = set()
    for c in STATS_CASES + APPLY_CASES + FIN_CASES + REDUCE_CASES + DXFIN_CASES:
        out.add(kernel_of(c))
    for c in BWD_CASES:
        v = bwd_variant(c.bf16, c.relu, c.y, c.dz, c.dres, c.train)
        out.update(x for x in (v["reduce"], v["dx"]) if x)
    return out
