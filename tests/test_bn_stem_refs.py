"""The fp64 references of the BatchNorm and stem kernels (tests/bn_refs.py, tests/stem_refs.py), their judges and the case
tables of tests/test_gpu_bn_kernels.py / tests/test_gpu_stem_kernels.py, without a GPU:
  * the references equal torch's fp64 batch_norm + autograd, conv2d(stride 2, padding 3) and max_pool2d(3, 2, 1) to 1e-12;
  * every row of the tables names the instance or edge it is there for and the mirror of the host dispatch confirms the
    name; every instance of bn_refs.REQUIRED and every edge the tables must hold is reached;
  * the bounds are attainable: torch's CPU fp32 evaluation of the same formulas passes every judge at every row (the worst
    err / bound per result is printed);
  * the judges are sensitive: the fp32 evaluation with one planted defect fails at least one row, for each defect of DEFECTS.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
import stem_refs as S
import test_gpu_bn_kernels as TB  # noqa: F401 (the GPU modules must import -- and collect -- without a GPU)
import test_gpu_stem_kernels as TS  # noqa: F401
from test_conv_refs import Worst

F32, F64 = torch.float32, torch.float64
t32 = lambda v: torch.tensor(float(v), dtype=F32)


# ==== torch's CPU fp32 evaluation of the kernels' formulas, with an optional planted defect ==============================
def store(v, bf16, defect=None):
    if not bf16:
        return v.float()
    if defect == "a bf16 store that truncates":
        return (v.float().contiguous().view(torch.int32) & -65536).view(F32)
    return v.to(B.BF).float()


def emu_finalize(s1, s2, shift, R, want, I, defect=None):
    """s1, s2 [C][n] fp32; want = (run_mean, run_var, ss) flags"""
    inv_n = t32(1) / t32(R)
    m1 = s1.sum(1) * inv_n
    mu = m1 if shift is None else shift + m1
    var = (s2.sum(1) * inv_n - m1 * m1).clamp_min(0)
    inv = torch.rsqrt(var + t32(B.EPS))
    m = t32(B.MOM)
    om = t32(1) - m
    out = {"mean": mu, "invstd": inv, "run_mean": None, "run_var": None, "ss": None}
    if want[0]:
        out["run_mean"] = om * I["run_mean"] + m * mu
    if want[1]:
        f = t32(1)
        if R > 1 or defect == "R/(R-1) applied at R = 1":
            f = t32(R) / t32(R - 1)
        if defect == "R for R - 1 in the running variance":
            f = t32(1)
        out["run_var"] = om * I["run_var"] + m * (var * f)
    if want[2]:
        sc = I["gamma"] * inv
        out["ss"] = torch.stack([sc, I["beta"] - mu * sc], 1)
    return out


def chunk_sums(t1, t2, R, C, defect=None):
    """chunk-major partials [nchunk][2][C] of fp32 terms over the chunks of pick_chunks"""
    nchunk, rpc = B.pick_chunks(R, C)
    part = torch.zeros(nchunk, 2, C)
    for i in range(nchunk):
        r0, r1 = i * rpc, min(R, (i + 1) * rpc)
        if defect == "the last row of a ragged chunk dropped" and r1 - r0 < rpc and r1 - r0 > 1:
            r1 -= 1
        part[i, 0], part[i, 1] = t1[r0:r1].sum(0), t2[r0:r1].sum(0)
    if defect == "a partial one slot off" and nchunk > 1:
        moved = part.roll(1, dims=0)
        assert torch.allclose(moved.sum(0), part.sum(0), rtol=1e-4, atol=1e-4)          # the channel sums cannot tell
        part = moved
    return part


def emu_stats(c, I, defect=None):
    x = I["x"]
    d = x - x[0]
    part = chunk_sums(d, d * d, c.R, c.C, defect)
    out = emu_finalize(part[:, 0].t(), part[:, 1].t(), x[0], c.R, (c.rm, c.rv, c.fold), I, defect)
    return dict(out, partial=part)


def emu_y(z, res, st, relu, bf16, defect=None):
    t = (z - st["mean"]) * st["invstd"] * st["gamma"] + st["beta"]
    if res is not None:
        t = t + res
    return store(torch.relu(t) if relu else t, bf16, defect)


def emu_apply(c, I, defect=None):
    return {"y": emu_y(I["z"], I["res"] if c.res else None, I, c.relu, c.bf16, defect)}


def emu_mask(I, relu, from_y, defect):
    if not relu:
        return torch.ones_like(I["dy"], dtype=torch.bool)
    if from_y:
        return I["y"] >= 0 if defect == "mask from >=" else I["y"] > 0
    if defect in ("mask from >=", "mask without the fused rounding"):
        f32, f64 = np.float32, np.float64
        xhat = B.CR.bn_mask(I["z"], I["mean"], I["invstd"], I["gamma"], I["beta"], False)[1].numpy()
        a, b = I["gamma"].numpy(), I["beta"].numpy()
        if defect == "mask from >=":
            return torch.from_numpy(xhat.astype(f64) * a.astype(f64) + b.astype(f64) >= 0)
        return torch.from_numpy(((xhat * a).astype(f32) + b) > 0)
    return B.mask_of(I, relu, from_y)


def emu_g(I, on, defect):
    if defect == "a masked g left as -0.0":
        return I["dy"] * on.float()
    return torch.where(on, I["dy"], torch.zeros(()))


def emu_dz(g, xh, st, dbeta, dgamma, R, train, bf16, defect=None):
    gi = st["gamma"] * st["invstd"]
    if not train:
        return store(gi * g, bf16, defect)
    inv_n = t32(1) / t32(R)
    dg = dgamma if defect == "dz with dgamma not divided by R" else dgamma * inv_n
    return store(gi * (g - dbeta * inv_n - xh * dg), bf16, defect)


def emu_bwd(c, I, defect=None):
    on = emu_mask(I, c.relu, c.y, defect)
    g = emu_g(I, on, defect)
    xh = (I["z"] - I["mean"]) * I["invstd"]
    part = chunk_sums(g, g * xh, c.R, c.C, defect)
    out = {"partial": part, "dbeta": part[:, 0].sum(0), "dgamma": part[:, 1].sum(0), "dz": None, "dres": None}
    if c.dz:
        out["dz"] = emu_dz(g, xh, I, out["dbeta"], out["dgamma"], c.R, c.train, c.bf16, defect)
    if c.dres:
        out["dres"] = g
    return out


def emu_fin(c, I, defect=None):
    p = I["partial"]
    n = c.nchunk
    if defect == "the padding slot of a partial summed" and c.ldp > n:
        p = p.clone()
        p[:, :, n] = 0.25 * c.R          # a finite value where the test keeps NaN
        n += 1
    out = emu_finalize(p[0, :, :n], p[1, :, :n], I["shift"] if c.shift else None, c.R, (c.rm, c.rv, c.ss), I, defect)
    out["y"] = emu_y(I["z"], I["res"] if c.res else None, dict(I, mean=out["mean"], invstd=out["invstd"]), c.relu, c.bf16, defect)
    return out


def emu_reduce(c, I, defect=None):
    on = emu_mask(I, c.relu, True, defect)
    g = emu_g(I, on, defect)
    part = chunk_sums(g, g * ((I["z"] - I["mean"]) * I["invstd"]), c.R, c.C, defect)
    return {"partial": part.permute(1, 2, 0).contiguous(), "gout": g if c.gout else None, "nchunk": B.pick_chunks(c.R, c.C)[0]}


def emu_dxfin(c, I, defect=None):
    p = I["partial"]
    n = c.nchunk
    if defect == "the padding slot of a partial summed" and c.ldp > n:
        p = p.clone()
        p[:, :, n] = 0.25 * c.R
        n += 1
    db, dg = p[0, :, :n].sum(1), p[1, :, :n].sum(1)
    xh = (I["z"] - I["mean"]) * I["invstd"]
    return {"dbeta": db, "dgamma": dg, "dz": emu_dz(I["g"], xh, I, db, dg, c.R, 1, c.bf16, defect)}


def emu_conv(c, I, defect=None):
    x, w = I["x"], I["w"]
    if defect == "a stem tap read across the right edge into the next row":
        xp = F.pad(x, (3, 3, 3, 3))
        flat = xp.reshape(c.N, 3, -1)
        Wp = c.W + 6
        for r in range(3, c.H + 3 - 1):          # the three columns right of row r hold the start of the next row
            flat[:, :, r * Wp + 3 + c.W:r * Wp + 6 + c.W] = flat[:, :, (r + 1) * Wp + 3:(r + 1) * Wp + 6]
        z = S._rows(F.conv2d(xp, w, stride=2))
    else:
        z = S._rows(F.conv2d(x, w, stride=2, padding=3))
    out = {"z": z, "partial": None}
    if c.stat:
        sh = I["shift"] if c.stat == 2 else torch.zeros(64)
        d = z - sh
        nslot = S.stem_tiles(c.N, c.H, c.W)
        slot = S.pixel_slots(c.N, c.H, c.W)
        part = torch.stack([torch.zeros(nslot, 64).index_add_(0, slot, t) for t in (d, d * d)])      # [2][slot][64]
        if defect == "a ragged tile's invalid pixels counted":
            for b, tiles in enumerate(S.tile_walk(c.N, c.H, c.W)):
                inv = sum(S.TH * S.TW - t[3] * t[4] for t in tiles)
                part[0, b] += inv * (0 - sh)
                part[1, b] += inv * sh * sh
        out["partial"] = part.permute(0, 2, 1).contiguous()
    return out


def emu_pool(c, I, defect=None):
    start = 0 if defect == "a pooling window starting at 2*oh" else -1
    out = S.pool_ref(c, I, F64, start, clamp=defect != "an all-negative window returning its max")[0].float()   # one fma each
    return store(out, c.obf, defect)


FAMILIES = [
    ("stats", B.STATS_CASES, B.inputs, emu_stats, B.judge_stats),
    ("apply", B.APPLY_CASES, B.inputs, emu_apply, B.judge_apply),
    ("bwd", B.BWD_CASES, B.inputs, emu_bwd, B.judge_bwd),
    ("fin", B.FIN_CASES, B.inputs, emu_fin, B.judge_fin),
    ("reduce", B.REDUCE_CASES, B.inputs, emu_reduce, B.judge_reduce),
    ("dxfin", B.DXFIN_CASES, B.inputs, emu_dxfin, B.judge_dxfin),
    ("conv7", S.CONV_CASES, lambda c: S.conv_inputs(c.N, c.H, c.W), emu_conv, S.judge_conv),
    ("pool", S.POOL_CASES, S.pool_inputs, emu_pool, S.judge_pool),
]


def _kernel(c):
    return B.kernel_of(c) if type(c).__module__ == "bn_refs" else type(c).__name__


class PerResult:
    """the worst err / bound per result name over every row"""

    def __init__(self):
        self.worst = {}

    def ok(self, kernel, name, got, want, bound, kind="sum"):
        w = Worst()
        try:
            w.ok(kernel, name, got, want, bound, kind)
        finally:
            key = (kernel.split("<")[0].split(" ")[0], name)
            self.worst[key] = max(self.worst.get(key, 0.0), w.ratio)


def test_cpu_fp32_passes_every_judge():
    per, failed, rows = PerResult(), [], 0
    for fam, cases, inputs, emu, judge in FAMILIES:
        for c in cases:
            I = inputs(c)
            rows += 1
            try:
                judge(c, I, emu(c, I), _kernel(c), per.ok)
            except AssertionError as e:
                failed.append("%s: %s" % (c, e))
    for (k, name), r in sorted(per.worst.items()):
        print("%-22s %-9s worst err/bound %.3f" % (k, name, r))
    print("CPU fp32 evaluation of %d rows" % rows)
    assert not failed and max(per.worst.values()) < 1.0, failed[:5]


# ==== planted defects ====================================================================================================
DEFECTS = [
    "the last row of a ragged chunk dropped", "a partial one slot off", "the padding slot of a partial summed",
    "R for R - 1 in the running variance", "R/(R-1) applied at R = 1", "mask from >=", "mask without the fused rounding",
    "a masked g left as -0.0", "dz with dgamma not divided by R", "a bf16 store that truncates",
    "a stem tap read across the right edge into the next row", "a ragged tile's invalid pixels counted",
    "a pooling window starting at 2*oh", "an all-negative window returning its max",
]
_DENSE = B.DENSE[:2]
# the families a defect can change anything in (the others are not evaluated)
_WHERE = {"the last row": "stats bwd reduce", "a partial one": "stats bwd reduce", "the padding": "fin dxfin", "R for": "stats fin",
          "R/(R-1)": "stats fin", "mask": "bwd reduce", "a masked": "bwd reduce", "dz with": "bwd dxfin",
          "a bf16": "apply bwd fin dxfin pool", "a stem": "conv7", "a ragged": "conv7", "a pooling": "pool", "an all-negative": "pool"}


def _passes(judge, c, I, out):
    try:
        judge(c, I, out, _kernel(c), Worst().ok)
        return True
    except AssertionError:
        return False


def _same(a, b):
    if a is None or b is None or not torch.is_tensor(a):
        return a is b or a == b
    return torch.equal(a.float().contiguous().view(torch.int32), b.float().contiguous().view(torch.int32))


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.replace(" ", "_") for d in DEFECTS])
def test_planted_defect_fails(defect):
    """rows the defect changes nothing at do not count; the defect-free evaluation of a counted row passes"""
    applied = caught = 0
    where = next(v for k, v in _WHERE.items() if defect.startswith(k)).split()
    for fam, cases, inputs, emu, judge in FAMILIES:
        for c in cases if fam in where else []:
            if getattr(c, "R", 0) == _DENSE[0]:
                continue
            I = inputs(c)
            good, bad = emu(c, I), emu(c, I, defect)
            if not torch.is_tensor(good) and all(_same(good[k], bad[k]) for k in good) or torch.is_tensor(good) and _same(good, bad):
                continue
            assert _passes(judge, c, I, good), "the defect-free evaluation of %s fails" % (c,)
            applied += 1
            caught += not _passes(judge, c, I, bad)
    print("%s: caught at %d of %d rows it changes" % (defect, caught, applied))
    assert applied and caught >= 1


# ==== the references against torch =======================================================================================
@pytest.mark.parametrize("R,C", [(300, 72), (4200, 8), (70, 2048), (16400, 4), (3, 8), (1, 4)])
def test_bn_reference_equals_torch_fp64(R, C):
    g = torch.Generator().manual_seed(R + C)
    z = (torch.randn(R, C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    res, dy = torch.randn(R, C, generator=g, dtype=F64), torch.randn(R, C, generator=g, dtype=F64)
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g, dtype=F64), 0.5 + torch.rand(C, generator=g, dtype=F64)
    zd = z.detach()
    d = zd - zd[0]                                               # the shifted sums of bn_stats, in exact chunks
    nchunk, rpc = B.pick_chunks(R, C)
    s1 = torch.stack([t.sum(0) for t in torch.split(d, rpc)], 1)
    s2 = torch.stack([t.sum(0) for t in torch.split(d * d, rpc)], 1)
    assert s1.shape[1] == nchunk
    s = B.stats_of_partials(s1, s2, zd[0], R)
    st = {"mean": s["mean"], "invstd": torch.rsqrt(s["var"] + B.EPS), "gamma": gamma.detach(), "beta": beta.detach()}
    y, _ = B.y_ref(zd, res, st, True)
    if R == 1:              # torch refuses one value per channel in training mode: the definition by hand
        assert float(s["var"].abs().max()) == 0 and float((s["mean"] - zd[0]).abs().max()) == 0
        assert float((y - torch.relu(beta.detach() + res[0])).abs().max()) <= 1e-12
        return
    rm, rv = rm0.clone(), rv0.clone()
    m = B.mom_pair()[1]
    yt = torch.relu(F.batch_norm(z.t().reshape(1, C, R), rm, rv, gamma, beta, True, m, B.EPS).reshape(C, R).t() + res)
    assert float((s["mean"] - zd.mean(0)).abs().max()) <= 1e-12 and float((s["var"] - zd.var(0, unbiased=False)).abs().max()) <= 1e-12
    assert float((y - yt.detach()).abs().max()) <= 1e-12
    yt.backward(dy)
    gm = torch.where(y > 0, dy, torch.zeros((), dtype=F64))
    xh = B.xhat64(zd, st)
    dbeta, dgamma = gm.sum(0), (gm * xh).sum(0)
    dz, _ = B.dz_ref(gm, xh, st, dbeta, dgamma, R, 1)
    for a, b in ((dz, z.grad), (dbeta, beta.grad), (dgamma, gamma.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # the running statistics as judge_finalize forms them: torch's (1 - m) is exact, the kernel's is fl32(1 - fl32(m))
    got = {}
    B.judge_finalize("ref", lambda k, name, g_, want, bound, kind: got.__setitem__(name, want), s1, s2, zd[0], R,
                     {"mean": s["mean"], "invstd": st["invstd"], "run_mean": rm0, "run_var": rv0}, {"run_mean": rm0, "run_var": rv0})
    om = B.mom_pair()[0]
    assert abs(om - (1 - m)) < 2.0 ** -24 and om != 1 - m
    assert float((got["run_mean"] - (rm + (om - (1 - m)) * rm0)).abs().max()) <= 1e-12
    assert float((got["run_var"] - (rv + (om - (1 - m)) * rv0)).abs().max()) <= 1e-12


@pytest.mark.parametrize("c", S.CONV_CASES[:6], ids=S.case_id)
def test_stem_conv_reference_equals_unfold(c):
    """conv2d is the definition; its row order and the |x|, |w| sum against an im2col product written with unfold"""
    I = S.conv_inputs(c.N, c.H, c.W)
    z, Sabs = S.conv_ref(c.N, c.H, c.W)
    Ho, Wo = S.out_hw(c.H, c.W)
    for want, (x, w) in ((z, (I["x"].double(), I["w"].double())), (Sabs, (I["x"].double().abs(), I["w"].double().abs()))):
        cols = F.unfold(x, 7, padding=3, stride=2)                      # [N, 147, Ho * Wo]
        got = torch.einsum("nkp,ok->npo", cols, w.reshape(64, 147)).reshape(c.N * Ho * Wo, 64)
        assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("c", S.POOL_CASES, ids=S.case_id)
def test_pool_reference_equals_max_pool2d(c):
    I = S.pool_inputs(c)
    z, ss = I["z"].double().reshape(c.N, c.Hz, c.Wz, c.C), I["ss"].double()
    want = F.max_pool2d(torch.relu(z * ss[:, 0] + ss[:, 1]).permute(0, 3, 1, 2), 3, 2, 1)
    assert float((S.pool_ref(c, I)[0] - S._rows(want)).abs().max()) <= 1e-12


# ==== the tables =========================================================================================================
def test_every_row_names_what_it_is_there_for():
    for c in B.STATS_CASES + B.APPLY_CASES + B.BWD_CASES + B.REDUCE_CASES:
        facts = dict(B.chunk_facts(c.R, c.C, B.pick_chunks), outlier=getattr(c, "outlier", 0))
        assert c.tags and B.tags_hold(c.tags, facts), (c, facts)
    for c in B.FIN_CASES + B.DXFIN_CASES:
        assert c.tags and B.tags_hold(c.tags, B.chunk_facts(c.R, c.C, B.ew_chunks)), c
        assert c.ldp % 4 == 0 and c.ldp >= c.nchunk
    for c in S.CONV_CASES:
        assert c.tags and B.tags_hold(c.tags, S.walk_facts(c.N, c.H, c.W)), (c, S.walk_facts(c.N, c.H, c.W))


def test_tables_reach_every_instance_and_edge():
    assert not set(B.REQUIRED) - B.reached(), sorted(set(B.REQUIRED) - B.reached())
    red = [B.chunk_facts(c.R, c.C, B.pick_chunks) for c in B.STATS_CASES]
    for fam in (B.STATS_CASES, B.BWD_CASES, B.REDUCE_CASES):
        f = [B.chunk_facts(c.R, c.C, B.pick_chunks) for c in fam]
        assert {x["R"] for x in f} >= {1, 3, 17} and {x["last"] for x in f if x["nchunk"] > 1} >= {1, 15, 16, 17, 48, 49, 63}
        assert {x["nchunk"] for x in f} >= {1, 2, 16, 17, 18, 66} and any(x["cap"] and x["rpc"] == 80 for x in f)
        assert any(x["colblocks"] == 32 and x["nchunk"] == 2 for x in f) and {x["C"] for x in f} >= {4, 8, 60, 64, 68, 72}
    assert red and {c.bf16 for c in B.STATS_CASES if c.outlier} == {0, 1}
    assert any(c.R == 1 and c.rv for c in B.STATS_CASES) and any(c.R == 1 and c.rv for c in B.FIN_CASES + B.STATS_CASES)
    for opt in ("rm", "rv", "fold"):
        assert {getattr(c, opt) for c in B.STATS_CASES} == {0, 1}
    # the second pass: dz NULL, dres NULL, train 0, the g-first form, both masks; the dense rows
    assert {(c.dz, c.dres) for c in B.BWD_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c.train for c in B.BWD_CASES} == {0, 1}
    assert any(B.bwd_variant(c.bf16, c.relu, c.y, c.dz, c.dres, c.train)["gfirst"] for c in B.BWD_CASES)
    for fam in (B.APPLY_CASES, B.BWD_CASES):
        assert any(B.chunk_facts(c.R, c.C, B.pick_chunks)["dense"] and not c.bf16 for c in fam)
    # finalize on load: the row shapes, the input partials, every optional pointer both ways
    for fam in (B.FIN_CASES, B.DXFIN_CASES):
        f = [B.chunk_facts(c.R, c.C, B.ew_chunks) for c in fam]
        assert any(x["nchunk"] == 1 and x["last"] < 16 for x in f) and {17, 63} <= {x["last"] for x in f if x["nchunk"] == 1}
        assert any(x["nchunk"] > 1 and x["last"] < x["rpc"] for x in f) and any(x["laps"] >= 2 for x in f)
        assert {c.C for c in fam} >= {4, 72} and {c.nchunk for c in fam} == set(B.PART_NCHUNK)
        assert any(c.ldp == c.nchunk + 8 for c in fam) and {c.bf16 for c in fam} == {0, 1}
    for opt in ("shift", "rm", "rv", "ss"):
        assert {getattr(c, opt) for c in B.FIN_CASES} == {0, 1}
    assert {(c.relu, c.gout) for c in B.REDUCE_CASES} == {(0, 0), (1, 0), (1, 1)} and any(c.alias for c in B.REDUCE_CASES)
    assert {c.bf16 for c in B.DXFIN_CASES if c.alias} == {0, 1}
    # the stem
    f = {S.case_id(c): S.walk_facts(c.N, c.H, c.W) for c in S.CONV_CASES}
    assert any(x["tiles"] == 1 and x["Ho"] == 1 for x in f.values()) and any(x["onerow"] and x["onecol"] for x in f.values())
    assert any(x["tiles"] == 770 and x["two"] == 2 for x in f.values()) and any(x["three"] == 64 for x in f.values())
    assert {(c.N, c.H, c.W) for c in S.CONV_CASES} >= {(1, 1, 1), (1, 33, 17), (3, 50, 70)}
    assert {c.xfmt for c in S.CONV_CASES} == {"nchw", "cl", "crop"} and {c.wfmt for c in S.CONV_CASES} == {"nchw", "cl"}
    assert {c.stat for c in S.CONV_CASES} == {0, 1, 2} and {c.stat for c in S.CONV_CASES if c.N >= 770} >= {1, 2}
    assert {(c.Hz, c.Wz) for c in S.POOL_CASES} == {(1, 1), (2, 2), (3, 3), (4, 5), (17, 9)}
    assert {(c.C, c.obf) for c in S.POOL_CASES} == {(C, o) for C in (4, 8, 64) for o in (0, 1)}
    for c in S.POOL_CASES:
        assert {bool(v > 0) for v in S.pool_inputs(c)["ss"][:, 0]} == {True, False}


def test_inputs_hold_the_planted_edges():
    seen_z = 0
    for c in B.BWD_CASES + B.REDUCE_CASES:
        I = B.inputs(c)
        if c.bf16:
            for k in ("dy", "z", "y"):
                assert B.C16.is_bf16(I[k]), (c, k)
        y = I["y"].view(-1)
        if y.numel() >= 8:
            assert y[0] == 0 and not torch.signbit(y[0]) and torch.signbit(y[1]) and y[1] == 0 and y[2] == 2.0 ** -126 and y[4] < 0
        assert not bool(((I["y"] != 0) & (I["y"].abs() < 2.0 ** -126)).any())
        if type(c).__name__ == "BwdCase" and c.relu and not c.y and c.C >= 8 and c.R >= 8 and c.R != _DENSE[0]:
            on, xhat = B.CR.bn_mask(I["z"], I["mean"], I["invstd"], I["gamma"], I["beta"], False)
            t = xhat.numpy().astype(np.float64)
            exact = t * I["gamma"].numpy().astype(np.float64) + I["beta"].numpy().astype(np.float64)
            assert (exact[0, :4] == 0).all() and not on[0, :4].any() and (on[1, :4] != on[2, :4]).all(), c
            unfused = (t.astype(np.float32) * I["gamma"].numpy()).astype(np.float32) + I["beta"].numpy()
            seen_z += bool(((unfused <= 0) & on.numpy())[:, 4].any())
    assert seen_z >= 2


def test_mirrors_of_the_issue_examples():
    assert B.pick_chunks(1100, 4) == (18, 64) and B.pick_chunks(4200, 8) == (66, 64) and B.pick_chunks(16400, 4)[1] == 80
    assert B.pick_chunks(70, 2048)[0] == 2 and B.workspace_floats(72) == 256 * 2 * 72
    assert B.ew_blocks(B.DENSE[0] * B.DENSE[1] // 4) == 8192 and B.ew_blocks(10) == 1
    assert S.stem_tiles(32, 256, 256) == 768 and S.stem_tiles(770, 5, 5) == 768 and S.ldp(1, 1, 1) == 4
    with pytest.raises(ValueError):
        B.reduce_variant(0, 0, 1)
