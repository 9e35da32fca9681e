"""Stage-wise fp64 reference, geometry table, inputs, judges and a CPU evaluator with planted defects for the drivers of the
mixed-precision training Bottleneck: csrc/block16.cpp (scnattn_block16_sizes / _fwd / _bwd) and the two autograd nodes of
scnattn/conv16.py.  Shared by tests/test_block16_refs.py (CPU) and tests/test_gpu_block16_driver.py.

Chain of custody.  Both calls leave every stored map in caller-owned memory (save, stats, tmp, dgb, dw[i], the running
statistics, part, bnpart), so each stage is judged against fp64 of THAT STAGE applied to the driver's own stored inputs of
it, widened exactly: nothing amplifies through the block, no element is excluded, and the per-element bounds are the kernel
tier's (tests/conv16_refs.py, tests/bn_refs.py; U = 2^-24):

  products          b = (n + 8) U sum|terms| MFMA_WIDEN; a bf16 store b + 2^-8 (|ref| + b), an fp32 store (weight gradients) b
  BatchNorm maps    bn_refs' element tier on the STORED statistics (judge_y, dz_ref), a bf16 store + 2^-8 (|ref| + bound)
  masked elements   +0.0 bit for bit where the masked map itself is stored (dres); a ReLU mask is decided exactly, from the
                    stored bf16 z and the stored fp32 statistics (conv_refs.bn_mask) or from the stored activation (> 0)

Composites.  Three results are visible only after a later stage has overwritten them in place; they are judged fused, the
inner stage's bound tensor pushed through the absolute value of the outer stage's linear map, the outer stage's own
rounding term added:
  dz2   g2 = (dz3 . W3) [mask of bn2], stored bf16 with bound bg = b + 2^-8 (|ref| + b) on the kept elements, then bn2's dx in
        place: dz = gamma invstd (g - dbeta / R - xhat dgamma / R) with the STORED dbeta, dgamma, so only g carries an inner
        bound: |gamma invstd| bg, plus dz_ref's own 8 U term taken at |g| + bg, plus the bf16 store
  dz1   the same through conv2's d input: stride 1 with bn1's mask epilogue, stride 2 through the parity-class product (a
        bf16 store), a reduce with gout == dy (mask a1 > 0) and dx_fin in place
  dx    of an identity block: dres + dz1 . W1 with beta = 1; dres = dout [out > 0] is exact, so it is one more exact term
        of the product of the STORED dz1 (n + 1 terms)
  d beta, d gamma against the fp64 sums of the reference g: sum of the element bounds (times |xhat|) + (R + 8) U sum|terms|;
        the mask-epilogue slots that survive in bnpart the same per 64-row slot.

Statistics.  bn1's and bn2's partials do not survive the call (`part` is reused), so stats (mean, invstd) and the updated
running statistics are judged against the fp64 statistics of the EXACT product of the stored input map: the slot sums and
slot bounds of conv16_refs.stats_bf16_ref pushed through bn_refs.stats_of_partials' formulas with the slot bounds as one more
error of each slot (exact_stats), then bn_refs.judge_finalize (RSQRT_ULP included).  The surviving slots of `part` (bn3's)
and `bnpart` are judged directly, the sentinel in [row_tiles, stat_ld) included.

What the bounds assume is asserted here on the CPU: the fp64 variance of every channel is at least 1e-3 of its mean square
(of the shifted values the kernel sums), and every masked map has both cut and kept elements.

No tolerance is fitted to the driver: the only admissible widenings are conv16_refs.MFMA_WIDEN and bn_refs.RSQRT_ULP
(DESIGN.md 3)."""
import zlib
from collections import namedtuple

import numpy as np
import torch

import bn_refs as BN
import conv16_refs as C16
import conv_refs as CR

BF = torch.bfloat16
F64 = torch.float64
U, U8 = CR.U, C16.U8
SENT32, SENT16 = C16.SENT32, C16.SENT16
WS_FLOATS = 1 << 20

# ==== geometries: the smallest at which the composition can go wrong (bf16 widths are multiples of 64) =================
Geom = namedtuple("Geom", "id N Cin p Hi Wi s down why")
GEOMS = [
    Geom("i35", 1, 256, 64, 5, 7, 1, 0, "identity; R = 35: one partial 64-row tile, odd W"),
    Geom("i306", 2, 256, 64, 9, 17, 1, 0, "identity; 5 row tiles, stat_ld 8 > row_tiles; W not a multiple of 16"),
    Geom("d1", 2, 64, 64, 6, 5, 1, 1, "downsample at stride 1 (layer1.0): both part and bnpart live"),
    Geom("d2", 3, 256, 128, 6, 10, 2, 1, "stride 2: Rin 180, Rout 45; nine tap launches; parity-class dgrad; gather, scatter"),
    Geom("d2min", 2, 128, 64, 4, 2, 2, 1, "stride 2 at Rout = 4"),
]
EPS = (1e-5, 1e-3, 1e-5, 2e-5)              # two of the four differ from the default, so that an index mix-up shows
MOM = (0.1, 0.25, 0.1, 0.03)
STEPS = 2
# (need_dx, which dw[i] are non-null): what the GPU module runs besides the full call
VARIANTS = {"full": (1, (1, 1, 1, 1)), "no_dx": (0, (1, 1, 1, 1)), "no_dw": (1, (0, 0, 0, 0)), "conv2_frozen": (1, (1, 0, 1, 1))}


def by_id(gid):
    return next(g for g in GEOMS if g.id == gid)


def dims(g):
    """-> dict(C4, Ho, Wo, Rin, Rout, nbn, Cn = channels of BatchNorm i, Rn = its rows)"""
    Ho, Wo = (g.Hi - 1) // g.s + 1, (g.Wi - 1) // g.s + 1
    C4, Rin, Rout = 4 * g.p, g.N * g.Hi * g.Wi, g.N * Ho * Wo
    return dict(C4=C4, Ho=Ho, Wo=Wo, Rin=Rin, Rout=Rout, nbn=4 if g.down else 3, Cn=(g.p, g.p, C4, C4), Rn=(Rin, Rout, Rout, Rout))


def branches(g, variant):
    """the branches of csrc/block16.cpp a (geometry, variant) reaches"""
    need_dx, dws = VARIANTS[variant]
    return {("has_down", g.down), ("stride", g.s), ("need_dx", need_dx)} | {("dw%d" % i, int(bool(d))) for i, d in enumerate(dws)
                                                                            if i < 3 or g.down}


def carve(g):
    """The test's own carve: cumulative piece sizes in the header's order (save: z1 a1 | z2 a2 | z3 out | [zd idn]; tmp: dres
    dz3 | dz2 | dz1 | [dzd dx dxd]), each piece rounded up to 8 elements -> dict(save = {name: (offset, rows, cols)}, tmp,
    save_elems, tmp_elems, out_offset, stats_floats, dgb_floats)"""
    d = dims(g)
    p, C4, Cin, Ri, Ro = g.p, d["C4"], g.Cin, d["Rin"], d["Rout"]

    def lay(pieces):
        off, out = 0, {}
        for name, r, c in pieces:
            out[name] = (off, r, c)
            off += (r * c + 7) & ~7
        return out, off
    save, se = lay([("z1", Ri, p), ("a1", Ri, p), ("z2", Ro, p), ("a2", Ro, p), ("z3", Ro, C4), ("out", Ro, C4)] +
                   ([("zd", Ro, C4), ("idn", Ro, C4)] if g.down else []))
    tmp, te = lay([("dres", Ro, C4), ("dz3", Ro, C4), ("dz2", Ro, p), ("dz1", Ri, p)] +
                  ([("dzd", Ro, C4), ("dx", Ri, Cin), ("dxd", Ro, Cin)] if g.down else []))
    return dict(save=save, tmp=tmp, save_elems=se, tmp_elems=te, out_offset=save["out"][0], stats_floats=8 * C4, dgb_floats=8 * C4)


def part_floats(g):
    """floats `part` and `bnpart` must hold (include/scnattn.h; scnattn/block.py part_floats)"""
    d = dims(g)
    return 2 * max(g.p * CR.stat_ld(d["Rin"]), d["C4"] * CR.stat_ld(d["Rout"]))


# ==== inputs =============================================================================================================
_INPUTS = {}


def inputs(g):
    """seeded operands of a geometry: bf16 weights w[i] [Cout][taps][Cin] (scaled by K^-1/2) and their transposed copies, random
    BatchNorm vectors, running statistics and first-step shifts (distinct per BatchNorm), and per step x, dout (bf16)"""
    if g.id in _INPUTS:
        return _INPUTS[g.id]
    d = dims(g)
    gen = torch.Generator().manual_seed(80000 + zlib.crc32(repr(tuple(g[:8])).encode()) % 100000)
    rn = lambda *s: torch.randn(*s, generator=gen)
    shapes = [(g.p, 1, g.Cin), (g.p, 9, g.p), (d["C4"], 1, g.p), (d["C4"], 1, g.Cin)][:d["nbn"]]
    I = {"w": [(rn(*s) * (s[1] * s[2]) ** -0.5).to(BF) for s in shapes]}
    I["wt"] = [w.permute(2, 1, 0).contiguous() for w in I["w"]]
    sign = lambda C: 1 - 2 * (torch.arange(C) % 3 == 1).float()
    I["gamma"] = [(1 + 0.3 * rn(C)) * sign(C) for C in d["Cn"][:d["nbn"]]]
    I["beta"] = [0.2 * rn(C) for C in d["Cn"][:d["nbn"]]]
    I["run_mean"] = [0.5 * rn(C) for C in d["Cn"][:d["nbn"]]]
    I["run_var"] = [0.5 + torch.rand(C, generator=gen) for C in d["Cn"][:d["nbn"]]]
    I["shift"] = [0.1 * rn(C) for C in d["Cn"][:d["nbn"]]]
    I["x"] = [(torch.relu(rn(d["Rin"], g.Cin)) + 0.1 * rn(d["Rin"], g.Cin)).to(BF) for _ in range(STEPS)]
    I["dout"] = [rn(d["Rout"], d["C4"]).to(BF) for _ in range(STEPS)]
    _INPUTS[g.id] = I
    return I


def first_state(I):
    """what a step reads besides x and dout: shift, run_mean, run_var per BatchNorm"""
    return {k: [v.clone() for v in I[k]] for k in ("shift", "run_mean", "run_var")}


def next_state(g, S):
    """the state after a step that stored S: the next shift is the stored mean, the running statistics the updated ones"""
    d = dims(g)
    st = S["stats"].view(4, 2, d["C4"])
    return {"shift": [st[i, 0, :d["Cn"][i]].clone() for i in range(d["nbn"])], "run_mean": [v.clone() for v in S["run_mean"]],
            "run_var": [v.clone() for v in S["run_var"]]}


# ==== a tally instead of assertions: the judges are run on planted defects too ==========================================
class Tally:
    def __init__(self, gid=""):
        self.gid, self.ratios, self.fails = gid, {}, []

    def ok(self, stage, name, got, want, bound, kind="sum"):
        want = want.double()
        bound = bound.double().expand(want.shape)
        if got is None or got.numel() != want.numel():
            self.fails.append("%s %s: missing" % (stage, name))
            return
        err = (got.double().reshape(want.shape) - want).abs()
        r = float(C16._ratio(err, bound).max()) if err.numel() else 0.0
        key = "%s %s" % (stage, name)
        self.ratios[key] = max(self.ratios.get(key, 0.0), r)
        if not bool((err <= bound).all()):
            self.fails.append("%s: worst err/bound %.3f, %d NaN" % (key, r, int(got.float().isnan().sum())))

    def bits(self, stage, name, good, what):
        self.ratios["%s %s" % (stage, name)] = 0.0 if good else 1e30
        if not good:
            self.fails.append("%s %s: %s" % (stage, name, what))


def _i32(t):
    return t.float().contiguous().view(torch.int32)


def _is_sent(t):
    return bool((t.contiguous().view(torch.int32) == SENT32).all())


# ==== the stage references ===============================================================================================
def _w64(I, i):
    w = I["w"][i].double()
    return w[:, 0] if w.shape[1] == 1 else w


def _st(g, I, S, i):
    """the stored statistics and the parameters of BatchNorm i as bn_refs takes them"""
    C = dims(g)["Cn"][i]
    st = S["stats"].view(4, 2, -1)
    return {"mean": st[i, 0, :C], "invstd": st[i, 1, :C], "gamma": I["gamma"][i], "beta": I["beta"][i]}


def exact_stats(ref, b, shift, R):
    """bn_refs.stats_of_partials for partials that are not stored: the fp64 slot sums of the exact d = P - shift and their slot
    bounds (conv16_refs.stats_bf16_ref), each slot bound one more error of that slot in the formulas -> (s, slots, slot bounds)"""
    want, sb = C16.stats_bf16_ref(ref, shift, b)
    n = want.shape[2]
    s1, s2 = want[0], want[1]
    m1 = s1.sum(1) / R
    bm1 = (sb[0].sum(1) + (n + 8) * U * (s1.abs().sum(1) + sb[0].sum(1))) / R
    var = s2.sum(1) / R - m1 * m1
    bvar = (sb[1].sum(1) + (n + 8) * U * (s2.abs().sum(1) + sb[1].sum(1))) / R + 2 * m1.abs() * bm1 + bm1 * bm1 + 4 * U * m1 * m1
    return {"conditioned": bool((var >= 1e-3 * s2.sum(1) / R).all()), "mean": shift.double() + m1, "var": var.clamp_min(0.0), "var_raw": var, "m1": m1, "bm1": bm1, "bvar": bvar}, want, sb


def _product(T, stage, name, got, ref, bf16=True):
    b = CR.bound_of(ref) * C16.MFMA_WIDEN
    T.ok(stage, name, got, ref["out"], b + U8 * (ref["out"].abs() + b) if bf16 else b)
    return b


def _slots(T, stage, flat, C, R, want, sb, pad=True):
    """a flat partial window: [2][C][stat_ld(R)] in front, live slots against want within sb, the sentinel in [row_tiles, ld)"""
    mt, ld = CR.row_tiles(R), CR.stat_ld(R)
    part = flat[:2 * C * ld].view(2, C, ld)
    T.ok(stage, "slots", part[:, :, :mt], want, sb)
    if pad:
        T.bits(stage, "slot-pad", _is_sent(part[:, :, mt:]), "a slot in [row_tiles, stat_ld) lost the sentinel")


def same_tiles(g):
    """A scratch array is reused by stages over Rin rows and stages over Rout rows.  Where both have the same number of
    64-row tiles every writer leaves the same slots [tiles, ld) alone, and the last writer's padding must still be the
    sentinel; where they differ (d2: 3 tiles against 1) an earlier stage's live slot lies in the last writer's padding."""
    d = dims(g)
    return CR.row_tiles(d["Rin"]) == CR.row_tiles(d["Rout"])


def _bn_stage(T, g, I, state, S, i, stage, ref, b, R):
    """statistics of BatchNorm i from the exact product `ref` of its stored input: stats, running statistics"""
    s, want, sb = exact_stats(ref, b, state["shift"][i], R)
    T.bits(stage, "conditioning", s["conditioned"], "a channel's variance is below 1e-3 of its mean square: the bound assumes more")
    st = _st(g, I, S, i)
    out = {"mean": st["mean"], "invstd": st["invstd"], "run_mean": S["run_mean"][i], "run_var": S["run_var"][i]}
    BN.judge_finalize(stage, T.ok, None, None, state["shift"][i], R, out, {"run_mean": state["run_mean"][i], "run_var": state["run_var"][i]},
                      eps=EPS[i], momentum=MOM[i], s=s)
    return want, sb


def judge_fwd(g, I, t, state, S, T=None):
    """Every stored result of scnattn_block16_fwd (S: save maps by name, stats [8 * 4p], run_mean / run_var lists, part, bnpart
    flat windows) against fp64 of its stage on the stored inputs of it -> Tally"""
    T = T or Tally(g.id)
    d = dims(g)
    p, C4, Ri, Ro = g.p, d["C4"], d["Rin"], d["Rout"]
    x = I["x"][t]
    f = lambda name: S[name].double()
    # conv1, bn1
    ref = CR.conv1x1_fwd(x.double(), _w64(I, 0))
    b = _product(T, "conv1", "z1", S["z1"], ref)
    _bn_stage(T, g, I, state, S, 0, "bn1", ref, b, Ri)
    BN.judge_y("bn1", T.ok, S["z1"].float(), None, _st(g, I, S, 0), 1, S["a1"], True)
    # conv2, bn2
    ref = CR.conv3_fwd(f("a1"), _w64(I, 1), CR.fwd_taps(g.N, g.Hi, g.Wi, g.s))
    b = _product(T, "conv2", "z2", S["z2"], ref)
    _bn_stage(T, g, I, state, S, 1, "bn2", ref, b, Ro)
    BN.judge_y("bn2", T.ok, S["z2"].float(), None, _st(g, I, S, 1), 1, S["a2"], True)
    # conv3, bn3 (its partials survive in `part`)
    ref = CR.conv1x1_fwd(f("a2"), _w64(I, 2))
    b = _product(T, "conv3", "z3", S["z3"], ref)
    want, sb = _bn_stage(T, g, I, state, S, 2, "bn3", ref, b, Ro)
    _slots(T, "bn3 part", S["part"], C4, Ro, want, sb, pad=same_tiles(g))
    res = x.float()
    st = S["stats"].view(4, 2, C4)
    T.bits("stats", "unused", _is_sent(st[:2, :, p:]) and (g.down or _is_sent(st[3])), "an unused word of stats was written")
    if g.down:
        ref = CR.conv1x1_fwd(x.double(), _w64(I, 3), CR.gather_rows(g.N, g.Hi, g.Wi, g.s) if g.s > 1 else None)
        b = _product(T, "down", "zd", S["zd"], ref)
        want, sb = _bn_stage(T, g, I, state, S, 3, "bnd", ref, b, Ro)
        _slots(T, "bnd bnpart", S["bnpart"], C4, Ro, want, sb)
        BN.judge_y("bnd", T.ok, S["zd"].float(), None, _st(g, I, S, 3), 0, S["idn"], True)
        res = S["idn"].float()
    else:
        T.bits("bnpart", "unused", _is_sent(S["bnpart"]), "the forward call of an identity block wrote to bnpart")
    BN.judge_y("bn3", T.ok, S["z3"].float(), res, _st(g, I, S, 2), 1, S["out"], True)
    return T


def _sums(T, stage, gref, bg, xh, R, got_db, got_dg):
    """d beta, d gamma against the fp64 sums of the reference g: sum of the element bounds + (R + 8) U sum|terms|"""
    T.ok(stage, "dbeta", got_db, gref.sum(0), bg.sum(0) + (R + 8) * U * gref.abs().sum(0))
    T.ok(stage, "dgamma", got_dg, (gref * xh).sum(0), (bg * xh.abs()).sum(0) + (R + 8) * U * (gref * xh).abs().sum(0))


def _masked_bn_bwd(T, stage, P, on, z, st, dgb_i, R, got_dz):
    """A masked d-input product seen only through the BatchNorm's dx written over it (module docstring) -> (g, bg, xhat)"""
    T.bits(stage, "mask mix", bool(on.any()) and not bool(on.all()), "the mask does not both cut and keep: the inputs are too easy")
    bP = CR.bound_of(P) * C16.MFMA_WIDEN
    zero = torch.zeros((), dtype=F64)
    gref = torch.where(on, P["out"], zero)
    bg = torch.where(on, bP + U8 * (P["out"].abs() + bP), zero)
    xh = BN.xhat64(z.float(), st)
    C = gref.shape[1]
    db, dg = dgb_i[0, :C], dgb_i[1, :C]
    _sums(T, stage, gref, bg, xh, R, db, dg)
    want, b = BN.dz_ref(gref, xh, st, db, dg, R, 1)
    gi = (st["gamma"].double() * st["invstd"].double()).abs()
    b = b + (1 + 8 * U) * gi * bg
    T.ok(stage, "dz", got_dz, want, b + U8 * (want.abs() + b))
    return gref, bg, xh


def _plain_bn_bwd(T, stage, gq, z, st, dgb_i, R, got_dz):
    """BatchNorm backward from a STORED (or exactly known) g: sums and dz"""
    xh = BN.xhat64(z.float(), st)
    db, dg = dgb_i[0], dgb_i[1]
    _sums(T, stage, gq, torch.zeros_like(gq), xh, R, db, dg)
    want, b = BN.dz_ref(gq, xh, st, db, dg, R, 1)
    T.ok(stage, "dz", got_dz, want, b + U8 * (want.abs() + b))
    return xh


def tap_table(g, transposed=False):
    """source rows [Rout][9] of conv2's weight gradient: stride 1 the forward taps, stride 2 the nine gathered launches, tap
    t = (dh, dw) at offsets (dh - 1, dw - 1); transposed plants the defect (dw - 1, dh - 1)"""
    if g.s == 1 and not transposed:
        return CR.fwd_taps(g.N, g.Hi, g.Wi, 1)
    return torch.stack([C16.tap_rows(g.N, g.Hi, g.Wi, g.s, *((t % 3 - 1, t // 3 - 1) if transposed else (t // 3 - 1, t % 3 - 1)))
                        for t in range(9)], 1)


def dx_sum(g, dx, dxd):
    """what the caller does with dx_out / dxd_out of a downsample block: dxd added into the strided rows, one bf16 rounding"""
    d = dims(g)
    out = dx.clone()
    out.view(g.N, g.Hi, g.Wi, g.Cin)[:, ::g.s, ::g.s].add_(dxd.view(g.N, d["Ho"], d["Wo"], g.Cin))
    return out


def judge_bwd(g, I, t, S, variant="full", T=None):
    """Every stored result of scnattn_block16_bwd (S additionally: tmp maps by name -- None where the call does not leave one
    --, dgb [8 * 4p], dw list (None: NULL), bnpart, and dx_final where the caller's add was made) -> Tally"""
    T = T or Tally(g.id)
    need_dx, dws = VARIANTS[variant]
    d = dims(g)
    p, C4, Ri, Ro, Cin = g.p, d["C4"], d["Rin"], d["Rout"], g.Cin
    x, dout = I["x"][t], I["dout"][t]
    f = lambda name: S[name].double()
    dgb = S["dgb"].view(4, 2, C4)
    T.bits("dgb", "unused", _is_sent(dgb[:2, :, p:]) and (g.down or _is_sent(dgb[3])), "an unused word of dgb was written")
    # bn3 (+ identity + relu): dres = dout [out > 0], exact
    on3 = S["out"].float() > 0
    T.bits("bn3", "mask mix", bool(on3.any()) and not bool(on3.all()), "the mask does not both cut and keep: the inputs are too easy")
    dres = torch.where(on3, dout, torch.zeros((), dtype=BF))
    if S.get("dres") is not None:
        T.bits("bn3", "dres", torch.equal(_i32(S["dres"]), _i32(dres)), "dres is not dout / +0.0 bit for bit")
    _plain_bn_bwd(T, "bn3 bwd", dres.double(), S["z3"], _st(g, I, S, 2), dgb[2], Ro, S["dz3"])
    # conv3: weight gradient, d input through bn2's mask, bn2's dx in place
    if dws[2]:
        _product(T, "conv3", "dw", S["dw"][2], CR.conv1x1_wgrad(f("dz3"), f("a2")), False)
    st1 = _st(g, I, S, 1)
    on2 = CR.bn_mask(S["z2"].float(), st1["mean"], st1["invstd"], st1["gamma"], st1["beta"], False)[0]
    _masked_bn_bwd(T, "conv3 d-in + bn2 bwd", CR.conv1x1_dgrad(f("dz3"), _w64(I, 2)), on2, S["z2"], st1, dgb[1], Ro, S["dz2"])
    # conv2: weight gradient, d input, bn1
    if dws[1]:
        _product(T, "conv2", "dw", S["dw"][1], CR.conv3_wgrad(f("dz2"), f("a1"), tap_table(g), per_tap=True), False)
    st0 = _st(g, I, S, 0)
    if g.s == 1:
        on1 = CR.bn_mask(S["z1"].float(), st0["mean"], st0["invstd"], st0["gamma"], st0["beta"], False)[0]
    else:
        on1 = S["a1"].float() > 0
    P1 = CR.conv3_dgrad(f("dz2"), _w64(I, 1), CR.dgrad_taps(g.N, g.Hi, g.Wi, g.s))
    g1, bg1, xh1 = _masked_bn_bwd(T, "conv2 d-in + bn1 bwd", P1, on1, S["z1"], st0, dgb[0], Ri, S["dz1"])
    if dws[0]:
        _product(T, "conv1", "dw", S["dw"][0], CR.conv1x1_wgrad(f("dz1"), x.double()), False)
    # identity branch and d x
    if g.down:
        std = _st(g, I, S, 3)
        xhd = _plain_bn_bwd(T, "bnd bwd", dres.double(), S["zd"], std, dgb[3], Ro, S["dzd"])
        if dws[3]:
            _product(T, "down", "dw", S["dw"][3],
                     CR.conv1x1_wgrad(f("dzd"), x.double(), CR.gather_rows(g.N, g.Hi, g.Wi, g.s) if g.s > 1 else None), False)
        if need_dx:
            _product(T, "conv1", "dx", S["dx"], CR.conv1x1_dgrad(f("dz1"), _w64(I, 0)))
            _product(T, "down", "dxd", S["dxd"], CR.conv1x1_dgrad(f("dzd"), _w64(I, 3)))
            if S.get("dx_final") is not None:      # one more bf16 rounding of the fp32 sum of two judged maps
                want = dx_sum(g, S["dx"].double(), S["dxd"].double())
                T.ok("dx + dxd", "dx", S["dx_final"], want, (U8 + 2 * U) * want.abs())
        else:
            T.bits("tmp", "no dx", S.get("dx") is None and S.get("dxd") is None, "dx / dxd written with need_dx == 0")
        # the reduce pass of the downsample's BatchNorm wrote bnpart last: chunk-major slots of the exact g
        nch, rpc = BN.pick_chunks(Ro, C4)
        ldp = BN.ldp_of(nch)
        part = S["bnpart"][:2 * C4 * ldp].view(2, C4, ldp)
        BN.judge_slots("bnd bwd bnpart", T.ok, part[:, :, :nch].permute(0, 2, 1), dres.double(), dres.double() * xhd,
                       torch.arange(Ro) // rpc, nch)
        if same_tiles(g):
            T.bits("bnd bwd bnpart", "slot-pad", _is_sent(part[:, :, nch:]), "a slot in [nchunk, ldp) lost the sentinel")
    else:
        if need_dx:
            _product(T, "conv1", "dx", S["dx"], CR.conv1x1_dgrad(f("dz1"), _w64(I, 0), 1.0, dres.double()))
        # bn1's mask epilogue wrote bnpart last: per slot the sums of its own rounded g, seen through the reference g
        r = CR.block_rows(Ri)[0]
        want = torch.stack([CR.block_sums(g1), CR.block_sums(g1 * xh1)])
        sb = torch.stack([CR.block_sums(bg1) + (r + 8) * U * CR.block_sums(g1.abs()),
                          CR.block_sums(bg1 * xh1.abs()) + (r + 8) * U * CR.block_sums((g1 * xh1).abs())])
        _slots(T, "bn1 bwd bnpart", S["bnpart"], p, Ri, want, sb)
    return T


# ==== an honest fp32 / bf16 evaluation of the driver's sequence on the CPU, and the planted composition defects =========
DEFECTS = ("bn2_reads_bn1", "stats_ld_p", "drop_last_tile", "down_relu", "identity_from_x", "down_gets_dout", "dx_beta0",
           "dgb_swapped", "taps_transposed", "dxd_not_added", "dxd_rows", "run_var_biased")


def applies(defect, g):
    d = dims(g)
    if defect == "drop_last_tile":               # more than one tile and the last one partial, for some BatchNorm
        return any(R > 64 and R % 64 for R in (d["Rin"], d["Rout"]))
    if defect in ("down_relu", "identity_from_x", "down_gets_dout", "dxd_not_added"):
        return bool(g.down)
    if defect == "dx_beta0":
        return not g.down
    if defect in ("taps_transposed", "dxd_rows"):
        return g.s == 2
    return True


def _sent(n):
    return torch.full((n,), SENT32, dtype=torch.int32).view(torch.float32).clone()


def _f32(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


def cpu_eval(g, I, t, state, defect=None, variant="full"):
    """Each stage in fp32 from the bf16-rounded stored maps, one rounding per stored map -> S as the judges take it (forward
    and backward, with dx_final for a downsample block); `defect` plants one composition defect."""
    need_dx, dws = VARIANTS[variant]
    d = dims(g)
    p, C4, Ri, Ro, Cin, nbn = g.p, d["C4"], d["Rin"], d["Rout"], g.Cin, d["nbn"]
    x, dout = I["x"][t], I["dout"][t]
    w = lambda i: (I["w"][i].float()[:, 0] if I["w"][i].shape[1] == 1 else I["w"][i].float())
    S = {"stats": _sent(8 * C4), "dgb": _sent(8 * C4), "part": _sent(part_floats(g)), "bnpart": _sent(part_floats(g)),
         "run_mean": [None] * nbn, "run_var": [None] * nbn, "dw": [None] * 4}
    ld4 = p if defect == "stats_ld_p" else C4

    def put(flat, i, which, v):
        o = (2 * i + which) * ld4
        flat[o:o + v.numel()] = v

    def slots_into(flat, a, bb, R):
        C = a.shape[1]
        mt, ld = CR.row_tiles(R), CR.stat_ld(R)
        flat[:2 * C * ld].view(2, C, ld)[:, :, :mt] = torch.stack([CR.block_sums(a), CR.block_sums(bb)])
        return flat[:2 * C * ld].view(2, C, ld)[:, :, :mt]

    def bn_fwd(i, acc, R, flat, res, relu, gb=None):
        """statistics of the fp32 accumulators, the finalize, the stored z and y"""
        dd = acc - state["shift"][i]
        live = slots_into(flat, dd, dd * dd, R)
        if defect == "drop_last_tile" and R > 64 and R % 64:
            live = live[:, :, :-1]
        m1 = live[0].sum(1) / R
        mean = state["shift"][i] + m1
        var = (live[1].sum(1) / R - m1 * m1).clamp_min(0.0)
        invstd = torch.rsqrt(var + _f32(EPS[i]))
        om, m = (_f32(v) for v in BN.mom_pair(MOM[i]))
        S["run_mean"][i] = om * state["run_mean"][i] + m * mean
        S["run_var"][i] = om * state["run_var"][i] + m * var * (1.0 if defect == "run_var_biased" or R == 1 else R / (R - 1.0))
        put(S["stats"], i, 0, mean)
        put(S["stats"], i, 1, invstd)
        z = acc.to(BF)
        gb = i if gb is None else gb
        y = ((z.float() - mean) * invstd) * I["gamma"][gb] + I["beta"][gb]
        if res is not None:
            y = y + res
        return z, (torch.relu(y) if relu else y).to(BF), (mean, invstd)

    # ---- forward
    S["z1"], S["a1"], s0 = bn_fwd(0, x.float() @ w(0).t(), Ri, S["part"], None, True)
    acc = CR.conv3_fwd(S["a1"].float(), w(1), CR.fwd_taps(g.N, g.Hi, g.Wi, g.s))["out"]
    S["z2"], S["a2"], s1 = bn_fwd(1, acc, Ro, S["part"], None, True, gb=0 if defect == "bn2_reads_bn1" else None)
    acc3 = S["a2"].float() @ w(2).t()
    res = x.float()
    if g.down:
        xs = x.float() if g.s == 1 else x.float()[CR.gather_rows(g.N, g.Hi, g.Wi, g.s)]
        S["zd"], S["idn"], sd = bn_fwd(3, xs @ w(3).t(), Ro, S["bnpart"], None, defect == "down_relu")
        res = S["idn"].float()
        if defect == "identity_from_x":          # x read as if it were the [Rout][4p] identity
            res = x.float().reshape(-1).repeat(Ro * C4 // x.numel() + 1)[:Ro * C4].view(Ro, C4)
    S["z3"], S["out"], s2 = bn_fwd(2, acc3, Ro, S["part"], res, True)
    S["bnpart_fwd"] = S["bnpart"].clone()

    # ---- backward
    def bn_dx(i, gq, z, stat, sums):
        gi = I["gamma"][i] * stat[1]
        xh = (z.float() - stat[0]) * stat[1]
        db, dg = sums if defect != "dgb_swapped" else sums[::-1]
        put(S["dgb"], i, 0, db)
        put(S["dgb"], i, 1, dg)
        return (gi * (gq - db / R_(z) - xh * dg / R_(z))).to(BF)

    R_ = lambda z: float(z.shape[0])

    def chunk_sums(gq, xh, R, C):                  # the reduce pass: chunk-major partials into bnpart
        nch, rpc = BN.pick_chunks(R, C)
        ldp = BN.ldp_of(nch)
        part = S["bnpart"][:2 * C * ldp].view(2, C, ldp)
        for k in range(nch):
            rows = slice(k * rpc, min((k + 1) * rpc, R))
            part[0, :, k], part[1, :, k] = gq[rows].sum(0), (gq[rows] * xh[rows]).sum(0)
        return part[0, :, :nch].sum(1), part[1, :, :nch].sum(1)

    def mask_sums(gq, xh, R):                      # the mask epilogue: 64-row slots into bnpart
        live = slots_into(S["bnpart"], gq, gq * xh, R)
        return live[0].sum(1), live[1].sum(1)

    xhat = lambda z, stat: (z.float() - stat[0]) * stat[1]
    dres = torch.where(S["out"].float() > 0, dout, torch.zeros((), dtype=BF))
    S["dz3"] = bn_dx(2, dres.float(), S["z3"], s2, chunk_sums(dres.float(), xhat(S["z3"], s2), Ro, C4))
    if dws[2]:
        S["dw"][2] = S["dz3"].float().t() @ S["a2"].float()
    on2 = CR.bn_mask(S["z2"].float(), s1[0], s1[1], I["gamma"][1], I["beta"][1], False)[0]
    g2 = torch.where(on2, S["dz3"].float() @ w(2), torch.zeros(())).to(BF).float()
    S["dz2"] = bn_dx(1, g2, S["z2"], s1, mask_sums(g2, xhat(S["z2"], s1), Ro))
    if dws[1]:
        S["dw"][1] = CR.conv3_wgrad(S["dz2"].float(), S["a1"].float(), tap_table(g, defect == "taps_transposed"))["out"]
    P1 = CR.conv3_dgrad(S["dz2"].float(), w(1), CR.dgrad_taps(g.N, g.Hi, g.Wi, g.s))["out"]
    if g.s == 1:
        on1 = CR.bn_mask(S["z1"].float(), s0[0], s0[1], I["gamma"][0], I["beta"][0], False)[0]
        g1 = torch.where(on1, P1, torch.zeros(())).to(BF).float()
        sums = mask_sums(g1, xhat(S["z1"], s0), Ri)
    else:
        g1 = torch.where(S["a1"].float() > 0, P1.to(BF).float(), torch.zeros(()))
        sums = chunk_sums(g1, xhat(S["z1"], s0), Ri, p)
    S["dz1"] = bn_dx(0, g1, S["z1"], s0, sums)
    if dws[0]:
        S["dw"][0] = S["dz1"].float().t() @ x.float()
    S["dres"] = dres
    if g.down:
        gd = (dout if defect == "down_gets_dout" else dres).float()
        S["dzd"] = bn_dx(3, gd, S["zd"], sd, chunk_sums(gd, xhat(S["zd"], sd), Ro, C4))
        if dws[3]:
            S["dw"][3] = S["dzd"].float().t() @ xs
        if need_dx:
            S["dx"], S["dxd"] = (S["dz1"].float() @ w(0)).to(BF), (S["dzd"].float() @ w(3)).to(BF)
            if defect == "dxd_not_added":
                S["dx_final"] = S["dx"].clone()
            elif defect == "dxd_rows":
                S["dx_final"] = S["dx"].clone()
                S["dx_final"].view(g.N, g.Hi, g.Wi, Cin)[:, :d["Ho"], :d["Wo"]].add_(S["dxd"].view(g.N, d["Ho"], d["Wo"], Cin))
            else:
                S["dx_final"] = dx_sum(g, S["dx"], S["dxd"])
    elif need_dx:
        S["dx"] = (S["dz1"].float() @ w(0) + (0.0 if defect == "dx_beta0" else dres.float())).to(BF)
        S["dres"] = None                           # overwritten in place
    return S


def judge_step(g, I, t, state, S, variant="full"):
    T = judge_fwd(g, I, t, state, dict(S, bnpart=S.get("bnpart_fwd", S["bnpart"])))
    return judge_bwd(g, I, t, S, variant, T)


# ==== refusals: a mutation of the valid struct of geometry d1, the calls that must refuse it, words of the message ========
REFUSAL_GEOM = "d1"


def refusals(g):
    """[(fields to change -- (i, v): element i of an array field --, ("fwd", "bwd") which calls, words of scnattn_last_error)]
    for the valid struct of geometry d1: wrong geometry, null buffers and parameters, a bnpart that is too small"""
    assert g.id == REFUSAL_GEOM
    d = dims(g)
    need_bnd = 2 * d["C4"] * CR.stat_ld(d["Rout"])
    both, fwd, bwd = ("fwd", "bwd"), ("fwd",), ("bwd",)
    return [
        (dict(p=96), both, b"multiples of 64"), (dict(Cin=96), both, b"multiples of 64"),
        (dict(stride=2, Hi=5), both, b"even maps"), (dict(stride=2, Wi=5, Hi=6), both, b"even maps"),
        (dict(has_down=0), both, b"keeps its shape"), (dict(has_down=0, Cin=256, stride=2, Wi=4), both, b"keeps its shape"),
        (dict(stride=3), both, b"geometry"), (dict(N=0), both, b"geometry"),
        (dict(x=None), both, b"null buffer"), (dict(save=None), both, b"null buffer"), (dict(stats=None), both, b"null buffer"),
        (dict(ws=None), both, b"null buffer"), (dict(bnpart=None), both, b"null buffer"), (dict(part=None), fwd, b"null buffer"),
        (dict(dout=None), bwd, b"null buffer"), (dict(tmp=None), bwd, b"null buffer"), (dict(dgb=None), bwd, b"null buffer"),
        (dict(gamma=(1, None)), both, b"null parameter"), (dict(beta=(3, None)), both, b"null parameter"),
        (dict(w=(2, None)), fwd, b"null parameter"), (dict(wt=(0, None)), bwd, b"null parameter"),
        (dict(bnpart_floats=need_bnd - 1), fwd, b"bnpart too small"), (dict(bnpart_floats=part_floats(g) - 1), bwd, b"bnpart too small"),
        (dict(bnpart_floats=0), both, b"bnpart too small"),
    ]
