"""fp64 references of the fp32 convolution forms of the trunk (include/scnattn.h: scnattn_cgemm with a
scnattn_conv_extra, scnattn_conv1x1_fwd / _dgrad / _wgrad, scnattn_conv3x3_fwd / _dgrad / _dgrad_strided / _wgrad,
the two _bn_eval forms), the case tables of tests/test_gpu_conv_kernels.py, their inputs, the judges, and `name`, which
renders the launch plan of a case's own call (scnattn_plan_next) as the kernel instance and second launch it reaches.

Written from the header comments.  Row gathers, the nine taps and the zero padding are plain index arithmetic here
(gather_rows, fwd_taps, dgrad_taps): an index table [rows][9] of source rows, -1 where the tap falls outside the image.
Nothing comes from F.conv2d; tests/test_conv_refs.py compares the two.  Like tests/gemm_refs.py every product computes in
the dtype of its operands and carries `out_abs` (sum of the magnitudes of the terms of each element) and `out_n` (their
number: the K of the launch) for the bound (n + 8) * 2^-24 * sum|terms| of DESIGN.md 3.

Which product an entry point launches, the row tile, the split and the second launch are never restated here: the GPU
module asks the library (test_gpu_conv_kernels.dispatch).  What stays is layout arithmetic that bears on expected values
(row_tiles, stat_ld, out_hw, rows_in / rows_out, the tap tables).
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

from scnattn import _lib as L

U = 2.0 ** -24
SROWS = 64                  # rows per statistics partial (SROWS of csrc/cgemm.hip)
OPTION_DEFAULTS = {"cgemm_combine": 1, "cgemm_mi": 0}


def cdiv(a, b):
    return -(-a // b)


def row_tiles(M):
    return cdiv(M, SROWS)


def stat_ld(M):
    return (cdiv(M, SROWS) + 3) & ~3


# ==== cases ==============================================================================================================
# op:  f1 / d1 / w1  1x1 forward / d input / d weight;  f3 / d3 / s3 / w3  3x3 forward / d input (stride 1) / d input
#      (stride 2) / d weight on the gathered form;  h3  3x3 d weight on the halo-staged kernel
# N, Hi, Wi: the INPUT map; an un-gathered 1x1 product of R rows is N = R maps of 1 x 1.  s: stride
# pro / epi: scnattn_conv_extra (epi 3: the _bn_eval entry point)
# var: flags -- s stat_shift given, f folded mask (pro_ss), t w_transposed, b beta = 1, r residual, l ReLU,
#      g through scnattn_cgemm itself with lda / ldb / ldc wider than the rows
# mi / split: force_mi / force_split (h3, w3: k_slices);  ws: a workspace is passed;  opts: scnattn_set_option values
Case = namedtuple("Case", "op N Hi Wi Cin Cout s pro epi var mi split ws opts")


def case(op, N, Hi, Wi, Cin, Cout, s=1, pro=0, epi=0, var="", mi=0, split=0, ws=1, opts=None):
    return Case(op, N, Hi, Wi, Cin, Cout, s, pro, epi, var, mi, split, ws, dict(opts or {}))


def case_id(c):
    o = "".join("-%s%d" % (k.replace("cgemm_", ""), v) for k, v in sorted(c.opts.items()))
    return "%s-%dx%dx%d-%dto%d-s%d-p%de%d%s-mi%d-S%d-ws%d%s" % (c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, c.pro, c.epi,
                                                                 c.var, c.mi, c.split, c.ws, o)


def out_hw(c):
    return (c.Hi - 1) // c.s + 1, (c.Wi - 1) // c.s + 1


def rows_in(c):
    return c.N * c.Hi * c.Wi


def rows_out(c):
    Ho, Wo = out_hw(c)
    return c.N * Ho * Wo


def out_shape(c):
    """(rows, columns) of the output map / weight gradient"""
    if c.op in ("f1", "f3"):
        return rows_out(c), c.Cout
    if c.op in ("d1", "d3", "s3"):
        return rows_in(c), c.Cin
    return c.Cout, (9 if c.op in ("w3", "h3") else 1) * c.Cin


def stat_rows(c):
    """rows the statistics partials of the case run over (None: no partials)"""
    return out_shape(c)[0] if c.epi in (1, 2) else None


def ws_floats(c):
    r, n = out_shape(c)
    return 16 * r * n if c.ws else 0


# ==== instance names, rendered from the launch plan of the real call (scnattn_plan_next) ===============================
_SECOND = {L.SECOND_NONE: None, L.SECOND_CSTATS1: "cstats<1> from slabs", L.SECOND_CSTATS2_SLABS: "cstats<2> from slabs",
           L.SECOND_CSTATS2_C: "cstats<2> from C", L.SECOND_CGEMM_REDUCE: "creduce<1>"}


def name(p):
    """launch plan -> (instance, second launch or None, info): the kernel names of the parity report and the fields the
    row selections read"""
    if p.family == L.PLAN_CONV3_WGRAD:
        return "conv3_wgrad<%d>" % p.seg, _SECOND[p.second], dict(S=p.S, Q=p.Q, ntiles=p.ntiles)
    assert p.family == L.PLAN_CGEMM
    lay = {(0, 1): "NT", (0, 0): "NN", (1, 0): "TN", (1, 1): "TT"}[(p.tA, p.tB)]
    inst = "cgemm<MI%d %s PRO%d EPI%d G%d C3_%d>" % (p.mi, lay, p.pro, p.epi, p.gather, p.c3)
    second = "creduce<%d>" % p.vec if p.second == L.SECOND_CREDUCE else _SECOND[p.second]
    return inst, second, dict(S=p.S, kper=p.kper, mi=p.mi, comb=bool(p.in_launch), tiles=p.tiles)


# ==== index tables =======================================================================================================
def _grid(N, H, W):
    n, h, w = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    return n.reshape(-1), h.reshape(-1), w.reshape(-1)


def gather_rows(N, Hi, Wi, s):
    """strided 1x1 convolution: output row (n, ho, wo) reads input row (n, ho * s, wo * s) of the Hi x Wi map"""
    n, ho, wo = _grid(N, (Hi - 1) // s + 1, (Wi - 1) // s + 1)
    return (n * Hi + ho * s) * Wi + wo * s


def fwd_taps(N, Hi, Wi, s):
    """3x3, padding 1: output row (n, ho, wo), tap (dh, dw) reads input row (n, ho*s + dh - 1, wo*s + dw - 1), -1 outside"""
    n, ho, wo = _grid(N, (Hi - 1) // s + 1, (Wi - 1) // s + 1)
    cols = []
    for dh in range(3):
        for dw in range(3):
            hi, wi = ho * s + dh - 1, wo * s + dw - 1
            ok = (hi >= 0) & (hi < Hi) & (wi >= 0) & (wi < Wi)
            cols.append(torch.where(ok, (n * Hi + hi) * Wi + wi, torch.full_like(n, -1)))
    return torch.stack(cols, 1)


def dgrad_taps(N, Hi, Wi, s):
    """d input: input row (n, hi, wi), tap (dh, dw) reads dy row (n, (hi + 1 - dh) / s, (wi + 1 - dw) / s) when both
    divisions are exact and the pixel lies in the Ho x Wo map; -1 otherwise"""
    Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
    n, hi, wi = _grid(N, Hi, Wi)
    cols = []
    for dh in range(3):
        for dw in range(3):
            th, tw = hi + 1 - dh, wi + 1 - dw
            ok = (th >= 0) & (tw >= 0) & (th % s == 0) & (tw % s == 0)
            ho, wo = torch.div(th, s, rounding_mode="floor"), torch.div(tw, s, rounding_mode="floor")
            ok = ok & (ho < Ho) & (wo < Wo)
            cols.append(torch.where(ok, (n * Ho + ho) * Wo + wo, torch.full_like(n, -1)))
    return torch.stack(cols, 1)


def take_rows(x, idx):
    """x [rows][C], idx [...] -> x[idx] with a zero row where idx == -1"""
    return torch.cat([x, x.new_zeros(1, x.shape[1])])[idx]


# ==== products ===========================================================================================================
def prologue(x, ss):
    """relu(x * scale[c] + shift[c]), ss [C][2] = {scale, shift}"""
    return torch.relu(x * ss[:, 0] + ss[:, 1])


def _res(out, out_abs, n):
    return {"out": out, "out_abs": out_abs, "out_n": n}


def conv1x1_fwd(a, w, rows=None):
    """y [R][Cout] = a[rows] . w^T, w [Cout][Cin]"""
    if rows is not None:
        a = a[rows]
    return _res(a @ w.t(), a.abs() @ w.abs().t(), w.shape[1])


def conv1x1_dgrad(dy, w, beta=0.0, dx0=None):
    """dx [R][Cin] = dy . w (+ beta * dx0)"""
    dx, dx_abs, n = dy @ w, dy.abs() @ w.abs(), w.shape[0]
    if beta != 0.0:
        dx, dx_abs, n = dx + beta * dx0, dx_abs + (beta * dx0).abs(), n + 1
    return _res(dx, dx_abs, n)


def conv1x1_wgrad(dy, a, rows=None):
    """dw [Cout][Cin] = dy^T . a[rows]"""
    if rows is not None:
        a = a[rows]
    return _res(dy.t() @ a, dy.abs().t() @ a.abs(), dy.shape[0])


def conv3_fwd(x, w, idx):
    """y [(n,ho,wo)][co] = sum over tap, ci of x[idx[row][tap]][ci] * w[co][tap][ci]; w [Cout][9][Cin]"""
    xg = take_rows(x, idx)
    return _res(torch.einsum("rtc,otc->ro", xg, w), torch.einsum("rtc,otc->ro", xg.abs(), w.abs()), 9 * x.shape[1])


def conv3_dgrad(dy, w, idx):
    """dx [(n,hi,wi)][ci] = sum over tap, co of dy[idx[row][tap]][co] * w[co][tap][ci]"""
    dg = take_rows(dy, idx)
    return _res(torch.einsum("rto,otc->rc", dg, w), torch.einsum("rto,otc->rc", dg.abs(), w.abs()), 9 * dy.shape[1])


def conv3_wgrad(dy, x, idx, per_tap=False):
    """dw [co][tap * Cin + ci] = sum over rows of dy[row][co] * x[idx[row][tap]][ci].  n = the rows (the K of the gathered
    launch), or with per_tap the in-image terms of each tap (the halo kernel)"""
    xg = take_rows(x, idx)
    Co, Ci = dy.shape[1], x.shape[1]
    n = (idx >= 0).sum(0).double().repeat_interleave(Ci).reshape(1, 9 * Ci) if per_tap else dy.shape[0]
    return _res(torch.einsum("ro,rtc->otc", dy, xg).reshape(Co, 9 * Ci),
                torch.einsum("ro,rtc->otc", dy.abs(), xg.abs()).reshape(Co, 9 * Ci), n)


def bound_of(ref, extra=0):
    return (ref["out_n"] + 8 + extra) * U * ref["out_abs"].double()


# ==== epilogues ==========================================================================================================
def block_sums(v):
    """v [rows][C] -> [C][row_tiles(rows)]: sums over each block of 64 rows (the last one shorter)"""
    rows, C = v.shape
    mt = row_tiles(rows)
    pad = torch.cat([v, v.new_zeros(mt * SROWS - rows, C)])
    return pad.reshape(mt, SROWS, C).sum(1).t().contiguous()


def block_rows(rows):
    mt = row_tiles(rows)
    return torch.tensor([min(SROWS, rows - b * SROWS) for b in range(mt)], dtype=torch.float64).reshape(1, 1, mt)


def stats_ref(y, shift):
    """partials [2][C][mt] of a STORED output y (fp32 values): sum(y - s), sum((y - s)^2) per channel and 64-row block, in fp64.
    Terms: the differences, one per row (each rounded once by the kernel, which the + 8 covers)."""
    d = y.double() - (0.0 if shift is None else shift.double())
    return {"out": torch.stack([block_sums(d), block_sums(d * d)]),
            "out_abs": torch.stack([block_sums(d.abs()), block_sums(d * d)]), "out_n": block_rows(y.shape[0])}


def mask_stats_ref(g, xhat):
    """partials [2][C][mt] of a STORED masked gradient g: sum(g), sum(g * xhat)"""
    g, xhat = g.double(), xhat.double()
    return {"out": torch.stack([block_sums(g), block_sums(g * xhat)]),
            "out_abs": torch.stack([block_sums(g.abs()), block_sums((g * xhat).abs())]), "out_n": block_rows(g.shape[0])}


def bn_mask(z, mean, invstd, a, b, folded):
    """The ReLU mask exactly as bn_relu_on (csrc/tile.h) decides it, and xhat as it computes it:
    xhat = fl32(fl32(z - mean) * invstd) in numpy float32 steps; the mask is the sign of fma(t, a, b), t = z (folded: a, b =
    scale, shift) or xhat (a, b = gamma, beta).  In fp64 the product of two fp32 numbers is exact and the sign of a sum
    survives its rounding, so `t * a + b > 0` in fp64 is the sign of the fp32 fma."""
    zn, f32, f64 = z.numpy().astype(np.float32), np.float32, np.float64
    xhat = ((zn - mean.numpy().astype(f32)).astype(f32) * invstd.numpy().astype(f32)).astype(f32)
    t = zn if folded else xhat
    on = t.astype(f64) * a.numpy().astype(f64) + b.numpy().astype(f64) > 0
    return torch.from_numpy(on), torch.from_numpy(xhat)


def bn_eval(ref, gamma, beta, mean, var, eps, res, relu):
    """y = act(P * scale + shift (+ res)), scale = gamma / sqrt(var + eps), shift = beta - mean * scale in fp64 from the fp32
    vectors, P the fp64 product (ref).  Bound (n + 16) * 2^-24 * (sum|terms| * |scale| + |mean * scale| + |beta| + |res|):
    the n + 8 of the product, and 8 more for what the epilogue rounds -- scale is var + eps, sqrt, 1 / x and * gamma (at most
    five roundings with a two-step reciprocal), shift is mean * scale and the subtraction (two), then one fma and the
    residual add; each acts on a quantity no larger than the sum of magnitudes it multiplies.
    -> dict(out = the activation of `pre`, pre, bound).  Under ReLU the bound applies before the clamp (judge_eval)."""
    g, b, m, v = gamma.double(), beta.double(), mean.double(), var.double()
    scale = g / torch.sqrt(v + float(np.float32(eps)))
    shift = b - m * scale
    pre = ref["out"] * scale + shift
    mag = ref["out_abs"] * scale.abs() + (m * scale).abs() + b.abs()
    if res is not None:
        pre, mag = pre + res.double(), mag + res.double().abs()
    return {"out": torch.relu(pre) if relu else pre, "pre": pre, "bound": (ref["out_n"] + 16) * U * mag}


# ==== inputs =============================================================================================================
def _nextafter(v, up):
    return torch.from_numpy(np.nextafter(v.numpy().astype(np.float32), np.float32(np.inf if up else -np.inf)))


def _plant_mask_edges(z, a, b, t_of, zero_at):
    """Elements where the mask expression is exactly 0 (must be masked) and one ulp either side, in channels 0-3, rows 0-2
    and 64-66; channel 4: b = -fl32(t * a) at a row where t * a is not representable and lies above its rounding, so the
    fused expression is a positive rounding residual while fl32(t * a) + b is exactly 0."""
    R, C = z.shape
    if C < 8:
        return
    b[:4] = 0.0
    for base in (0, 64):
        for i, how in enumerate(("eq", "up", "down")):
            if base + i < R:
                v = zero_at[:4]
                z[base + i, :4] = v if how == "eq" else _nextafter(v, how == "up")
    for r in range(3, R):
        if r in (64, 65, 66):
            continue
        t = float(t_of(z[r:r + 1])[0, 4])
        p = float(np.float32(np.float32(t) * np.float32(a[4])))
        if t * float(a[4]) - p > 0:          # exact in fp64
            b[4] = -p
            return


def inputs(c):
    """seeded unit-scale fp32 operands of a case (CPU), weights scaled by K^-1/2; every image and row differs"""
    key = repr((c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s)).encode()
    g = torch.Generator().manual_seed(40000 + zlib.crc32(key) % 100000)
    Ri, Ro = rows_in(c), rows_out(c)
    I = {"x": torch.randn(Ri, c.Cin, generator=g), "dy": torch.randn(Ro, c.Cout, generator=g)}
    if c.op in ("f1", "d1", "w1"):
        I["w"] = torch.randn(c.Cout, c.Cin, generator=g) * (c.Cout if c.op == "d1" else c.Cin) ** -0.5
    else:
        I["w"] = torch.randn(c.Cout, 9, c.Cin, generator=g) * (9 * (c.Cin if c.op == "f3" else c.Cout)) ** -0.5
    I["ss"] = torch.stack([1 + 0.5 * torch.randn(c.Cin, generator=g), 0.2 * torch.randn(c.Cin, generator=g)], 1).contiguous()
    I["shift"] = 0.1 * torch.randn(c.Cout, generator=g)
    I["dx0"] = torch.randn(Ri, c.Cin, generator=g)
    # mask epilogue (channel = Cin of the d input)
    I["z"] = torch.randn(Ri, c.Cin, generator=g)
    I["mean"] = 0.1 * torch.randn(c.Cin, generator=g)
    I["invstd"] = 1 + 0.2 * torch.rand(c.Cin, generator=g)
    I["gamma"] = 1 + 0.3 * torch.randn(c.Cin, generator=g)
    I["beta"] = 0.2 * torch.randn(c.Cin, generator=g)
    if c.epi == 2:
        if "f" in c.var:
            ss = I["ss"]
            if c.Cin >= 8:
                ss[:4, 0] = torch.tensor([2.0, -2.0, 4.0, 0.5])
                v = torch.tensor([0.25, 0.35, 0.45, 0.55])
                sc, sh = ss[:, 0].clone(), ss[:, 1].clone()
                _plant_mask_edges(I["z"], sc, sh, lambda zz: zz, torch.cat([v, torch.zeros(c.Cin - 4)]))
                sh[:4] = -(sc[:4] * v)           # exact: powers of two
                ss[:, 1] = sh
        else:
            _plant_mask_edges(I["z"], I["gamma"], I["beta"],
                              lambda zz: bn_mask(zz, I["mean"], I["invstd"], I["gamma"], I["beta"], False)[1], I["mean"].clone())
    # eval BatchNorm epilogue (channel = Cout)
    I["bn_gamma"] = 1 + 0.3 * torch.randn(c.Cout, generator=g)
    I["bn_beta"] = 0.2 * torch.randn(c.Cout, generator=g)
    I["bn_mean"] = 0.1 * torch.randn(c.Cout, generator=g)
    I["bn_var"] = 0.5 + torch.rand(c.Cout, generator=g)
    I["res"] = torch.randn(Ro, c.Cout, generator=g)
    return I


BN_EPS = 1e-5


# ==== the reference of a case ============================================================================================
def tables(c):
    """the index tables of a case: dict(rows=, idx=)"""
    if c.op in ("f1", "w1"):
        return {"rows": gather_rows(c.N, c.Hi, c.Wi, c.s) if c.s > 1 else None}
    if c.op in ("f3", "w3", "h3"):
        return {"idx": fwd_taps(c.N, c.Hi, c.Wi, c.s)}
    if c.op in ("d3", "s3"):
        return {"idx": dgrad_taps(c.N, c.Hi, c.Wi, c.s)}
    return {}


def reference(c, I, dt=torch.float64, tab=None):
    """the product of a case in dtype dt (fp64: the reference) -> out / out_abs / out_n, n + 1 with a prologue (its fma)"""
    tab = tables(c) if tab is None else tab
    x, dy, w = I["x"].to(dt), I["dy"].to(dt), I["w"].to(dt)
    if c.pro:
        x = prologue(x, I["ss"].to(dt))
    if c.op == "f1":
        r = conv1x1_fwd(x, w, tab["rows"])
    elif c.op == "d1":
        r = conv1x1_dgrad(dy, w, 1.0 if "b" in c.var else 0.0, I["dx0"].to(dt))
    elif c.op == "w1":
        r = conv1x1_wgrad(dy, x, tab["rows"])
    elif c.op == "f3":
        r = conv3_fwd(x, w, tab["idx"])
    elif c.op in ("d3", "s3"):
        r = conv3_dgrad(dy, w, tab["idx"])
    else:
        r = conv3_wgrad(dy, x, tab["idx"], per_tap=c.op == "h3")
    if c.pro:
        r["out_n"] = r["out_n"] + 1
    return r


def mask_of(c, I):
    """(mask, xhat) of an epi = 2 case"""
    if "f" in c.var:
        return bn_mask(I["z"], I["mean"], I["invstd"], I["ss"][:, 0], I["ss"][:, 1], True)
    return bn_mask(I["z"], I["mean"], I["invstd"], I["gamma"], I["beta"], False)


# ==== judging a case =====================================================================================================
def judge(c, I, out, part, kernel, ok, tab=None):
    """`out` [rows][cols] and `part` [2][C][row_tiles] (None without partials) as the kernel -- or any other evaluation --
    stored them (fp32), against the fp64 reference.  ok(kernel, name, got, want, bound, kind) is the judge
    (kernel_harness._bound_ok).  No element is excluded."""
    ref = reference(c, I, tab=tab)
    if c.epi == 3:
        e = bn_eval(ref, I["bn_gamma"], I["bn_beta"], I["bn_mean"], I["bn_var"], BN_EPS, I["res"] if "r" in c.var else None,
                    "l" in c.var)
        ok(kernel, "y", out, e["out"], e["bound"], "eval")
        if "l" in c.var:      # below zero by more than the bound: the clamp must have produced 0 itself
            assert bool((out[e["pre"] < -e["bound"]] == 0).all()), "%s: ReLU left a negative element's value" % kernel
        return
    bound = bound_of(ref)
    if c.epi == 2:
        on, xhat = mask_of(c, I)
        zero = torch.zeros((), dtype=torch.float64)
        ok(kernel, "g", out, torch.where(on, ref["out"], zero), torch.where(on, bound, zero), "sum")
        assert bool((out.contiguous().view(torch.int32)[~on] == 0).all()), "%s: a masked element is not +0.0" % kernel
        s = mask_stats_ref(out, xhat)
        ok(kernel, "sums", part, s["out"], bound_of(s), "sum")
        return
    ok(kernel, {"f": "y", "d": "dx", "s": "dx", "w": "dw", "h": "dw"}[c.op[0]], out, ref["out"], bound, "sum")
    if c.epi == 1:
        s = stats_ref(out, I["shift"] if "s" in c.var else None)
        ok(kernel, "stats", part, s["out"], bound_of(s), "sum")


# ==== the case tables ====================================================================================================
def _f1_cases():
    rows = []
    shapes = [(65, 16, 4), (129, 20, 68), (200, 144, 132), (65, 20, 132), (129, 144, 4), (200, 16, 68), (65, 144, 68),
              (129, 16, 132), (200, 20, 4)]
    k = 0
    for (R, Cin, Cout) in shapes:
        for mi in (1, 2, 4):
            for split in ((1,) if Cin == 16 else (1, 2, 3)):
                k += 1
                rows.append(case("f1", R, 1, 1, Cin, Cout, pro=1, epi=1, var="s" if k % 2 else "", mi=mi, split=split))
                if split > 1 and k % 2:       # the reduce launch + cstats_kernel<1>
                    rows.append(case("f1", R, 1, 1, Cin, Cout, pro=1, epi=1, var="" if k % 4 == 1 else "s", mi=mi, split=split,
                                     opts={"cgemm_combine": 0}))
    rows += [
        case("f1", 129, 1, 1, 144, 4, pro=1, epi=1, var="s"),                       # the policy's own pick of the 128 x 64 tile
        case("f1", 200, 1, 1, 20, 4, pro=1, epi=1),
        case("f1", 200, 1, 1, 144, 132, pro=1, epi=1, var="s", split=9),             # deeper than cgemm_combine_max
        case("f1", 129, 1, 1, 144, 4, pro=1, epi=1, split=9, mi=1),
        case("f1", 129, 1, 1, 144, 68, pro=1, epi=1, var="s", split=2, ws=1, opts={"cgemm_combine": 2}),
        case("f1", 129, 1, 1, 20, 68, pro=1, epi=0, mi=1), case("f1", 200, 1, 1, 144, 132, pro=1, epi=0, mi=2, split=2),
        case("f1", 129, 1, 1, 144, 4, pro=1, epi=0, mi=4),
        case("f1", 65, 1, 1, 20, 68, epi=1, var="s", mi=1), case("f1", 200, 1, 1, 144, 132, epi=1, mi=2, split=3),
        case("f1", 129, 1, 1, 16, 4, epi=1, var="s", mi=4), case("f1", 129, 1, 1, 144, 68, ws=0),
        case("f1", 129, 1, 1, 20, 68, pro=1, epi=1, var="sg", split=2), case("f1", 65, 1, 1, 144, 132, var="g", mi=2),
    ]
    # strided gather: N = 3, 7 x 5 -> 4 x 3, 36 rows
    G = dict(N=3, Hi=7, Wi=5, s=2)
    rows += [case("f1", Cin=16, Cout=68, **G), case("f1", Cin=144, Cout=132, split=2, **G)]
    for mi in (1, 2, 4):
        rows += [case("f1", Cin=20, Cout=68, pro=1, epi=1, var="s", mi=mi, **G), case("f1", Cin=144, Cout=4, epi=1, mi=mi, **G)]
    rows += [case("f1", Cin=144, Cout=68, pro=1, epi=1, split=3, **G), case("f1", Cin=16, Cout=16, pro=1, **G),
             case("f1", Cin=144, Cout=68, pro=1, epi=1, var="s", split=2, opts={"cgemm_combine": 0}, **G)]
    # the _bn_eval form: plain and gathered, residual / ReLU, split (in-launch combine only)
    for i, (R, Cin, Cout) in enumerate([(65, 16, 16), (129, 144, 64), (200, 32, 144)]):
        for j, var in enumerate(("", "r", "l", "rl")):
            rows.append(case("f1", R, 1, 1, Cin, Cout, epi=3, var=var, mi=(0, 1, 2, 4)[(i + j) % 4],
                             split=(1, 2, 3)[j % 3] if Cin > 16 else 1))
    rows += [case("f1", Cin=16, Cout=16, epi=3, var="rl", **G), case("f1", Cin=144, Cout=64, epi=3, var="r", split=2, **G),
             case("f1", Cin=32, Cout=144, epi=3, var="l", mi=1, **G)]
    return rows


def _d1_cases():
    rows = []
    k = 0
    for (R, Cin, Cout) in [(65, 16, 16), (129, 68, 144), (65, 68, 16), (129, 16, 144)]:
        for fold in ("", "f"):
            for split in ((1,) if Cout == 16 else (1, 2)):
                k += 1
                mi = (1, 2, 4, 0)[k % 4]
                rows.append(case("d1", R, 1, 1, Cin, Cout, epi=2, var=fold, mi=mi, split=split))
                if split > 1:
                    rows.append(case("d1", R, 1, 1, Cin, Cout, epi=2, var=fold, mi=mi, split=split, opts={"cgemm_combine": 0}))
            rows.append(case("d1", R, 1, 1, Cin, Cout, epi=2, var=fold + "t"))        # cstats_kernel<2> reading C back
        rows.append(case("d1", R, 1, 1, Cin, Cout, var="b", split=1 if Cout == 16 else 2))
        rows.append(case("d1", R, 1, 1, Cin, Cout, var="bt"))
    rows += [case("d1", 129, 1, 1, 16, 144, epi=2, mi=4), case("d1", 129, 1, 1, 16, 144, epi=2, var="f", mi=4, split=2),
             case("d1", 129, 1, 1, 68, 144, epi=2, mi=1, split=2), case("d1", 129, 1, 1, 68, 144, epi=2, var="f", mi=2),
             case("d1", 129, 1, 1, 68, 144, epi=2, var="g", split=2), case("d1", 65, 1, 1, 16, 16, var="g"),
             case("d1", 129, 1, 1, 68, 144, epi=2, split=9), case("d1", 129, 1, 1, 68, 144, epi=2, split=2, opts={"cgemm_combine": 2})]
    return rows


def _w1_cases():
    rows = []
    k = 0
    for R in (36, 100, 257):
        for (Cout, Cin) in ((4, 16), (68, 132), (4, 132), (68, 16)):
            k += 1
            split = 1 if R == 36 or k % 2 else 2
            rows.append(case("w1", R, 1, 1, Cin, Cout, pro=0, split=split))
            rows.append(case("w1", R, 1, 1, Cin, Cout, pro=2, split=3 - split if R > 36 else 1, mi=(1, 2)[k % 2]))
    rows += [case("w1", 257, 1, 1, 132, 68, pro=2), case("w1", 257, 1, 1, 16, 4, ws=0),
             case("w1", 100, 1, 1, 132, 68, pro=2, var="g", split=2),
             case("w1", 257, 1, 1, 132, 68, split=2, opts={"cgemm_combine": 0})]
    G = dict(N=3, Hi=7, Wi=5, s=2)
    rows += [case("w1", Cin=16, Cout=68, **G), case("w1", Cin=132, Cout=4, pro=2, **G), case("w1", Cin=132, Cout=68, pro=2, split=2, **G),
             case("w1", Cin=16, Cout=4, split=2, **G)]
    return rows


C3_GEO = [(1, 1, 1, 16, 16, 1), (2, 3, 5, 16, 16, 1), (2, 5, 4, 32, 80, 2), (3, 7, 7, 16, 64, 1)]


def _f3_cases():
    rows = []
    for i, (N, Hi, Wi, Cin, Cout, s) in enumerate(C3_GEO):
        geo = dict(N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, s=s)
        for epi in (0, 1):
            var = "s" if epi and i % 2 else ""
            rows += [case("f3", epi=epi, var=var, ws=0, **geo), case("f3", epi=epi, var=var, **geo)]
            rows += [case("f3", epi=epi, var=var, mi=mi, ws=(mi + i) % 2, **geo) for mi in (1, 2, 4)]
        rows.append(case("f3", epi=1, var="s", opts={"cgemm_combine": 0}, **geo))
        rows.append(case("f3", opts={"cgemm_combine": 0}, **geo))                      # creduce_kernel<true> behind a split 3x3
        for j, var in enumerate(("", "r", "l", "rl")):
            rows.append(case("f3", epi=3, var=var, ws=j % 2, mi=(0, 1, 2, 4)[(i + j) % 4], **geo))
        rows.append(case("f3", epi=3, var="rl", **geo))
    return rows


def _d3_cases():
    rows = []
    for i, (N, Hi, Wi, Cin, Cout, s) in enumerate(C3_GEO):
        geo = dict(N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout)      # stride 1 on the same maps
        rows += [case("d3", ws=0, **geo), case("d3", **geo), case("d3", mi=1, **geo), case("d3", mi=4, ws=i % 2, **geo)]
        for fold in ("", "f"):
            rows += [case("d3", epi=2, var=fold, ws=0, **geo), case("d3", epi=2, var=fold, **geo),
                     case("d3", epi=2, var=fold, mi=(1, 4)[i % 2], ws=(i + 1) % 2, **geo)]
        rows.append(case("d3", epi=2, opts={"cgemm_combine": 0}, **geo))
        rows.append(case("d3", epi=2, var="f", opts={"cgemm_combine": 2}, **geo))
    return rows


def _s3_cases():
    rows = []
    for (N, Hi, Wi, Cin, Cout) in [(1, 2, 2, 32, 16), (2, 4, 6, 16, 16), (3, 8, 4, 16, 80), (2, 16, 16, 16, 16)]:
        geo = dict(N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, s=2)
        rows += [case("s3", **geo), case("s3", ws=0, opts={"cgemm_mi": 2}, **geo)]
    return rows


def _w3_cases():
    return [case("w3", 2, 3, 5, 128, 16, s=1, split=-1, ws=0), case("w3", 2, 3, 5, 128, 16, s=1, split=-1),
            case("w3", 2, 5, 4, 128, 32, s=2, ws=0), case("w3", 2, 5, 4, 128, 32, s=2),
            case("w3", 2, 12, 12, 128, 16, s=1, split=-1),                            # 288 rows: the policy splits K in two
            case("w3", 2, 12, 12, 128, 16, s=1, split=-1, opts={"cgemm_combine": 0}),
            case("w3", 2, 5, 4, 128, 80, s=2, opts={"cgemm_mi": 1})]


def _h3_cases():
    rows = []
    chans = [(32, 64), (64, 32), (96, 32), (32, 96), (64, 96)]
    for i, (N, H, W) in enumerate([(1, 1, 3), (1, 2, 8), (1, 5, 1), (2, 3, 16), (2, 2, 32), (3, 4, 12), (2, 3, 20), (4, 8, 16),
                                   (2, 9, 20)]):
        C, Co = chans[i % len(chans)]
        legal = [0, 1] + {(4, 8, 16): [2], (2, 9, 20): [2, 3]}.get((N, H, W), [])
        for ksl in legal:
            rows.append(case("h3", N, H, W, C, Co, split=ksl, ws=1 if ksl != 1 else 0))
    rows.append(case("h3", 2, 9, 20, 96, 64, split=3))
    return rows


CASES = list({case_id(c): c for c in _f1_cases() + _d1_cases() + _w1_cases() + _f3_cases() + _d3_cases() + _s3_cases() +
              _w3_cases() + _h3_cases()}.values())       # a round-robin pairing may name a row twice
