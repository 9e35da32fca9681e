"""fp64 references, cases, fp32 CPU yardsticks and judges of the tagger loss family on the logits (csrc/taghead.hip:
scnattn_tagloss_fwd / _bwd; include/scnattn.h: "Tagger losses for rare tags"), shared by tests/test_tagloss_refs.py (CPU) and
tests/test_gpu_tagloss_kernels.py / test_gpu_tagloss_step.py (the kernels, the head).  The references are index arithmetic on
the header's formulas, not torch's loss ops.

    sp(x)  = max(x, 0) + log1p(exp(-|x|));  p = exp(-sp(-z));  q = 1 - p = exp(-sp(z))
    term   = t w_s Lpos + (1 - t) Lneg
    Lpos   = exp(-gp sp(z)) sp(-z)
    Lneg   = exp(-gn sp(-z)) sp(z)                                 m = 0
    Lneg   = p_m^gn (-log1p(-p_m)),  p_m = max(p - m, 0), 0^0 = 1  m > 0
    dLpos  = -exp(-gp sp(z)) (gp p sp(-z) + q)
    dLneg  = exp(-gn sp(-z)) (gn q sp(z) + p)                      m = 0
    dLneg  = [p > m] (gn p_m^(gn-1) (-log1p(-p_m)) + p_m^gn / (1 - p_m)) p q
    loss   = sum(term) / (B S);  dz = g / (B S) (t w_s dLpos + (1 - t) dLneg)

Bounds (u = 2^-24).  Every value sits behind a chain of expf / log1pf / logf whose condition depends on the setting (a margin
puts p - m behind a cancellation), so the per-element allowance is measured, not fixed: per case the worst element error of
the fp32 CPU evaluation of the SAME expressions (cpu32_tagloss_*) against fp64, relative to |t w L+| + |(1-t) L-| (its
derivative for dz: the two parts have opposite signs), is the yardstick, and a kernel gets 4 x that -- the convention
taghead_refs.judge_probs uses for the sigmoid.
    probs, agree   the bits scnattn_bce_fwd writes (the GPU test compares the two calls)
    row sum        (S + 8) u sum|parts| + 4 yard sum|parts| against the fp64 sum of the fp64 terms at the given z
    loss           (B + 8) u sum|row| / (B S) against the fp64 mean of the stored rows (taghead_refs.judge_loss)
    dz             4 yard |g| / (B S) (|t w dL+| + |(1-t) dL-|); with m > 0 an element with |p - m| <= 2^-20 (fp64 p) is not
                   judged (the gradient jumps there for gn = 0), at most 1 % of a case, asserted
fp32 carries no relative precision below its smallest normal number 2^-126 (at z = -120 the fp64 p is 8e-53, the fp32 p is 0),
so every element's scale |t w L+| + |(1-t) L-| (and its derivative's) gets FLOOR = 2^-100 added, in the yardstick and in the
bound alike: a part below that is judged absolutely, to 4 yard 2^-100.
gp, gn and m reach the references as the fp32 values the kernel is handed."""
import torch

import taghead_refs as T
from kernel_harness import U, _bound_ok, _note

F64 = torch.float64
SHAPES = ((1, 1), (3, 37), (2, 1001), (2, 1028), (32, 1000))                       # (B, S)
# (gamma_pos, gamma_neg, margin, with weights)
SETTINGS = ((0.0, 0.0, 0.0, True), (2.0, 2.0, 0.0, False), (0.0, 4.0, 0.05, False), (1.0, 4.0, 0.05, True),
            (0.0, 0.0, 0.05, False), (0.5, 1.5, 0.0, False))
GUARD = 2.0 ** -20
FLOOR = 2.0 ** -100
G = 0.37                    # d/d loss handed to the backward


def setting_id(s):
    return "gp%g_gn%g_m%g_%s" % (s[0], s[1], s[2], "w" if s[3] else "now")


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- cases --------------------------------------------------------------------------------------------------------------
def gen(B, S, weights, seed=0):
    """taghead_refs.gen_bce's logits and targets with its planted row 0 (z = +-120, +-30 under t in {0, 1}, z = 0, a fractional
    t) and, with `weights`, w in [1, 10] with w = 0 and w = 99 planted under t = 1: z, t, w or None, planted"""
    z, t, planted = T.gen_bce(B, S, seed)
    if planted:     # gen_bce plants -30 only; +30: p rounds to 1 in fp32 while q = 9.4e-14 still carries the gradient
        planted = dict(planted)
        for name, s, tv in (("big_t0", 33, 0.0), ("big_t1", 35, 1.0)):
            z[0, s], t[0, s] = 30.0, tv
            planted[name] = s
    if not weights:
        return z, t, None, planted
    g = torch.Generator().manual_seed(3000 * seed + B * 31 + S)
    w = (1.0 + 9.0 * torch.rand(S, generator=g)).float()
    if planted:
        planted = dict(planted)
        for name, src, val in (("w99_sat", "sat0_t1", 99.0), ("w0_sat", "sat1_t1", 0.0), ("w99_half", "half_t1a", 99.0),
                               ("w0_tiny", "tiny_t1", 0.0), ("w0_half", "half_t1b", 0.0)):
            w[planted[src]] = val
            planted[name] = planted[src]
    else:
        w[0] = 99.0 if float(t[0, 0]) >= 0.5 else 0.0
    return z, t, w, planted


# ---- fp64 references ----------------------------------------------------------------------------------------------------
def sp(x):
    return x.clamp_min(0.0) + torch.log1p(torch.exp(-x.abs()))


def _w64(w, S):
    return torch.ones(S, dtype=F64) if w is None else w.to(F64)


def parts_ref(z, t, w, gp, gn, m):
    """(t w Lpos, (1 - t) Lneg) in fp64"""
    z, t, gp, gn, m = z.to(F64), t.to(F64), f32(gp), f32(gn), f32(m)
    spz, spn = sp(z), sp(-z)
    lpos = torch.exp(-gp * spz) * spn
    if m == 0.0:
        lneg = torch.exp(-gn * spn) * spz
    else:
        pm = (torch.exp(-spn) - m).clamp_min(0.0)
        lneg = (torch.ones_like(pm) if gn == 0.0 else pm ** gn) * -torch.log1p(-pm)
    return t * _w64(w, z.shape[1]) * lpos, (1.0 - t) * lneg


def grad_parts_ref(z, t, w, gp, gn, m):
    """(t w dLpos/dz, (1 - t) dLneg/dz) in fp64, and the mask of the elements inside the guard band of the margin"""
    z, t, gp, gn, m = z.to(F64), t.to(F64), f32(gp), f32(gn), f32(m)
    spz, spn = sp(z), sp(-z)
    p, q = torch.exp(-spn), torch.exp(-spz)
    dpos = -torch.exp(-gp * spz) * (gp * p * spn + q)
    guard = torch.zeros_like(z, dtype=torch.bool)
    if m == 0.0:
        dneg = torch.exp(-gn * spn) * (gn * q * spz + p)
    else:
        on = p > m
        pm = torch.where(on, p - m, torch.full_like(p, 0.5))            # any value off the mask: it is discarded
        nl = -torch.log1p(-pm)
        a = torch.zeros_like(pm) if gn == 0.0 else gn * pm ** (gn - 1.0) * nl
        pw = torch.ones_like(pm) if gn == 0.0 else pm ** gn
        dneg = torch.where(on, (a + pw / (1.0 - pm)) * p * q, torch.zeros_like(p))
        guard = (p - m).abs() <= GUARD
    return t * _w64(w, z.shape[1]) * dpos, (1.0 - t) * dneg, guard


def fwd_ref(z, t, w, gp, gn, m):
    a, b = parts_ref(z, t, w, gp, gn, m)
    terms = a + b
    B, S = terms.shape
    rows, rows_abs = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
    for s in range(S):
        rows += terms[:, s]
        rows_abs += a[:, s].abs() + b[:, s].abs()
    return dict(terms=terms, scale=a.abs() + b.abs() + FLOOR, rows=rows, rows_abs=rows_abs, loss=rows.sum() / (B * S))


def bwd_ref(z, t, w, gp, gn, m, g):
    a, b, guard = grad_parts_ref(z, t, w, gp, gn, m)
    k = float(g) / z.numel()
    return dict(dz=k * (a + b), scale=abs(k) * (a.abs() + b.abs() + FLOOR), guard=guard)


def head_ref(x, ks, W, b, t, w, gp, gn, m):
    """taghead_refs.head_ref with the new term: x [B, HW, C] -> probs, loss, agree, z, dx, dW, db in fp64"""
    x, W, b = x.to(F64), W.to(F64), b.to(F64)
    B, HW, C = x.shape
    xd = T.pool_fwd_ref(x, ks)["pooled"]
    z = torch.zeros(B, W.shape[0], dtype=F64)
    for c in range(C):
        z += xd[:, c:c + 1] * W[:, c].unsqueeze(0)
    z += b
    p = T.sigmoid_ref(z)
    f = fwd_ref(z, t, w, gp, gn, m)
    dz = bwd_ref(z, t, w, gp, gn, m, 1.0)["dz"]
    dW = torch.zeros_like(W)
    dxd = torch.zeros_like(xd)
    for i in range(B):
        dW += dz[i].unsqueeze(1) * xd[i].unsqueeze(0)
        dxd[i] = (dz[i].unsqueeze(1) * W).sum(0)
    agree = int(((p >= 0.5) == (t.to(F64) >= 0.5)).sum())
    return dict(z=z, probs=p, loss=f["loss"], agree=agree, dx=T.pool_bwd_ref(dxd, ks, HW), dW=dW, db=dz.sum(0))


# ---- torch's CPU fp32 evaluation of the kernel's expressions -----------------------------------------------------------
def _parts32(z):
    z = z.float()
    e = torch.exp(-z.abs())
    l, r = torch.log1p(e), 1.0 / (1.0 + e)
    pos = z >= 0
    return z.clamp_min(0.0) + l, (-z).clamp_min(0.0) + l, torch.where(pos, r, e * r), torch.where(pos, e * r, r)


def _w32(w, S):
    return torch.ones(S) if w is None else w.float()


def cpu32_tagloss_terms(z, t, w, gp, gn, m):
    """the element terms in torch CPU float32 and the probabilities 1 / (1 + exp(-z))"""
    spz, spn, _, _ = _parts32(z)
    t = t.float()
    p = 1.0 / (1.0 + torch.exp(-z.float()))
    lp, ln = spn, spz
    if m > 0 or gp != 0 or gn != 0:
        lp = lp * torch.exp(-gp * spz)
    if m > 0:
        pm = (p - m).clamp_min(0.0)
        safe = pm.clamp_min(1e-30)
        pw = torch.ones_like(pm) if gn == 0 else torch.where(pm > 0, torch.exp((gn - 1.0) * torch.log(safe)) * pm, torch.zeros_like(pm))
        ln = pw * -torch.log1p(-pm)
    elif gp != 0 or gn != 0:
        ln = ln * torch.exp(-gn * spn)
    return t * _w32(w, z.shape[1]) * lp + (1.0 - t) * ln, p


def cpu32_tagloss_fwd(z, t, w, gp, gn, m):
    """p, row sums, loss, agreement count"""
    terms, p = cpu32_tagloss_terms(z, t, w, gp, gn, m)
    rows = terms.sum(dim=1)
    return p, rows, rows.sum() / terms.numel(), ((p >= 0.5) == (t >= 0.5)).float().sum()


def cpu32_tagloss_bwd(z, t, w, gp, gn, m, g):
    spz, spn, p, q = _parts32(z)
    t = t.float()
    dp, dn = -q, p
    if m > 0 or gp != 0 or gn != 0:
        dp = -torch.exp(-gp * spz) * (gp * p * spn + q)
    if m > 0:
        ps = 1.0 / (1.0 + torch.exp(-z.float()))
        pm = ps - m
        on = pm > 0
        pm = torch.where(on, pm, torch.full_like(pm, 0.5))
        pw1 = torch.zeros_like(pm) if gn == 0 else torch.exp((gn - 1.0) * torch.log(pm))
        pw = torch.ones_like(pm) if gn == 0 else pw1 * pm
        dn = torch.where(on, (gn * pw1 * -torch.log1p(-pm) + pw / (1.0 - pm)) * ps * q, torch.zeros_like(pm))
    elif gp != 0 or gn != 0:
        dn = torch.exp(-gn * spn) * (gn * q * spz + p)
    scale = torch.tensor(g, dtype=torch.float32) / torch.tensor(float(z.numel()), dtype=torch.float32)
    return scale * (t * _w32(w, z.shape[1]) * dp + (1.0 - t) * dn)


# ---- yardsticks ---------------------------------------------------------------------------------------------------------
def _worst_rel(err, scale, skip=None):
    """worst err / scale over the elements with a scale (the others must be exact and are judged so, not measured)"""
    ok = scale > 0
    if skip is not None:
        ok = ok & ~skip
    return float((err[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


def yard_terms(z, t, w, gp, gn, m):
    r = fwd_ref(z, t, w, gp, gn, m)
    got, _ = cpu32_tagloss_terms(z, t, w, gp, gn, m)
    return _worst_rel((got.to(F64) - r["terms"]).abs(), r["scale"])


def yard_dz(z, t, w, gp, gn, m, g):
    r = bwd_ref(z, t, w, gp, gn, m, g)
    got = cpu32_tagloss_bwd(z, t, w, gp, gn, m, g)
    return _worst_rel((got.to(F64) - r["dz"]).abs(), r["scale"], r["guard"])


# ---- judges -------------------------------------------------------------------------------------------------------------
MEASURED = []       # (kernel, result, case, yardstick, worst kernel error in the yardstick's measure): the GPU test's report


def judge_rows(kernel, rows, z, t, w, gp, gn, m, case=""):
    r = fwd_ref(z, t, w, gp, gn, m)
    yard = yard_terms(z, t, w, gp, gn, m)
    S = z.shape[1]
    rel = _worst_rel((rows.to(F64) - r["rows"]).abs(), r["rows_abs"])
    print("%s rows %s: CPU fp32 worst element error %.3e, worst row error / sum|parts| %.3e" % (kernel, case, yard, rel))
    MEASURED.append((kernel, "rows", case, yard, rel))
    _bound_ok(kernel, "rows", rows, r["rows"], ((S + 8) * U + 4.0 * yard) * r["rows_abs"], "=((S+8) 2^-24 + 4 yard) sum|parts|")


def judge_loss(kernel, loss, rows, B, S):
    T.judge_loss(kernel, loss, rows, B, S)


def judge_dz(kernel, dz, z, t, w, gp, gn, m, g, planted=None, case=""):
    r = bwd_ref(z, t, w, gp, gn, m, g)
    yard = yard_dz(z, t, w, gp, gn, m, g)
    guard = r["guard"]
    assert int(guard.sum()) <= 0.01 * guard.numel(), "%s: %d of %d elements inside the guard band" % (
        kernel, int(guard.sum()), guard.numel())
    got = dz.to(F64)
    assert not bool(got.isnan().any()), "%s dz: NaN" % kernel
    rel = _worst_rel((got - r["dz"]).abs(), r["scale"], guard)
    print("%s dz %s: CPU fp32 worst element error %.3e, kernel %.3e, %d in the guard band" % (kernel, case, yard, rel,
                                                                                           int(guard.sum())))
    MEASURED.append((kernel, "dz", case, yard, rel))
    keep = (~guard).to(F64)
    _bound_ok(kernel, "dz", got * keep, r["dz"] * keep, 4.0 * yard * r["scale"] * keep, "=4 yard |g|/(B S) (|t w dL+| + |(1-t) dL-|)")
    if planted and m == 0.0:     # nothing is clamped: a saturated logit keeps the gradient of the logits form
        k, s = float(g) / z.numel(), planted["sat0_t1"]
        ws = 1.0 if w is None else float(w[s])
        assert abs(float(dz[0, s]) + ws * k) <= 1e-6 * abs(ws * k), "sat0_t1"
        assert abs(float(dz[0, planted["sat1_t0"]]) - k) <= 1e-6 * abs(k), "sat1_t0"
