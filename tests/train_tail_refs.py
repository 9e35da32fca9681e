"""fp64 references, cases and judges of the tail of the train step: the loss backward (csrc/loss.hip: scnattn_caption_loss_bwd,
and the sm1 of scnattn_caption_loss_fwd), the fused clamp + Adam update (scnattn_clamp_adam), the sequence glue of
csrc/misc.hip (scnattn_gather_rows_tm, _scatter_add_rows_tm, _hidden_to_bm, _hidden_from_bm, _colsum_masked, _reduce_slabs,
_copy2d, _add_bcast_rows), the encoder's pooling (scnattn_pool_permute_fwd / _bwd) and scnattn_f32_to_bf16.  Shared by
tests/test_train_tail_refs.py (CPU: the references against torch's own fp64 ops and autograd, the judges against torch's CPU
fp32 evaluation and against planted defects) and tests/test_gpu_train_tail_kernels.py (the kernels).  The references are index
arithmetic in fp64 on the fp32 inputs, not the torch ops they are held to.

Three tiers (u = 2^-24):

  bit-equal (bound 0)   gather_rows_tm, copy2d, hidden_to_bm / hidden_from_bm (with a mask: ONE fp32 product, which is the
                        fp64 product rounded once), rowmask, every region that must be exactly 0 (d scores of undecoded rows,
                        inactive cells), the dtable row of a token that does not occur, f32_to_bf16 (NaN: any quiet NaN).
  sum                   |got - ref| <= (n + 8) u sum|terms|: any order of n terms and up to 8 more roundings.
                        colsum_masked   n = R + 1 (the rows and beta*out; a masked-out row and, at beta = 0, the old out are
                                        not terms: NaN there must not show)
                        reduce_slabs    n = slabs
                        scatter_add     per vocabulary row, n = its cells + 1 (the old dtable value)
                        pool fwd        per output cell, n = its window; terms x / |window|
                        pool bwd        per pixel, n = the windows that contain it; terms dy / |window|
                        add_bcast_rows  n = 2 (x and scale*v; the product fused into the add or not)
                        sm1             n = T + 1 (the alphas of a pixel and the 1)
                        dalphas         n = 1 (g * (2 alpha_c / (B P)) * sm1: three roundings of one term)
  derived               ce_bwd and clamp_adam, per element, below.

ce_bwd.  want = (exp(x - lse) - onehot) * g / N at the row_lse the kernel is GIVEN (the fp32 rounding of the fp64 log-sum-exp:
the forward kernel is not in the loop).  d = fl(x - lse) carries u|d|, which is a relative error of the probability p; expf
rounded correctly adds u p; the subtraction of the one-hot rounds once, g * (1/N) twice, the last product once: 4u |p - onehot|.
    bound = (1 + CE_SLACK) u |g/N| ((|d| + 1) p + 4 |p - onehot|)            (0 for an undecoded row)
At the target p - 1 cancels and the first term is the whole bound.  Chained behind the forward kernel, the reference takes the
fp64 log-sum-exp and the bound gains |g/N| p |row_lse - lse64|.

clamp_adam.  The hyper-parameters are rounded as scn::clamp_adam passes them (lr, b1, b2, eps, clip, gscale cast to fp32; bc1 =
1 - b1^step and sqrt(1 - b2^step) formed in double from the double b1, b2, then cast).  With gi = clamp(g * gscale):
    m' = b1 m + (1 - b1) gi             4u (|b1 m| + |(1-b1) gi|)          gi, 1 - b1, the product, b1 m: <= 3 per term, + the add
    v' = b2 v + (1 - b2) gi gi          6u (|b2 v| + |(1-b2) gi gi|)       gi twice, 1 - b2, two products: 5, + the add
    p' = p - (lr/bc1) m' / (sqrt(v')/sqrt_bc2 + eps)   against fp64 AT THE STORED m', v' (what the kernel divides):
                                        (1 + ADAM_SLACK) u (6 |update| + |p'|)   lr/bc1, sqrtf, two divisions, + eps, the product: 6
each plus TINY = 4 x 2^-149 for a product that underflows gradually.  A non-finite expectation (a NaN gradient, an infinite one
with clip = 0) must come out as the same infinity or as NaN.

The slacks cover what nothing here derives: the error of the device expf (CE_SLACK), of sqrtf, the divisions and contraction
(ADAM_SLACK).  A constant added to one term cannot do that: the first-order terms are attained (d just above a power of two
rounds by the whole u|d|, p' just below one by the whole u|p'|), so a correctly rounded evaluation already reaches 0.8 to 1.0 of
the derived bound.  Each slack is therefore a whole number of further copies of the derived bound, sized from torch's CPU fp32
evaluation of the same formulas over every case of the GPU test (tests/test_train_tail_refs.py prints the ratios): the smallest
at which that evaluation sits at or below 0.5, which leaves a device function of twice its error inside."""
import math

import torch

from kernel_harness import U, _bound_ok, _note

F64 = torch.float64
BF = torch.bfloat16
NAN = float("nan")
INF = float("inf")
TINY = 4.0 * 2.0 ** -149

CE_SLACK = 1.0          # sized in test_train_tail_refs.py::test_cpu_fp32_passes_every_judge (measured ratios: its docstring)
ADAM_SLACK = 1.0


def f32(x):
    """the fp32 rounding of a Python float, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def _bits(x):
    return x.contiguous().view(torch.int32)


def judge_bits(kernel, name, got, want):
    """bit for bit (a float32 or int32 tensor)"""
    got, want = got.reshape(want.shape), want
    same = _bits(got) == _bits(want) if got.dtype == torch.float32 else got == want
    n = int((~same).sum())
    print("%s %s: %d of %d elements differ in bits" % (kernel, name, n, same.numel()))
    assert n == 0, "%s %s: %d elements differ in bits, first at %d" % (kernel, name, n, int((~same).reshape(-1).nonzero()[0]))
    _note(kernel, name, 0.0, "=bit for bit")


def judge_nonfinite(kernel, name, got, want, bound, kind):
    """_bound_ok on the elements whose expectation is finite; the others must be the same infinity, or NaN for NaN"""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    bound = bound.double().expand(want.shape).reshape(-1) if torch.is_tensor(bound) else torch.full_like(want, bound)
    fin = want.isfinite()
    odd = ~fin
    ok = torch.where(want[odd].isnan(), got[odd].isnan(), got[odd] == want[odd])
    assert bool(ok.all()), "%s %s: %d non-finite expectations not met (first at %d: got %r, want %r)" % (
        kernel, name, int((~ok).sum()), int(odd.nonzero().reshape(-1)[(~ok).nonzero()[0, 0]]),
        float(got[odd][(~ok).nonzero()[0, 0]]), float(want[odd][(~ok).nonzero()[0, 0]]))
    if bool(fin.any()):
        _bound_ok(kernel, name, got[fin], want[fin], bound[fin], kind)


# =========================================================================================================================
# caption_loss_bwd
# =========================================================================================================================
CE_B, CE_T, CE_LENS = 3, 4, (4, 2, 1)
CE_LDT = CE_T + 2
CE_VS = (1, 3, 4, 1023, 1024, 1028, 2051)
CE_PS = (0, 5, 196)
CE_BAD = (-1, "V", 2 ** 32 + 3)
GOUT = 2.5
ALPHA_C = f32(0.7)
CE_KIND = "=%g u |g/N| ((|x-lse| + 1) p + 4 |p - onehot|)" % (1.0 + CE_SLACK)


def ce_cells(lens=CE_LENS, T=CE_T):
    return [(b, t) for b in range(len(lens)) for t in range(min(lens[b], T))]


def gen_ce(V, bad=None, seed=0):
    """scores [B, T, V] with NaN in the undecoded rows, one row whose target dominates (p - 1 cancels) and one whose target is
    rare; targets [B, ldt] int64 at 0, V-1, both sides of the first vector boundary (3, 4) and of the 256 x 4 sweep (1023,
    1024), garbage in the undecoded cells and in [T, ldt); `bad` replaces the label of cell (0, 2)"""
    g = torch.Generator().manual_seed(7000 + 31 * V + seed)
    B, T = CE_B, CE_T
    scores = (torch.randn(B, T, V, generator=g) * 3.0).float()
    want_t = [0, V - 1, 3, 4, 1023, 1024, (V - 1) // 2]
    targets = torch.full((B, CE_LDT), V + 5, dtype=torch.int64)
    for (b, t), tg in zip(ce_cells(), want_t):
        targets[b, t] = min(tg, V - 1)
    if V > 1:
        scores[0, 1, int(targets[0, 1])] += 14.0        # p ~ 1 - 1e-5 at the target
        scores[1, 0, int(targets[1, 0])] -= 9.0         # p ~ 1e-7 at the target
    if bad is not None:
        targets[0, 2] = V if bad == "V" else bad
    for b in range(B):
        scores[b, CE_LENS[b]:, :] = NAN
    return scores, targets


def lse64(scores, lens=CE_LENS):
    """fp64 log-sum-exp of the decoded rows (0 elsewhere), [B, T]"""
    B, T, V = scores.shape
    out = torch.zeros(B, T, dtype=F64)
    for b, t in ce_cells(lens, T):
        x = scores[b, t].double()
        m = x.max()
        out[b, t] = m + torch.log(torch.exp(x - m).sum())
    return out


def ce_fwd_ref(scores, targets, lens=CE_LENS):
    """the packed cross-entropy in fp64: mean over the decoded rows of lse - x[target]"""
    B, T, V = scores.shape
    l = lse64(scores, lens)
    cells = ce_cells(lens, T)
    return sum(l[b, t] - scores[b, t, int(targets[b, t])].double() for b, t in cells) / len(cells)


def ce_bwd_ref(scores, targets, lse, gout=GOUT, lens=CE_LENS, n_rows=None):
    """d scores in fp64 at the given row_lse [B, T]; n_rows: the N of the mean (the planted defect passes B * T)"""
    B, T, V = scores.shape
    cells = ce_cells(lens, T)
    N = len(cells) if n_rows is None else n_rows
    want, p, d, hot = (torch.zeros(B, T, V, dtype=F64) for _ in range(4))
    for b, t in cells:
        d[b, t] = scores[b, t].double() - lse[b, t].double()
        p[b, t] = torch.exp(d[b, t])
        tg = int(targets[b, t])
        if 0 <= tg < V:
            hot[b, t, tg] = 1.0
        want[b, t] = (p[b, t] - hot[b, t]) * gout / N
    return dict(want=want, p=p, d=d, hot=hot, scale=abs(gout) / N)


def ce_bound(r, dlse=None):
    b = (1.0 + CE_SLACK) * U * r["scale"] * ((r["d"].abs() + 1.0) * r["p"] + 4.0 * (r["p"] - r["hot"]).abs())
    if dlse is not None:
        b = b + r["scale"] * r["p"] * dlse.double().unsqueeze(-1)
    return b


def judge_ce_bwd(kernel, got, scores, targets, lse, dlse=None, lens=CE_LENS):
    r = ce_bwd_ref(scores, targets, lse, lens=lens)
    got = got.reshape(r["want"].shape)
    for b in range(len(lens)):
        off = got[b, lens[b]:]
        assert bool((_bits(off) == 0).all()), "%s: d scores of an undecoded row of image %d is not +0.0 everywhere" % (kernel, b)
    _bound_ok(kernel, "dscores", got, r["want"], ce_bound(r, dlse), CE_KIND)


def cpu32_ce_bwd(scores, targets, lse32, gout=GOUT, lens=CE_LENS):
    B, T, V = scores.shape
    cells = ce_cells(lens, T)
    g = torch.tensor(gout, dtype=torch.float32) * (torch.tensor(1.0) / torch.tensor(float(len(cells))))
    out = torch.zeros(B, T, V)
    for b, t in cells:
        hot = torch.zeros(V)
        if 0 <= int(targets[b, t]) < V:
            hot[int(targets[b, t])] = 1.0
        out[b, t] = (torch.exp(scores[b, t] - lse32[b, t]) - hot) * g
    return out


def gen_alphas(P, seed=0):
    """alphas [B, T, P] (every t counts: alphas.sum(dim=1) runs over all T) and an sm1 [B, P] for the backward alone"""
    g = torch.Generator().manual_seed(7100 + P + seed)
    a = torch.rand(CE_B, CE_T, P, generator=g).float() * (2.0 / CE_T)
    sm1 = (torch.randn(CE_B, P, generator=g) * 0.3).float()
    return a, sm1


def alpha_reg_ref(alphas):
    a = alphas.double()
    B, T, P = a.shape
    s, sa = torch.zeros(B, P, dtype=F64), torch.zeros(B, P, dtype=F64)
    for t in range(T):
        s += a[:, t]
        sa += a[:, t].abs()
    return dict(sm1=s - 1.0, sm1_abs=sa + 1.0, sm1_n=T + 1)


def dalphas_ref(sm1, T, gout=GOUT, alpha_c=ALPHA_C):
    B, P = sm1.shape
    row = gout * 2.0 * alpha_c / (B * P) * sm1.double()
    out = torch.empty(B, T, P, dtype=F64)
    for t in range(T):
        out[:, t] = row
    return dict(dalphas=out, dalphas_abs=out.abs(), dalphas_n=1)


def cpu32_dalphas(sm1, T, gout=GOUT, alpha_c=ALPHA_C):
    B, P = sm1.shape
    scale = torch.tensor(2.0 * alpha_c, dtype=torch.float32) / (torch.tensor(float(B)) * torch.tensor(float(P)))
    return ((torch.tensor(gout, dtype=torch.float32) * scale) * sm1).unsqueeze(1).expand(B, T, P).contiguous()


# =========================================================================================================================
# clamp_adam
# =========================================================================================================================
ADAM_NS = (1, 255, 257, 10007, 4096 * 256 + 777)
ADAM_CLIPS = (5.0, 0.0)
ADAM_GSCALES = (1.0, 0.25)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 4e-4, 0.9, 0.999, 1e-8
ADAM_KIND_P = "=%g u (6 |update| + |p'|) at the stored m', v'" % (1.0 + ADAM_SLACK)


def adam_hyper(step, clip, gscale, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS, rounded=True):
    """the scalars of one step; rounded: as scn::clamp_adam hands them to the kernel (bc1, sqrt_bc2 formed in double first)"""
    h = dict(lr=lr, b1=b1, b2=b2, eps=eps, bc1=1.0 - b1 ** step, sbc2=math.sqrt(1.0 - b2 ** step), clip=clip, gs=gscale)
    return {k: f32(v) for k, v in h.items()} if rounded else h


def gen_adam(n, seed=0, zero_state=False):
    """p, g, m, v [n] float32.  g straddles +-5 (the clip) and +-20 (the clip at gscale 0.25) by one ulp and holds +-inf, +-0
    and values whose square underflows (to 0 and to a subnormal), at both ends of the buffer when n >= 64"""
    gen = torch.Generator().manual_seed(9000 + n % 10007 + 17 * seed)
    p = torch.randn(n, generator=gen).float()
    g = (torch.randn(n, generator=gen) * 3.0).float()
    m = torch.zeros(n) if zero_state else (torch.randn(n, generator=gen) * 0.1).float()
    v = torch.zeros(n) if zero_state else (torch.rand(n, generator=gen) * 0.01).float()
    up, dn = lambda x: float(torch.nextafter(torch.tensor(x), torch.tensor(INF))), \
        lambda x: float(torch.nextafter(torch.tensor(x), torch.tensor(-INF)))
    special = [5.0, -5.0, up(5.0), dn(5.0), -up(5.0), 20.0, -20.0, up(20.0), dn(20.0), 7.0, -300.0, INF, -INF, 0.0, -0.0,
               1e-25, -1e-20, 3e-23]
    if n >= 64:
        for k, s in enumerate(special):
            g[1 + 3 * k] = s
            g[n - 2 - 3 * k] = -s
    else:
        g[0] = 7.0
    return p, g, m, v


def adam_ref(p, g, m, v, h):
    """one step in fp64 on the values given: m', v' with their term magnitudes, and p' from those m', v'"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gi = g * h["gs"]
    if h["clip"] > 0:       # comparisons: a NaN gradient stays NaN, as torch's clamp_ keeps it
        c = h["clip"]
        gi = torch.where(gi < -c, torch.full_like(gi, -c), torch.where(gi > c, torch.full_like(gi, c), gi))
    t1, t2 = h["b1"] * m, (1.0 - h["b1"]) * gi
    u1, u2 = h["b2"] * v, (1.0 - h["b2"]) * gi * gi
    r = dict(m=t1 + t2, m_abs=t1.abs() + t2.abs(), v=u1 + u2, v_abs=u1.abs() + u2.abs())
    r.update(adam_p_ref(p, r["m"], r["v"], h))
    return r


def adam_p_ref(p, m2, v2, h):
    upd = (h["lr"] / h["bc1"]) * (m2.double() / (torch.sqrt(v2.double()) / h["sbc2"] + h["eps"]))
    return dict(p=p.double() - upd, upd=upd)


def judge_adam(kernel, got_p, got_m, got_v, p, g, m, v, h):
    r = adam_ref(p, g, m, v, h)
    judge_nonfinite(kernel, "m", got_m, r["m"], 4.0 * U * r["m_abs"] + TINY, "=4u (|b1 m| + |(1-b1) gi|)")
    judge_nonfinite(kernel, "v", got_v, r["v"], 6.0 * U * r["v_abs"] + TINY, "=6u (|b2 v| + |(1-b2) gi gi|)")
    q = adam_p_ref(p, got_m, got_v, h)
    judge_nonfinite(kernel, "p", got_p, q["p"], (1.0 + ADAM_SLACK) * U * (6.0 * q["upd"].abs() + q["p"].abs()) + TINY, ADAM_KIND_P)


def cpu32_adam(p, g, m, v, h, defect=None):
    """torch's CPU fp32 evaluation (every scalar an fp32 tensor); defect: one of the planted ones"""
    t = {k: torch.tensor(x, dtype=torch.float32) for k, x in h.items()}
    one = torch.tensor(1.0)
    gi = g if defect == "clamp_first" else g * t["gs"]
    if h["clip"] > 0:
        gi = torch.clamp(gi, -t["clip"], t["clip"])
    if defect == "clamp_first":
        gi = gi * t["gs"]
    if defect == "nan_to_clip":
        gi = torch.where(gi.isnan(), -t["clip"], gi)
    m2 = t["b1"] * m + (one - t["b1"]) * gi
    v2 = t["b2"] * v + (one - t["b2"]) * gi * gi
    root = torch.sqrt(v2) / (t["sbc2"] * t["sbc2"]) if defect == "sqrt_outside" else torch.sqrt(v2) / t["sbc2"]
    p2 = p - (t["lr"] / t["bc1"]) * (m2 / (root + t["eps"]))
    if defect == "skip_tail":
        k = 4096 * 256
        p2[k:], m2[k:], v2[k:] = p[k:], m[k:], v[k:]
    return p2, m2, v2


# =========================================================================================================================
# embedding: gather_rows_tm / scatter_add_rows_tm
# =========================================================================================================================
GATHER_MS = (1, 255, 256, 257, 513)
GATHER_B, GATHER_T, GATHER_L, GATHER_V = 3, 4, 6, 7
SCAT_B, SCAT_T, SCAT_L, SCAT_V = 48, 39, 41, 12
SCAT_MS = (3, 257)
SCAT_COUNTS = (1025, 1024, 1023)        # cells of the crowded token: the ordered scan, the last sorted list, one below
SCAT_TOKEN, SCAT_ABSENT = 5, 7


def gen_gather(M, seed=0):
    g = torch.Generator().manual_seed(11000 + M + seed)
    B, T, L, V = GATHER_B, GATHER_T, GATHER_L, GATHER_V
    caps = torch.randint(0, V, (B, L), generator=g)
    caps[0, 0], caps[0, 1], caps[1, 0], caps[1, 1] = 0, V - 1, -3, V + 2       # the last two: clamped to rows 0 and V-1
    caps[2, T - 1] = V - 1
    caps[:, T:] = 1 << 40                                                      # never looked up
    return caps, torch.randn(V, M, generator=g).float()


def gather_ref(caps, table, T):
    B, V, M = caps.shape[0], table.shape[0], table.shape[1]
    out = torch.empty(T * B, M, dtype=torch.float32)
    for t in range(T):
        for b in range(B):
            out[t * B + b] = table[min(max(int(caps[b, t]), 0), V - 1)]
    return out


def gen_scatter(M, count, seed=0):
    """caps [B, L], decode lengths, demb [T*B, M] (NaN in the rows of inactive cells and of cells whose token is out of range:
    neither may be read), dtable [V, M] nonzero.  Token 5 fills exactly `count` active cells and every inactive one, token 7
    none; -3 and V+2 sit in active cells."""
    g = torch.Generator().manual_seed(12000 + 7 * M + count + seed)
    B, T, L, V = SCAT_B, SCAT_T, SCAT_L, SCAT_V
    lens = [T] * B
    lens[B - 1], lens[B - 2], lens[B - 3], lens[3] = 1, 20, 5, 38
    caps = torch.full((B, L), SCAT_TOKEN, dtype=torch.int64)
    cells = [(b, t) for b in range(B) for t in range(lens[b])]
    assert len(cells) >= count + 200
    order = torch.randperm(len(cells), generator=g).tolist()
    others = [v for v in range(V) if v not in (SCAT_TOKEN, SCAT_ABSENT)] + [-3, V + 2]
    for k, i in enumerate(order):
        b, t = cells[i]
        if k >= count:
            caps[b, t] = others[(k - count) % len(others)] if k < count + len(others) else \
                others[int(torch.randint(0, len(others), (1,), generator=g))]
    demb = torch.randn(T * B, M, generator=g).float()
    for b in range(B):
        for t in range(T):
            if t >= lens[b] or not 0 <= int(caps[b, t]) < V:
                demb[t * B + b] = NAN
    dtable = torch.randn(V, M, generator=g).float()
    return caps, lens, demb, dtable


def scatter_ref(caps, lens, demb, dtable, T, drop_after=None):
    """fp64 row sums over the active cells in (t, b) order; drop_after: the planted defect (cells past that many are lost)"""
    B, (V, M) = caps.shape[0], dtable.shape
    want, sabs = dtable.double().clone(), dtable.double().abs()
    n = torch.zeros(V, dtype=torch.long)
    for t in range(T):
        for b in range(B):
            v = int(caps[b, t])
            if t < lens[b] and 0 <= v < V:
                n[v] += 1
                if drop_after is None or int(n[v]) <= drop_after:
                    want[v] += demb[t * B + b].double()
                    sabs[v] += demb[t * B + b].double().abs()
    bound = torch.where(n > 0, n + 1 + 8, torch.zeros_like(n)).double().unsqueeze(1) * U * sabs
    return dict(want=want, bound=bound, n=n, present=(n > 0).to(torch.int32))


def judge_scatter(kernel, got, present, caps, lens, demb, dtable, T):
    r = scatter_ref(caps, lens, demb, dtable, T)
    assert int(r["n"][SCAT_ABSENT]) == 0
    _bound_ok(kernel, "dtable", got, r["want"], r["bound"], "=(cells+1+8) u sum|terms| per row; 0 for an absent token")
    if present is not None:
        judge_bits(kernel, "present", present, r["present"])


def cpu32_scatter(caps, lens, demb, dtable, T):
    out = dtable.clone()
    B, V = caps.shape[0], dtable.shape[0]
    for v in range(V):
        rows = [t * B + b for t in range(T) for b in range(B) if t < lens[b] and int(caps[b, t]) == v]
        if rows:
            out[v] += demb[rows].sum(dim=0)
    return out


# =========================================================================================================================
# layout: hidden_to_bm / hidden_from_bm, copy2d, add_bcast_rows, reduce_slabs, colsum_masked
# =========================================================================================================================
HID_B, HID_T, HID_LENS = 3, 4, (4, 2, 1)
HID_DS = (1, 255, 256, 257, 513)
COPY_SHAPES = ((1, 1), (1, 257), (33, 7))
BCAST_B, BCAST_PS, BCAST_ES, BCAST_SCALE = 2, (1, 7), (1, 130), f32(1.0 / 7.0)
SLAB_NS, SLAB_ROWS, SLAB_WS = (1, 2, 16), 3, (1, 259)
COLSUM_RS = (0, 1, 15, 16, 63, 64, 65, 200)
COLSUM_NS = (1, 15, 16, 17, 50)
COLSUM_BETAS = (0.0, 1.5)


def gen_hidden(D, to_bm, seed=0):
    """source and mask with NaN in the rows of inactive cells; to_bm: the source is time-major [T*B, D], the mask [B*T, D]"""
    g = torch.Generator().manual_seed(13000 + D + seed)
    B, T = HID_B, HID_T
    src = torch.randn(T * B, D, generator=g).float()
    mask = ((torch.rand(B * T, D, generator=g) >= 0.5).float() * 2.0)
    mask[0, 0] = 0.0
    for b in range(B):
        for t in range(HID_LENS[b], T):
            src[(t * B + b) if to_bm else (b * T + t)] = NAN
            mask[b * T + t] = NAN
    return src, mask


def hidden_ref(src, mask, to_bm, lens=HID_LENS, T=HID_T):
    """to_bm: out[b*T+t] = src[t*B+b] * mask[b*T+t]; else out[t*B+b] = src[b*T+t] * mask[b*T+t]; 0 for an inactive cell"""
    B, D = len(lens), src.shape[1]
    out = torch.zeros(B * T, D, dtype=torch.float32)
    rowmask = torch.zeros(B * T, dtype=torch.float32)
    for b in range(B):
        for t in range(min(lens[b], T)):
            bm, tm = b * T + t, t * B + b
            s = src[tm if to_bm else bm].double()
            k = 1.0 if mask is None else mask[bm].double()
            out[bm if to_bm else tm] = (s * k).float()
            rowmask[bm] = 1.0
    return out, rowmask


def gen_bcast(P, E, seed=0):
    g = torch.Generator().manual_seed(13500 + 131 * P + E + seed)
    return torch.randn(BCAST_B, P, E, generator=g).float(), torch.randn(BCAST_B, E, generator=g).float()


def gen_slabs(n, W, seed=0):
    g = torch.Generator().manual_seed(13700 + 263 * n + W + seed)
    return torch.randn(n, SLAB_ROWS, W, generator=g).float()


def bcast_ref(x, v, scale=BCAST_SCALE):
    B, P, E = x.shape
    want, sabs = torch.empty(B, P, E, dtype=F64), torch.empty(B, P, E, dtype=F64)
    for p in range(P):
        want[:, p] = x[:, p].double() + scale * v.double()
        sabs[:, p] = x[:, p].double().abs() + (scale * v.double()).abs()
    return dict(x=want, x_abs=sabs, x_n=2)


def slabs_ref(vals):
    n = vals.shape[0]
    s, a = torch.zeros(vals.shape[1:], dtype=F64), torch.zeros(vals.shape[1:], dtype=F64)
    for i in range(n):
        s += vals[i].double()
        a += vals[i].double().abs()
    return dict(out=s, out_abs=a, out_n=n)


def gen_colsum(R, N, seed=0):
    """X [R, N] with NaN and inf in the masked-out rows, rowmask [R] of 0 / 1 / 2 (any nonzero selects), old out [N]"""
    g = torch.Generator().manual_seed(14000 + 53 * R + N + seed)
    X = torch.randn(max(R, 1), N, generator=g).float()
    mask = (torch.rand(max(R, 1), generator=g) >= 0.4).float()
    if R >= 15:
        mask[0], mask[R - 1], mask[7] = 0.0, 0.0, 2.0
    for r in range(max(R, 1)):
        if mask[r] == 0:
            X[r] = NAN if r % 2 == 0 else INF
    return X, mask, torch.randn(N, generator=g).float()


def colsum_ref(X, mask, old, R, beta, multiply=False):
    """multiply: the planted defect (mask as a factor)"""
    N = X.shape[1]
    s, a = torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
    if beta != 0:
        s, a = s + beta * old.double(), a + (beta * old.double()).abs()
    for r in range(R):
        if multiply:
            s = s + X[r].double() * float(mask[r])
        elif float(mask[r]) != 0:
            s, a = s + X[r].double(), a + X[r].double().abs()
    return dict(out=s, out_abs=a, out_n=R + 1)


# =========================================================================================================================
# pool_permute
# =========================================================================================================================
POOL_SIZES = ((8, 8, 14, 14), (7, 7, 14, 14), (16, 16, 14, 14), (14, 14, 14, 14), (9, 7, 14, 14), (8, 8, 3, 5))
POOL_B, POOL_CS = 2, (1, 70, 300)


def pool_window(o, n_in, n_out, floor_hi=False):
    """[floor(o n_in / n_out), ceil((o+1) n_in / n_out)); floor_hi: the planted defect"""
    hi = ((o + 1) * n_in) // n_out if floor_hi else -((-(o + 1) * n_in) // n_out)
    return (o * n_in) // n_out, hi


def gen_pool2d(C, size, seed=0):
    Hin, Win, Ho, Wo = size
    g = torch.Generator().manual_seed(15000 + C + 11 * Hin + Win + 3 * Ho + Wo + seed)
    return torch.randn(POOL_B, C, Hin, Win, generator=g).float(), torch.randn(POOL_B, Ho, Wo, C, generator=g).float()


def pool_fwd_ref(x, Ho, Wo, floor_hi=False):
    """x [B, C, Hin, Win] -> y [B, Ho, Wo, C], with sum|terms| and the per-cell bound"""
    B, C, Hin, Win = x.shape
    xd = x.double()
    y, ya, n = torch.zeros(B, Ho, Wo, C, dtype=F64), torch.zeros(B, Ho, Wo, C, dtype=F64), torch.zeros(Ho, Wo)
    for oh in range(Ho):
        h0, h1 = pool_window(oh, Hin, Ho, floor_hi)
        for ow in range(Wo):
            w0, w1 = pool_window(ow, Win, Wo, floor_hi)
            cnt = max((h1 - h0) * (w1 - w0), 1)
            n[oh, ow] = cnt
            for h in range(h0, h1):
                for w in range(w0, w1):
                    y[:, oh, ow, :] += xd[:, :, h, w] / cnt
                    ya[:, oh, ow, :] += xd[:, :, h, w].abs() / cnt
    return dict(y=y, bound=(n + 8).double().view(1, Ho, Wo, 1) * U * ya)


def pool_bwd_ref(dy, Hin, Win):
    """dy [B, Ho, Wo, C] -> dx [B, C, Hin, Win]"""
    B, Ho, Wo, C = dy.shape
    d = dy.double()
    dx, da, n = torch.zeros(B, C, Hin, Win, dtype=F64), torch.zeros(B, C, Hin, Win, dtype=F64), torch.zeros(Hin, Win)
    for oh in range(Ho):
        h0, h1 = pool_window(oh, Hin, Ho)
        for ow in range(Wo):
            w0, w1 = pool_window(ow, Win, Wo)
            cnt = (h1 - h0) * (w1 - w0)
            n[h0:h1, w0:w1] += 1
            for h in range(h0, h1):
                for w in range(w0, w1):
                    dx[:, :, h, w] += d[:, oh, ow, :] / cnt
                    da[:, :, h, w] += d[:, oh, ow, :].abs() / cnt
    return dict(dx=dx, bound=(n + 8).double().view(1, 1, Hin, Win) * U * da)


POOL_KIND = "=(n+8) u sum|terms|, n = the window (fwd) / the windows over the pixel (bwd)"


def judge_pool_fwd(kernel, got, x, Ho, Wo):
    r = pool_fwd_ref(x, Ho, Wo)
    _bound_ok(kernel, "y", got, r["y"], r["bound"], POOL_KIND)


def judge_pool_bwd(kernel, got, dy, Hin, Win):
    r = pool_bwd_ref(dy, Hin, Win)
    _bound_ok(kernel, "dx", got, r["dx"], r["bound"], POOL_KIND)


# =========================================================================================================================
# f32_to_bf16
# =========================================================================================================================
BF16_NS = (4, 1028, 4 * 256 * 4096 + 1024)
BF16_SPECIAL = (0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,      # ties to even (down, up), around
                0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x80008000,       # subnormals
                0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF,       # inf, 0, the largest
                0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF, 0xFF810000, 0x7FBFFFFF)                   # NaN, quiet and signalling


def gen_bf16(n, seed=0):
    """the special values at both ends (a buffer of 4 takes the first four and is run once per group of four)"""
    g = torch.Generator().manual_seed(16000 + n % 9973 + seed)
    x = (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8.0)).float()
    sp = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in BF16_SPECIAL], dtype=torch.int32).view(torch.float32)
    k = len(sp)
    if n >= 2 * k + 8:
        x[1:1 + k] = sp
        x[n - 1 - k:n - 1] = sp.flip(0)
    else:
        x[:] = sp[(4 * seed + torch.arange(n)) % k]
    return x


def bf16_ref_bits(x):
    """round to nearest even on the bit pattern, as int32 in [0, 65536); a NaN gives 0x7FC0 (judged as "a quiet NaN")"""
    u = _bits(x).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, torch.full_like(r, 0x7FC0), r).to(torch.int32)


def judge_bf16(kernel, got, x):
    """got: a bf16 tensor; x: the float32 input"""
    gb = got.contiguous().view(torch.int16).to(torch.int32).reshape(-1) & 0xFFFF
    want = bf16_ref_bits(x).reshape(-1)
    nan = x.reshape(-1).isnan()
    quiet = ((gb & 0x7FFF) > 0x7F80) & ((gb & 0x0040) != 0)
    ok = torch.where(nan, quiet, gb == want)
    print("%s: %d of %d elements differ (%d NaN inputs)" % (kernel, int((~ok).sum()), ok.numel(), int(nan.sum())))
    assert bool(ok.all()), "%s: %d elements differ, first at %d: got %#06x, want %#06x" % (
        kernel, int((~ok).sum()), int((~ok).nonzero()[0]), int(gb[(~ok).nonzero()[0, 0]]), int(want[(~ok).nonzero()[0, 0]]))
    _note(kernel, "bf16", 0.0, "=bit for bit (a NaN: any quiet NaN)")


# =========================================================================================================================
# the case walks both test modules share: `step` / `bwd` is the code under test (the kernel, or torch's CPU fp32 evaluation)
# =========================================================================================================================
def walk_adam(kernel, n, step):
    """step(p, g, m, v, step, clip, gscale) -> (p', m', v'): steps 1, 2, 3 chained from zero moments on the outputs of the code
    under test, then step 1000 and step 100000 from given moments (both bias corrections round to 1 at the latter), for both
    clips and both gradient scales; every step is judged on its own inputs"""
    for clip in ADAM_CLIPS:
        for gs in ADAM_GSCALES:
            p, g, m, v = gen_adam(n, 0, zero_state=True)
            for k in (1, 2, 3):
                g = gen_adam(n, k)[1]
                p2, m2, v2 = step(p, g, m, v, k, clip, gs)
                judge_adam(kernel, p2, m2, v2, p, g, m, v, adam_hyper(k, clip, gs))
                p, m, v = p2, m2, v2
            for k in (1000, 100000):
                p, g, m, v = gen_adam(n, k)
                p2, m2, v2 = step(p, g, m, v, k, clip, gs)
                judge_adam(kernel, p2, m2, v2, p, g, m, v, adam_hyper(k, clip, gs))
    assert adam_hyper(100000, 5.0, 1.0)["bc1"] == 1.0 and adam_hyper(100000, 5.0, 1.0)["sbc2"] == 1.0


def walk_ce(kernel, V, bwd):
    """bwd(scores, targets, lse32) -> d scores [B, T, V]: the good labels, then each bad label in cell (0, 2), whose row must be
    the softmax term without a one-hot"""
    for bad in (None,) + CE_BAD:
        scores, targets = gen_ce(V, bad)
        lse32 = lse64(scores).float()
        for b in range(CE_B):
            lse32[b, CE_LENS[b]:] = NAN         # the row_lse of an undecoded row is not read
        got = bwd(scores, targets, lse32)
        judge_ce_bwd(kernel if bad is None else kernel + " bad label", got, scores, targets, lse32)
        if bad is not None:
            r = ce_bwd_ref(scores, targets, lse32)
            assert float(r["hot"][0, 2].sum()) == 0.0 and float(r["hot"].sum()) == len(ce_cells()) - 1
