"""References of scoring given captions (csrc/rollout.hip: rollout_score, the `scnattn_rollout_*_sc` and `scnattn_rollout_score`
entries of include/scnattn.h), written from the header's description, not from the kernel.  Every function computes in the
dtype of its inputs (fp64: the reference).  Shared by tests/test_scoring_refs.py (CPU) and the GPU modules
test_gpu_scoring_kernels.py and test_gpu_scoring.py.

THE QUANTITIES.  y_v = logits_v * inv_temp; the ORDER is y descending, index ascending (-0 == +0, as comparing floats has it).
    best  = the first word of the ORDER
    rank  = #{v: y_v > y_t} + #{v < t: y_v == y_t}              t: the given token
    logp  = y_t - (m + log S),   m = max y,   S = sum_v exp(y_v - m)

THE BOUND of the device's logp against `of_y` run in fp64 ON THE DEVICE'S OWN fp32 y (the header defines every quantity on
y_v = fl(logits * inv_temp), the fp32 number, so the product's rounding is part of the input, not of the error), u = 2^-24:
    d_v = fl(y_v - m)          one fp32 rounding: |d_v| (1 + delta), |delta| <= u.  exp(d (1 + delta)) = exp(d) exp(d delta): a
                               RELATIVE error of the term of at most u |d_v| <= u dmax (first order), dmax = max over the
                               finite y_v of |y_v - m|
    e_v = expf(d_v)            the documented error of the device's expf is 1 ulp, and an ulp is at most 2u of the value: 2u.
                               A term below the fp32 normal range may be flushed: an absolute error below 2^-126 per term,
                               2^-106 for 2^20 terms, against S >= 1 (the maximum's own term is expf(0) = 1 exactly).
                               A -inf logit contributes exactly 0 on both sides.
    S                          every term is non-negative and relatively within u (dmax + 2), hence so is their exact sum; the
                               fp64 summation of V <= 2^20 terms adds at most V 2^-53 <= 2^-33.  S is relatively within
                               u (dmax + 2) + 2^-32 IN ANY ORDER of the terms, so the fixed order of the kernel does not enter.
    log S                      log(S (1 + eps)) = log S + eps: the relative error becomes an ABSOLUTE one.  The fp64 log, sum
                               and difference add a few 2^-53 of |m| + |log S| + |y_t| (< 2^-44 for |y| < 2^8): with the 2^-32
                               above, well inside one more u.
    (float)                    the ONE rounding to fp32: u |logp|
    bound = 2 u (dmax + 3 + |logp|)
the leading 2 being the project's safety factor (it also covers the second-order terms, (u dmax)^2 < 2^-32 for dmax < 256).
An infinite logp (a -inf target) must be met exactly.

RANK AND BEST are exact: the device compares the same fp32 numbers, and comparing two floats has no rounding.  On the fp32 y
widened to fp64, #{y_v > y_t} <= rank <= #{y_v >= y_t}, and with ties resolved by index the interval collapses to the ORDER's
count: equality is asserted.  In a whole run (`score`) the device's y differ from the reference's by the decode step's error,
so there rank / best are judged only where the reference's gap between the target (the maximum) and its neighbours in the
ORDER exceeds rollout_refs.band with no noise: 16 u (max|y| + 1)."""
import torch
import torch.nn.functional as F

import beam_refs as BR
import rollout_refs as RR
from kernel_harness import U

F64 = torch.float64
MAX_STEPS = BR.MAX_STEPS


def of_y(y, target):
    """y [R, V], target [R] (inside [0, V)) -> dict logp, rank, best [R], dmax [R] (over the finite y), m, S"""
    R, V = y.shape
    target = torch.as_tensor(target, dtype=torch.long)
    m = y.max(dim=1)[0]
    d = y - m.unsqueeze(1)
    S = torch.exp(d).sum(dim=1)
    yt = y.gather(1, target.unsqueeze(1)).squeeze(1)
    logp = yt - (m + torch.log(S))
    idx = torch.arange(V).unsqueeze(0)
    before = (y > yt.unsqueeze(1)) | ((y == yt.unsqueeze(1)) & (idx < target.unsqueeze(1)))
    rank = before.sum(dim=1)
    best = (y == m.unsqueeze(1)).to(torch.int64).argmax(dim=1)       # the first of the maxima
    dmax = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d)).max(dim=1)[0]
    return dict(logp=logp, rank=rank, best=best, dmax=dmax, m=m, S=S)


def score_step(logits, target, inv_temp):
    """logits [R, V] -> (y, logp, rank, best), y = logits * inv_temp in the dtype of `logits`"""
    y = logits * torch.tensor(inv_temp, dtype=logits.dtype)
    r = of_y(y, target)
    return y, r["logp"], r["rank"], r["best"]


def logp_bound(r):
    """per row: 2 u (dmax + 3 + |logp|); infinite where logp is (judge those by equality)"""
    return 2.0 * U * (r["dmax"].double() + 3.0 + r["logp"].double().abs())


def rank_interval(y, target):
    """(#{y_v > y_t}, #{y_v >= y_t}) per row on y widened to fp64"""
    y = y.double()
    yt = y.gather(1, torch.as_tensor(target, dtype=torch.long).unsqueeze(1))
    return (y > yt).sum(dim=1), (y >= yt).sum(dim=1)


def gaps(y, target):
    """per row of y [R, V]: (the smallest |y_v - y_t| over v != t, the gap between the two largest y); inf for V = 1"""
    R, V = y.shape
    inf = torch.full((R,), float("inf"), dtype=y.dtype)
    if V == 1:
        return inf, inf
    target = torch.as_tensor(target, dtype=torch.long)
    diff = (y - y.gather(1, target.unsqueeze(1))).abs()
    diff.scatter_(1, target.unsqueeze(1), float("inf"))
    top = torch.topk(y, 2, dim=1)[0]
    return diff.min(dim=1)[0], top[:, 0] - top[:, 1]


# ---- a whole teacher-forced run ------------------------------------------------------------------------------------------
def score(kind, Pm, K, word_map, encoder_out, tag_out, targets, ntok, inv_temp=1.0):
    """N images x K slots from beam_refs' attention pieces and the cells of oracle/scnattn_ref, in the dtype of the
    parameters, like rollout_refs.rollout with the tokens given: targets [R][>= ntok[r]], ntok [R].  -> dict: logp, rank, best
    [R][ntok[r]], sum_logp [R] (accumulated in the dtype), alpha [steps] of [R, P] (attention), tgap / bgap [R][ntok[r]] (the
    target's distance to its nearest neighbour, the gap of the two largest y), band [R][ntok[r]], bound_score / bound_pick
    [R][ntok[r]] (this module's bound of logp and rollout_refs' bound of the pick's logp at the same token, from the
    reference's y), steps = max ntok."""
    from oracle import scnattn_ref as R_
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    start = word_map["<start>"]
    N, hh, ww, E = encoder_out.shape
    enc = encoder_out.reshape(N, hh * ww, E)
    R = N * K
    dt = enc.dtype
    mean = enc.mean(1)
    h = F.linear(mean, Pm["init_h.weight"], Pm["init_h.bias"]).repeat_interleave(K, 0)
    c = F.linear(mean, Pm["init_c.weight"], Pm["init_c.bias"]).repeat_interleave(K, 0)
    tags = tag_out.repeat_interleave(K, 0) if use_tags else None
    emb = Pm["embedding.weight"][start].expand(R, -1)
    if use_att:
        att1 = F.linear(enc, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
    ntok = [int(x) for x in ntok]
    steps = max(ntok + [0])
    out = dict(logp=[[] for _ in range(R)], rank=[[] for _ in range(R)], best=[[] for _ in range(R)],
               tgap=[[] for _ in range(R)], bgap=[[] for _ in range(R)], band=[[] for _ in range(R)],
               bound_score=[[] for _ in range(R)], bound_pick=[[] for _ in range(R)], alpha=[], steps=steps)
    sum_logp = [torch.zeros((), dtype=dt) for _ in range(R)]
    for t in range(steps):
        if use_att:
            att2 = F.linear(h, Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
            e = BR.attn_scores(att1, att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                               Pm["attention.full_att.bias"], K)["e"]
            gpre = F.linear(h, Pm["f_beta.weight"], Pm["f_beta.bias"])
            ctx = BR.attn_context(enc, e, gpre.unsqueeze(0), None, K)
            out["alpha"].append(ctx["alpha"])
            step_in = torch.cat([emb, ctx["z"]], dim=1)
        else:
            step_in = emb
        if kind == "pure_attention":
            h, c = R_.lstm_cell_forward(Pm, "decode_step.", step_in, (h, c))
        else:
            h, c = R_.scn_cell_forward(Pm, "decode_step.", step_in, tags, (h, c))
        logits = F.linear(h, Pm["fc.weight"], Pm["fc.bias"])
        tgt = [int(targets[r][t]) if t < ntok[r] else 0 for r in range(R)]
        y, logp, rank, best = score_step(logits, tgt, inv_temp)
        bs = logp_bound(of_y(y, tgt))
        tg, bg = gaps(y, tgt)
        band = 16.0 * U * (y.abs().max(dim=1)[0].double() + 1.0)
        for r in range(R):
            if t >= ntok[r]:            # closed: zero records; the slot keeps computing on <pad> and is ignored
                continue
            out["logp"][r].append(float(logp[r]))
            out["rank"][r].append(int(rank[r]))
            out["best"][r].append(int(best[r]))
            out["tgap"][r].append(float(tg[r]))
            out["bgap"][r].append(float(bg[r]))
            out["band"][r].append(float(band[r]))
            out["bound_score"][r].append(float(bs[r]))
            out["bound_pick"][r].append(RR.logp_at(dict(y=y), r, tgt[r])[1])
            sum_logp[r] = sum_logp[r] + logp[r]
        emb = Pm["embedding.weight"][torch.tensor(tgt)]
    out["sum_logp"] = [float(s) for s in sum_logp]
    return out


def combine_at(ls, w, mode):
    """the header's ensemble formula at one word: ls the members' log-probabilities of it (tensors), w the weights"""
    if mode == 0:
        c = w[0] * ls[0]
        for wm, l in zip(w[1:], ls[1:]):
            c = c + wm * l
        return c
    a = ls[0]
    for l in ls[1:]:
        a = torch.maximum(a, l)
    s = w[0] * torch.exp(ls[0] - a)
    for wm, l in zip(w[1:], ls[1:]):
        s = s + wm * torch.exp(l - a)
    return a + torch.log(s)
