"""References of TRUNCATED sampling (top-k / nucleus; csrc/rollout.hip: rollout_pick_filtered, the `scnattn_rollout_*_f`
entries of include/scnattn.h), written from the header's description, not from the kernel.  They reuse the Philox noise, `pick`,
the key band and the rollout of tests/rollout_refs.py and compute in the dtype of their inputs (fp64: the reference).  Shared by
tests/test_sampling_refs.py (CPU) and the GPU modules test_gpu_sampling_kernels.py and test_gpu_sampling.py.

THE SEMANTICS (restated).  y_v = fl(logits_v * inv_temp); the ORDER is y descending, index ascending (-0 == +0, -inf last).
    L_k = top_k when 1 <= top_k < V, else V
    L_p = the smallest L >= 1 with sum_{i<L} e_(i) >= top_p * sum_all e, e_v = exp(fl(y_v - m)), m = max y, e = 0 for y = -inf;
          the terms in the dtype of y, the sums and the comparison in fp64; top_p (taken as the fp32 number the library is
          handed) == 1: L_p = V
    nkeep = min(L_k, L_p): the kept set is the first nkeep words of the ORDER.  Both limits are measured on the full
    distribution.  token = the first key in the ORDER among the kept words, key_v = y_v + noisy * g_v with the noise of
    rollout_refs (it does not depend on the filter); logp = y_token - (m + log(sum_kept e)), fp64 up to one final rounding.

WHAT IS EXACT.  In the kernel tests y is handed over as the fp32 product (torch's float32 multiply gives the device's bits),
so the ORDER and L_k are exact: no band.

THE MASS BAND of L_p (u = 2^-24, dmax = max |y - m| over the finite y).  The device's term is e32 = expf(fl(y - m)): the
subtraction rounds once, an ABSOLUTE error u |d| of the argument and so a RELATIVE error u |d| of the term; expf is good to
2 ulp, at most 4 u relative.  Every term of a sum therefore carries a relative error of at most u (dmax + 4), and so does any
sum of them (the terms are non-negative); the fp64 additions of at most 2^20 terms add 2^-32, nothing visible.  The device
decides A >= top_p * S, that is A / S >= top_p, and the ratio of two such sums carries at most u (2 dmax + 8): absolute as
well, the ratio being at most 1.  With c_L the fp64 cumulative mass of the first L words over the whole mass, the device's
comparison can differ from c_L >= top_p only when |c_L - top_p| is inside
    band_m = u (2 dmax + 16)            (twice the 8 for room; independent of V).
    L_lo = the shortest prefix with c >= top_p - band_m,   L_hi = the shortest prefix with c >= top_p + band_m (V if none)
and a device nkeep is ACCEPTED iff min(L_k, L_lo) <= nkeep <= min(L_k, L_hi).  A row is SHARP when the two ends coincide.

TOKEN AND LOGP are judged GIVEN THE DEVICE'S nkeep (inside its range): the token must be within rollout_refs' key band of
the fp64 maximum over the first nkeep words of the ORDER and the lowest index among the kept keys exactly equal to its own.
THE BOUND of logp = y_token - (m + log s), s = sum_kept e, dk = max |y - m| over the KEPT words: s carries the relative
error u (dk + 4) of its terms (above; the fp64 sum adds nothing visible, which is where rollout_refs' 4 (V + 8) went), log s
turns it into an absolute one, y_token and m are the device's own numbers, and the one rounding to fp32 costs u |logp|:
    bound = u (|logp| + 2 dk + 8)       (the term part doubled for room).
For nkeep = 1 every part vanishes but the 8 u: s = expf(0) = 1 and logp = +0.0 exactly.

A WHOLE FILTERED ROLLOUT is rollout_refs.rollout with this pick in place of its own.  There y comes out of a decoder in the
dtype of the parameters, so neither the ORDER nor the masses are the device's to the bit, and the decidability rule of
rollout_refs.decidable_rows is EXTENDED (decidable_rows below): a row also needs, at every open step,
    (1) SHARP in fp64, and the fp32 reference's nkeep equal to the fp64 reference's;
    (2) the cut clear of the threshold: with need_m = max(8 x the worst fp32-vs-fp64 difference of the cumulative masses
        next to the cut over the row's steps, 1e-5), top_p - c_{nkeep} >= need_m where top-k binds (nkeep = L_k < L_p), else
        c_{nkeep} - top_p >= need_m and top_p - c_{nkeep-1} >= need_m (c_0 = 0);
    (3) the words on either side of the cut apart: y_(nkeep) - y_(nkeep+1) >= max(8 x the worst fp32-vs-fp64 key difference
        of the row, 1e-5) when nkeep < V, so that the kept SET, not only its size, is the same;
the 8 x and the 1e-5 being those of the key rule, for the same reason: the device's logits differ from the fp32 reference's
by about what the fp32 reference's differ from the fp64 one's."""
import contextlib

import numpy as np
import torch

import rollout_refs as RR
from kernel_harness import U

F64 = torch.float64
_PLAIN_PICK = RR.pick   # rollout() below swaps RR.pick for the filtered one while rollout_refs.rollout runs
OUTSIDE = -1e30         # the key of a word outside the kept set in a whole rollout: finite, so that key differences stay numbers


def f32(x):
    """the fp32 number the library is handed"""
    return float(np.float32(x))


def y32(logits, inv_temp):
    """the device's y: ONE fp32 product per word"""
    return logits.float() * torch.tensor(inv_temp, dtype=torch.float32)


def order(y):
    """the ORDER: indices by y descending, index ascending (-0 == +0; -inf last)"""
    return torch.sort(-(y + 0.0), stable=True)[1]


def terms(y):
    """e_v = exp(fl(y_v - m)) in the dtype of y, 0 for -inf; -> (e, m)"""
    m = y.max()
    e = torch.where(torch.isinf(y) & (y < 0), torch.zeros_like(y), torch.exp(y - m))
    return e, m


def band_m(y):
    fin = y[torch.isfinite(y)].double()
    dmax = float((fin - fin.max()).abs().max()) if fin.numel() else 0.0
    return U * (2.0 * dmax + 16.0)


def _shortest(c, x):
    """the shortest prefix length L >= 1 with c_L >= x; V when there is none"""
    hit = (c >= x).nonzero()
    return int(hit[0]) + 1 if hit.numel() else c.numel()


def kept(y, top_k, top_p):
    """One row y [V] (the dtype of the terms) -> dict: order [V]; L_k; L_p (None when top_p is off); nkeep; lo, hi (the
    accepted range of a device nkeep); sharp; c (fp64 cumulative mass over the whole mass along the ORDER, c[L-1] = c_L)"""
    V = y.numel()
    top_k, top_p = int(top_k), f32(top_p)
    assert top_k >= 0 and 0.0 < top_p <= 1.0
    o = order(y)
    L_k = top_k if 1 <= top_k < V else V
    e, _ = terms(y)
    ed = e[o].double()
    cum = torch.cumsum(ed, 0)
    total = ed.sum()
    c = cum / total
    if top_p == 1.0:
        L_p, lo_p, hi_p = None, V, V
    else:
        L_p = _shortest(cum, top_p * total)
        b = band_m(y)
        lo_p, hi_p = _shortest(c, top_p - b), _shortest(c, top_p + b)
    nkeep = min(L_k, V if L_p is None else L_p)
    lo, hi = min(L_k, lo_p), min(L_k, hi_p)
    return dict(order=o, L_k=L_k, L_p=L_p, nkeep=nkeep, lo=lo, hi=hi, sharp=lo == hi, c=c, top_p=top_p)


def pick(logits, K, inv_temp, seed, draw, t, greedy_first, top_k=0, top_p=1.0, rows=None, nkeep=None):
    """rollout_refs.pick inside the kept set: logits [R, V] -> its dict (y, g, key over ALL words, lse of the KEPT words) with
    token / logp / gap taken among the kept words, and per row: kept (the dicts of `kept`), nkeep, mask [R, V].
    nkeep: forced sizes per row (the device's own, to judge token and logp given them).  Filter off: rollout_refs.pick's
    numbers exactly."""
    p = _PLAIN_PICK(logits, K, inv_temp, seed, draw, t, greedy_first, rows=rows)
    R, V = logits.shape
    dt = logits.dtype
    ks, mask = [], torch.zeros(R, V, dtype=torch.bool)
    token, logp, lse, gap, nk = [], [], [], [], []
    off = (not 1 <= int(top_k) < V) and f32(top_p) == 1.0
    for i in range(R):
        k = kept(p["y"][i], top_k, top_p)
        n = k["nkeep"] if nkeep is None else int(nkeep[i])
        idx = k["order"][:n]
        mask[i, idx] = True
        ks.append(k)
        nk.append(n)
        if off and nkeep is None:
            token.append(int(p["token"][i])), logp.append(p["logp"][i]), lse.append(p["lse"][i]), gap.append(p["gap"][i])
            continue
        key = p["key"][i][idx]
        srt = torch.sort(idx)[0]                                    # kept words by index: the tie rule among equal keys
        tok = int(srt[RR.first_in_order(p["key"][i][srt])])
        e, m = terms(p["y"][i])
        l = (m.double() + torch.log(e[idx].double().sum()))
        token.append(tok)
        lse.append(l.to(dt))
        logp.append((p["y"][i, tok].double() - l).to(dt))
        top = torch.sort(key, descending=True)[0]
        gap.append(top[0] - top[1] if n > 1 else torch.tensor(float("inf"), dtype=dt))
    p.update(token=torch.tensor(token), logp=torch.stack(logp), lse=torch.stack(lse), gap=torch.stack(gap), kept=ks,
             nkeep=nk, mask=mask)
    return p


def key_band(p, i):
    """rollout_refs' band of row i, 16 u (max|y| + max|g| + 1), over the FINITE y (a -inf word has no key to mis-order)"""
    y = p["y"][i]
    fin = y[torch.isfinite(y)]
    ymax = float(fin.abs().max()) if fin.numel() else 0.0
    return 16.0 * U * (ymax + float(p["g"][i].abs().max()) + 1.0)


def nkeep_ok(p, i, nkeep):
    return p["kept"][i]["lo"] <= nkeep <= p["kept"][i]["hi"]


def token_ok(p, i, tok, nkeep):
    """the device's token of row i given ITS nkeep: among the first nkeep words of the ORDER, inside the key band of their
    fp64 maximum, and the lowest index among the kept keys exactly equal to its own"""
    idx = p["kept"][i]["order"][:nkeep]
    if tok not in idx.tolist():
        return False
    key = p["key"][i].double()
    if not float(key[idx].max() - key[tok]) <= key_band(p, i):
        return False
    return int(torch.sort(idx[key[idx] == key[tok]])[0][0]) == tok


def logp_at(p, i, tok, nkeep):
    """fp64 logp of row i at the DEVICE's token over the first nkeep words of the ORDER, and its bound (docstring); the terms
    are taken from the fp64 image of y"""
    y = p["y"][i].double()
    idx = p["kept"][i]["order"][:nkeep]
    m = y.max()
    s = torch.exp(y[idx] - m).sum()
    want = y[tok] - (m + torch.log(s))
    d = (y[idx] - m).abs()
    dk = d[torch.isfinite(d)].max()
    return float(want), float(U * (want.abs() + 2.0 * dk + 8.0))


def logp_at_plain(p, i, tok):
    """rollout_refs.logp_at for a filter that is OFF (the plain kernel and its fp32 sums run), dmax over the finite words"""
    y = p["y"][i].double()
    m = y.max()
    s = torch.exp(y - m).sum()
    lse = m + torch.log(s)
    want = y[tok] - lse
    d = (y - m).abs()
    dmax = d[torch.isfinite(d)].max()
    bound = U * (y[tok].abs() + lse.abs() + 2.0 * torch.log(s).abs() + want.abs() + 4.0 * (y.numel() + 8) + 2.0 * dmax + 2.0)
    return float(want), float(bound)


# ---- a whole filtered rollout ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _pick_in_rollout(fn):
    saved = RR.pick
    RR.pick = fn
    try:
        yield
    finally:
        RR.pick = saved


def rollout(kind, Pm, K, word_map, encoder_out, tag_out, seed, draw, inv_temp=1.0, greedy_first=False, top_k=0, top_p=1.0,
            max_steps=RR.MAX_STEPS, tokens=None):
    """rollout_refs.rollout with the filtered pick -> its dict, and per step t (while any row was open) and row r:
    nkeep [steps][R], rank [steps][R] (the place of this run's OWN pick in the ORDER, 0-based), cut [steps][R] = dict(sharp, binds_k, c_in = c_{nkeep}, c_below = c_{nkeep-1}, ygap = y_(nkeep) -
    y_(nkeep+1) or inf).  top2 (rollout_refs) is taken among the KEPT keys: the words outside are no candidates."""
    nk, cut, rank = [], [], []

    def fn(logits, K_, inv_temp_, seed_, draw_, t_, greedy_first_):
        p = pick(logits, K_, inv_temp_, seed_, draw_, t_, greedy_first_, top_k, top_p)
        p["key"] = torch.where(p["mask"], p["key"], torch.full_like(p["key"], OUTSIDE))
        rec = []
        for i, k in enumerate(p["kept"]):
            n, o, y = k["nkeep"], k["order"], p["y"][i]
            rec.append(dict(sharp=k["sharp"], binds_k=k["L_p"] is not None and k["L_k"] < k["L_p"], use_p=k["L_p"] is not None,
                            c_in=float(k["c"][n - 1]), c_below=float(k["c"][n - 2]) if n > 1 else 0.0,
                            ygap=float(y[o[n - 1]] - y[o[n]]) if n < y.numel() else float("inf"), top_p=k["top_p"]))
        nk.append(list(p["nkeep"]))
        rank.append([int((k["order"] == int(p["token"][i])).nonzero()[0]) for i, k in enumerate(p["kept"])])
        cut.append(rec)
        return p

    with _pick_in_rollout(fn):
        res = RR.rollout(kind, Pm, K, word_map, encoder_out, tag_out, seed, draw, inv_temp, greedy_first, max_steps, tokens)
    res["nkeep"], res["cut"], res["rank"] = nk, cut, rank
    return res


def open_steps(res, r):
    return res["length"][r] or res["steps"]


def decidable_rows(r64, r32):
    """rollout_refs.decidable_rows and the three further needs of a filtered rollout (docstring) -> [bool] per row"""
    base = RR.decidable_rows(r64, r32)
    out = []
    for r, good in enumerate(base):
        n = open_steps(r64, r)
        a, b = r64["top2"][r], r32["top2"][r]
        fin = [abs(x - y) for p, q in zip(a, b) for x, y in zip(p, q) if np.isfinite(x) and np.isfinite(y)]
        need_y = max(8.0 * max(fin or [0.0]), 1e-5)
        c64 = [r64["cut"][t][r] for t in range(n)]
        c32 = [r32["cut"][t][r] for t in range(n)]
        worst_m = max([max(abs(x["c_in"] - y["c_in"]), abs(x["c_below"] - y["c_below"])) for x, y in zip(c64, c32)] or [0.0])
        need_m = max(8.0 * worst_m, 1e-5)
        for t in range(n):
            x = c64[t]
            good = good and x["sharp"] and r64["nkeep"][t][r] == r32["nkeep"][t][r]
            if x["use_p"]:
                if x["binds_k"]:
                    good = good and x["top_p"] - x["c_in"] >= need_m
                else:
                    good = good and x["c_in"] - x["top_p"] >= need_m and x["top_p"] - x["c_below"] >= need_m
            good = good and x["ygap"] >= need_y
        out.append(bool(good))
    return out
