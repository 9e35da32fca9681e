"""References of the sampled rollout and of the reward-weighted loss (csrc/rollout.hip, the `scnattn_rollout_*` and
`scnattn_caption_loss_weighted_*` entries of include/scnattn.h), written from the header's description, not from the kernels.
Every function computes in the dtype of its inputs (fp64: the reference).  Shared by tests/test_rollout_refs.py (CPU) and the
GPU modules test_gpu_rollout_kernels.py, test_gpu_rollout.py, test_gpu_weighted_loss.py, test_gpu_scst_step.py.

THE NOISE.  bits_v = word (v & 3) of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (v >> 2, row, t, draw);
u_v = ((bits_v >> 9) + 0.5) * 2^-23 (24 significant bits: exact in fp32 and fp64, inside (0, 1), so -log(u) lies in
[2^-24, 16.64]); g_v = -log(-log(u_v)), in [-2.82, 16.64].  key_v = y_v + g_v with y_v = logits_v * inv_temp; the arg-max slot
has key_v = y_v.  The token is the first key in the order (value descending, index ascending).

THE BAND of the pick test (per row; u = 2^-24).  The device forms each key in fp32 from the same fp32 logits:
    y = fl(x * inv_temp)                      one rounding:                                  u |y|
    L = -logf(u_v), relative error e_in       <= 2 ulp = 2u (the documented bound of the device's logf is 1 ulp; 2 leaves room)
    g = -logf(L)                              log(L (1 + e_in)) = log L + e_in: the inner RELATIVE error is an ABSOLUTE error
                                              of g, 2u; the outer logf adds 2 ulp of its result, 2u |g|
    key = fl(y + g)                           one rounding:                                  u (|y| + |g|)
so |key32 - key64| <= u (2 |y| + 3 |g| + 2) <= 4 u (max|y| + max|g| + 1), and the ORDER of two keys can only change when their
fp64 gap is below twice that, 8 u (max|y| + max|g| + 1).  The band is twice that again,
    band = 16 u (max|y| + max|g| + 1),
(for an arg-max row max|g| = 0; the derivation then over-estimates: a greedy key is y itself, and two keys that differ in fp64
differ in fp32 in the same direction or are equal).  A device token is accepted when its fp64 key is within the band of the
fp64 maximum, and must be the lowest index among the keys EXACTLY equal to its own.  A row is AMBIGUOUS when the fp64 gap
between its two best keys is positive and inside the band; the reference alone decides that, and a case may hold at most 1 %
of such rows.

THE BOUND of logp = y_token - (m + log s), s = sum_v exp(y_v - m), with dmax = max_v |y_v - m|, in any order of the V terms:
    a term exp(d): d = fl(y - m) carries u |d|, a relative error of the term; expf 2 ulp; each re-scaling by exp(m_old - m_new)
    when a new maximum arrives or two partial sums merge costs (u |delta| + 2u + u), the deltas of a term's chain sum to at
    most dmax and a term is re-scaled at most once per term added after it: relative error of s <= u (2 dmax + 2 + 3 V) from
    the terms and u (V + 8) from the additions (the house rule of n terms and 8 more roundings);
    log s: that relative error becomes absolute, plus 2 ulp of |log s|; m + log s rounds once (u |lse|), y_token carries
    u |y_token|, the subtraction rounds once (u |logp|):
    bound = u (|y_token| + |lse| + 2 |log s| + |logp| + 4 (V + 8) + 2 dmax + 2)."""
import numpy as np
import torch
import torch.nn.functional as F

import beam_refs as BR
import train_tail_refs as TT
from kernel_harness import U

F64 = torch.float64
MAX_STEPS = BR.MAX_STEPS
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 scalars -> four uint32 arrays.  Ten rounds; the key is
    bumped by the Weyl constants between rounds (Salmon et al., SC'11)."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]           # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def noise_bits(seed, draw, row, t, V):
    """bits_v for v in [0, V): uint32 [V]"""
    groups = (V + 3) // 4
    w = philox4x32_10((np.arange(groups), row, t, draw), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:V]


def uniform(bits, dtype=F64):
    """u = ((bits >> 9) + 0.5) * 2^-23: exact in either dtype"""
    return (torch.from_numpy((bits >> np.uint32(9)).astype(np.int64)).to(dtype) + 0.5) * 2.0 ** -23


def gumbel(seed, draw, row, t, V, dtype=F64):
    u = uniform(noise_bits(seed, draw, row, t, V), dtype)
    return -torch.log(-torch.log(u))


def first_in_order(key):
    """index of the first element in the order (value descending, index ascending)"""
    return int(torch.sort(-key, stable=True)[1][0])


# ---- the pick of one step ------------------------------------------------------------------------------------------------
def pick(logits, K, inv_temp, seed, draw, t, greedy_first, rows=None):
    """logits [R, V] -> dict: y, g, key [R, V]; token [R]; logp [R] = y_token - logsumexp(y); gap [R] (best minus second-best
    key; inf for V = 1).  rows: the global row numbers of the R rows (default 0 .. R-1), which key the noise."""
    R, V = logits.shape
    dt = logits.dtype
    rows = list(range(R)) if rows is None else list(rows)
    y = logits * torch.tensor(inv_temp, dtype=dt)
    g = torch.zeros(R, V, dtype=dt)
    for i, r in enumerate(rows):
        if not (greedy_first and r % K == 0):
            g[i] = gumbel(seed, draw, r, t, V, dt)
    key = y + g
    token = torch.tensor([first_in_order(key[i]) for i in range(R)])
    lse = torch.logsumexp(y, dim=1)
    logp = y.gather(1, token.unsqueeze(1)).squeeze(1) - lse
    top = torch.sort(key, dim=1, descending=True)[0]
    gap = top[:, 0] - top[:, 1] if V > 1 else torch.full((R,), float("inf"), dtype=dt)
    return dict(y=y, g=g, key=key, token=token, logp=logp, lse=lse, gap=gap)


def band(p):
    """per row: 16 u (max|y| + max|g| + 1)"""
    return 16.0 * U * (p["y"].abs().max(dim=1)[0] + p["g"].abs().max(dim=1)[0] + 1.0).double()


def ambiguous(p):
    gap = p["gap"].double()
    return (gap > 0) & (gap < band(p))


def token_ok(p, i, tok):
    """the device's token of row i: inside the band, and the lowest index among the keys exactly equal to its own"""
    key = p["key"][i].double()
    if not 0 <= tok < key.numel():
        return False
    if float(key.max() - key[tok]) > float(band(p)[i]):
        return False
    return int((key == key[tok]).nonzero()[0]) == tok


def logp_at(p, i, tok):
    """fp64 logp of row i at the DEVICE's token, and its bound"""
    y = p["y"][i].double()
    m = y.max()
    s = torch.exp(y - m).sum()
    lse = m + torch.log(s)
    want = y[tok] - lse
    V = y.numel()
    dmax = (y - m).abs().max()
    bound = U * (y[tok].abs() + lse.abs() + 2.0 * torch.log(s).abs() + want.abs() + 4.0 * (V + 8) + 2.0 * dmax + 2.0)
    return float(want), float(bound)


# ---- the reward-weighted loss --------------------------------------------------------------------------------------------
def weighted_loss(scores, targets, lens, weight, alphas=None, alpha_c=0.0):
    """(1/n) sum_b w[b] sum_{t < lens[b]} (logsumexp(scores[b, t]) - scores[b, t, targets[b, t]]) + alpha_c * mean_{b,p}
    (1 - sum_t alphas[b, t, p])^2, index arithmetic in the dtype of `scores`; -> dict(loss, row_loss [B, T], row_lse [B, T])"""
    B, T, V = scores.shape
    dt = scores.dtype
    row_lse, row_loss = torch.zeros(B, T, dtype=dt), torch.zeros(B, T, dtype=dt)
    n = sum(min(int(l), T) for l in lens)
    for b in range(B):
        for t in range(min(int(lens[b]), T)):
            x = scores[b, t]
            m = x.max()
            row_lse[b, t] = m + torch.log(torch.exp(x - m).sum())
            row_loss[b, t] = (row_lse[b, t] - x[int(targets[b, t])]) * weight[b].to(dt)
    loss = row_loss.sum() / n
    if alphas is not None:
        loss = loss + alpha_c * ((1.0 - alphas.to(dt).sum(dim=1)) ** 2).sum() / (B * alphas.shape[2])
    return dict(loss=loss, row_loss=row_loss, row_lse=row_lse, n=n)


def weighted_bwd(scores, targets, lse, weight, lens, gout):
    """d scores of the weighted loss at the given row_lse: train_tail_refs.ce_bwd_ref with every row times w[b]; the bound is
    that reference's derived bound times |w[b]| plus one more rounding, u |want| (the product (g / N) * w[b])"""
    r = TT.ce_bwd_ref(scores, targets, lse, gout=gout, lens=lens)
    w = weight.double().reshape(-1, 1, 1)
    want = r["want"] * w
    return want, TT.ce_bound(r) * w.abs() + U * want.abs()


# ---- a whole rollout -----------------------------------------------------------------------------------------------------
def rollout(kind, Pm, K, word_map, encoder_out, tag_out, seed, draw, inv_temp=1.0, greedy_first=False,
            max_steps=MAX_STEPS, tokens=None):
    """N images x K slots from beam_refs' attention pieces and the cells of oracle/scnattn_ref, in the dtype of the
    parameters.  -> dict: tokens [R][steps], logp [R][steps], length [R] (0: cut off), sum_logp [R], alpha [steps][R, P]
    (attention), top2 [R][steps] = (the picked key, the best other key) and own [R][steps] (the pick was this run's own first
    key) while the row was open, steps.  tokens: forced picks
    [R][steps] (the fp32 run of the decidability rule follows the fp64 run's tokens, so that their keys can be compared)."""
    from oracle import scnattn_ref as R_
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    V = len(word_map)
    start, end = word_map["<start>"], word_map["<end>"]
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
    length, sum_logp = [0] * R, [0.0] * R
    tok_rec, lp_rec, top2, own = ([[] for _ in range(R)] for _ in range(4))
    alpha = []
    steps = 0
    for t in range(max_steps):
        if all(length):
            break
        steps += 1
        if use_att:
            att2 = F.linear(h, Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
            e = BR.attn_scores(att1, att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                               Pm["attention.full_att.bias"], K)["e"]
            gpre = F.linear(h, Pm["f_beta.weight"], Pm["f_beta.bias"])
            ctx = BR.attn_context(enc, e, gpre.unsqueeze(0), None, K)
            alpha.append(ctx["alpha"])
            step_in = torch.cat([emb, ctx["z"]], dim=1)
        else:
            step_in = emb
        if kind == "pure_attention":
            h, c = R_.lstm_cell_forward(Pm, "decode_step.", step_in, (h, c))
        else:
            h, c = R_.scn_cell_forward(Pm, "decode_step.", step_in, tags, (h, c))
        logits = F.linear(h, Pm["fc.weight"], Pm["fc.bias"])
        p = pick(logits, K, inv_temp, seed, draw, t, greedy_first)
        nxt = []
        for r in range(R):
            if length[r]:                   # closed: <pad> / 0.0 records, the slot keeps computing and is ignored
                tok_rec[r].append(0)
                lp_rec[r].append(0.0)
                nxt.append(0)
                continue
            tok = int(p["token"][r]) if tokens is None else int(tokens[r][t])
            lp = float(p["y"][r, tok] - p["lse"][r])
            srt = torch.sort(p["key"][r], descending=True)[0]
            mine = int(p["token"][r]) == tok
            own[r].append(mine)
            top2[r].append((float(p["key"][r, tok]), float(srt[1] if mine else srt[0])))
            tok_rec[r].append(tok)
            lp_rec[r].append(lp)
            sum_logp[r] = float(torch.tensor(sum_logp[r], dtype=dt) + torch.tensor(lp, dtype=dt))
            if tok == end:
                length[r] = t + 1
            nxt.append(tok)
        emb = Pm["embedding.weight"][torch.tensor(nxt)]
    return dict(tokens=tok_rec, logp=lp_rec, length=length, sum_logp=sum_logp, alpha=alpha, top2=top2, own=own, steps=steps)


def decidable_rows(r64, r32):
    """The rule of the beam tests, per row: (1) the fp32 reference, run on its own, picks the fp64 reference's tokens at every
    step (r32 was run FORCED onto r64's tokens; its `own` says whether each forced token was its own pick); (2) every step's fp64 top-2 key gap is at least
    max(8 x the worst fp32-vs-fp64 key difference of that row, 1e-5).  -> [bool] per row"""
    out = []
    for a, b, mine in zip(r64["top2"], r32["top2"], r32["own"]):
        same = all(mine)
        worst = max([abs(x - y) for p, q in zip(a, b) for x, y in zip(p, q)] or [0.0])
        need = max(8.0 * worst, 1e-5)
        out.append(same and all(k - o >= need for k, o in a))
    return out


def caption_of(res, r, start):
    """[<start>, tokens ...] of row r: up to and including <end>, or every step of a cut-off row"""
    n = res["length"][r] or res["steps"]
    return [start] + res["tokens"][r][:n]


def teacher_forced_logp(kind, Pm, seq, encoder_out, tag_out, inv_temp=1.0):
    """log-likelihood of seq[1:] given seq[:-1] for ONE image through oracle/scnattn_ref's decoder forward, at the
    temperature of the rollout"""
    from oracle import scnattn_ref as R_
    caps = torch.tensor([seq], dtype=torch.long)
    caplens = torch.tensor([[len(seq)]])
    if kind == "attention_scn":
        preds = R_.attention_scn_forward(Pm, encoder_out, tag_out, caps, caplens)[0]
    elif kind == "pure_scn":
        preds = R_.pure_scn_forward(Pm, encoder_out, tag_out, caps, caplens)[0]
    else:
        preds = R_.pure_attention_forward(Pm, encoder_out, caps, caplens)[0]
    lp = torch.log_softmax(preds[0] * inv_temp, dim=1)
    return float(lp.gather(1, caps[0, 1:].unsqueeze(1)).sum())
