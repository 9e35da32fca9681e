"""References of scheduled sampling (csrc/rollout.hip: rollout_pick_mixed, the `scnattn_rollout_*_ss` and
`scnattn_rollout_pick_mixed` entries of include/scnattn.h), written from the header's description, not from the kernel.  Every
function computes in the dtype of its inputs (fp64: the reference).  Shared by tests/test_scheduled_refs.py (CPU) and the GPU
modules test_gpu_scheduled_kernels.py, test_gpu_scheduled.py and test_gpu_scheduled_step.py.

THE COIN.  bits = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (0xFFFFFFFF, row, t, draw);
u = ((bits >> 9) + 0.5) * 2^-23 has 24 significant bits, so it is the same number in fp32 and fp64; prob is rounded to fp32
first (the kernel's argument is a float), and comparing two floats has no rounding: `replaced = u < prob` is EXACT, and the
tests ask for equality.

A REPLACED position is rollout_refs.pick (the band of the token, the bound of logp: its docstring); with `greedy` every row
is an arg-max row.  A position that keeps its gold word involves no arithmetic at all.

DECIDABILITY of a whole run (rollout_refs.decidable_rows): only the REPLACED positions enter it -- only they are discrete
choices of the model and only they steer the chain; a gold word is given.  top2 / own hold one entry per replaced position."""
import numpy as np
import torch
import torch.nn.functional as F

import beam_refs as BR
import rollout_refs as RR
from helpers import params_from, t as _t

F64 = torch.float64
MAX_STEPS = BR.MAX_STEPS
COIN_WORD = 0xFFFFFFFF


# ---- the coin --------------------------------------------------------------------------------------------------------------
def coin_bits(seed, draw, rows, t):
    """uint32 array, one per row (rows / t broadcast as numpy arrays)"""
    return RR.philox4x32_10((COIN_WORD, np.asarray(rows), np.asarray(t), draw), (seed & 0xFFFFFFFF, seed >> 32))[0]


def coin_u(seed, draw, rows, t):
    """u as float64 (exact)"""
    return ((coin_bits(seed, draw, rows, t) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def fl32(x):
    return float(np.float32(x))


def coin(seed, draw, rows, t, prob):
    """replaced: bool array, u < fl32(prob)"""
    return coin_u(seed, draw, rows, t) < fl32(prob)


# ---- one mixed step ----------------------------------------------------------------------------------------------------------
def pick_of(logits, K, inv_temp, seed, draw, t, greedy):
    """rollout_refs.pick of every row, as the mixed kernel would pick IF the row is replaced: with greedy every row takes the
    arg-max (a pick whose every slot is slot 0), else no row does"""
    return RR.pick(logits, 1, inv_temp, seed, draw, t, True) if greedy else RR.pick(logits, K, inv_temp, seed, draw, t, False)


def mixed_step(logits, K, inv_temp, prob, seed, draw, t, greedy, gold_t, nmix):
    """logits [R, V], gold_t [R], nmix [R] -> dict: open [R] bool, replaced [R] bool, token / sample [R] (int), logp [R] (the
    dtype of logits), closing [R] bool, p (the pick of every row)"""
    R = logits.shape[0]
    p = pick_of(logits, K, inv_temp, seed, draw, t, greedy)
    nmix = torch.as_tensor(nmix, dtype=torch.long)
    is_open = t < nmix
    rep = torch.from_numpy(coin(seed, draw, np.arange(R), t, prob)) & is_open
    gold_t = torch.as_tensor(gold_t, dtype=torch.long)
    token = torch.where(rep, p["token"], torch.where(is_open, gold_t, torch.zeros_like(gold_t)))
    sample = torch.where(rep, p["token"], torch.full_like(gold_t, -1))
    logp = torch.where(rep, p["logp"], torch.zeros_like(p["logp"]))
    return dict(open=is_open, replaced=rep, token=token, sample=sample, logp=logp, closing=is_open & (t + 1 == nmix), p=p)


# ---- a whole mixed run ---------------------------------------------------------------------------------------------------------
def mix_rollout(kind, Pm, K, word_map, encoder_out, tag_out, gold, nmix, prob, seed, draw, inv_temp=1.0, greedy=False,
                samples=None):
    """N images x K slots like rollout_refs.rollout, in the dtype of the parameters, with the gold words gold [R][>= nmix[r]]
    and the coin.  -> dict: tokens, sample, replaced [R][nmix[r]], logp [R][nmix[r]], sum_logp [R], alpha [steps] of [R, P]
    (attention), top2 / own [R][one per REPLACED position] (rollout_refs.decidable_rows), steps = max nmix.
    samples: forced picks [R][...] at the replaced positions (the fp32 run of the decidability rule follows the fp64 run's)."""
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
    nmix = [min(max(int(x), 0), MAX_STEPS) for x in nmix]
    steps = max(nmix + [0])
    V = len(word_map)
    out = dict(tokens=[[] for _ in range(R)], sample=[[] for _ in range(R)], replaced=[[] for _ in range(R)],
               logp=[[] for _ in range(R)], top2=[[] for _ in range(R)], own=[[] for _ in range(R)], alpha=[], steps=steps)
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
        p = pick_of(logits, K, inv_temp, seed, draw, t, greedy)
        rep = coin(seed, draw, np.arange(R), t, prob)
        nxt = []
        for r in range(R):
            if t >= nmix[r]:                # closed: zero records, the slot keeps computing on <pad> and is ignored
                nxt.append(0)
                continue
            if not rep[r]:
                tok, lp = int(gold[r][t]), 0.0
                out["sample"][r].append(-1)
            else:
                tok = int(p["token"][r]) if samples is None else int(samples[r][t])
                lp_t = p["y"][r, tok] - p["lse"][r]
                lp = float(lp_t)
                srt = torch.sort(p["key"][r], descending=True)[0]
                mine = int(p["token"][r]) == tok
                out["own"][r].append(mine)
                out["top2"][r].append((float(p["key"][r, tok]), float((srt[1] if mine else srt[0]) if V > 1 else -float("inf"))))
                out["sample"][r].append(tok)
                sum_logp[r] = sum_logp[r] + lp_t
            out["tokens"][r].append(tok)
            out["replaced"][r].append(bool(rep[r]))
            out["logp"][r].append(lp)
            nxt.append(min(max(tok, 0), V - 1))
        emb = Pm["embedding.weight"][torch.tensor(nxt)]
    out["sum_logp"] = [float(s) for s in sum_logp]
    return out


# ---- the cases of the driver tests (the issue's: decided on the CPU, 0 of 90 rows left out) ----------------------------------
INV_TEMP = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))
SEED, DRAW = 5, 0
MIXES = ((1, 0.5, False), (2, 0.25, False), (1, 0.5, True), (1, 1.0, False))       # (K, prob, greedy)
_CASES = {}


def gold_of(R, V):
    """(gold [R, 51] int64, nmix [R] int64): the generator's draws in this order, then the fixed rows"""
    g = torch.Generator().manual_seed(11)
    nmix = torch.randint(0, 51, (R,), generator=g)
    gold = torch.randint(1, V - 3, (R, 51), generator=g)
    nmix[0] = 50
    if R > 2:
        nmix[1], nmix[2] = 0, 1
    return gold, nmix


def driver_case(name, kind, mix):
    """-> dict d, wm, enc, tags, K, prob, greedy, gold, nmix, ref (fp64), ok (per row); computed once, shared, left unchanged"""
    key = (name, mix)
    if key not in _CASES:
        K, prob, greedy = mix
        d, V = BR.sharpened(name)
        wm = BR.word_map(V)
        enc = _t(d["enc"])
        tags = _t(d["tags"]) if kind != "pure_attention" else None
        gold, nmix = gold_of(enc.shape[0] * K, V)
        P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
        a = (K, wm)
        b = (gold.tolist(), nmix.tolist(), prob, SEED, DRAW, INV_TEMP, greedy)
        r64 = mix_rollout(kind, P64, *a, enc.double(), None if tags is None else tags.double(), *b)
        r32 = mix_rollout(kind, P32, *a, enc.float(), None if tags is None else tags.float(), *b,
                          samples=r64["tokens"])      # read at the replaced positions only
        _CASES[key] = dict(d=d, wm=wm, enc=enc, tags=tags, K=K, prob=prob, greedy=greedy, gold=gold, nmix=nmix, ref=r64,
                           ok=RR.decidable_rows(r64, r32))
    return _CASES[key]


def as_caps(wm, gold, nmix, L=None):
    """the form `forward` takes, for which mix_batch's nmix is the given one: caps (R, L) = <start>, nmix gold words, one last
    gold word (<end>), <pad> ...; caplens = nmix + 2.  A row with nmix == 0 alternates between caplens 2 (<start>, <end>) and
    an empty slot (caplens 0)."""
    R = gold.shape[0]
    L = L or int(nmix.max()) + 2
    caps = torch.full((R, L), wm["<pad>"], dtype=torch.int64)
    caplens = torch.zeros(R, 1, dtype=torch.int64)
    for r in range(R):
        n = int(nmix[r])
        if n == 0 and r % 2 == 0:
            continue
        caps[r, 0] = wm["<start>"]
        caps[r, 1:1 + n] = gold[r, :n]
        caps[r, 1 + n] = wm["<end>"]
        caplens[r] = n + 2
    return caps, caplens
