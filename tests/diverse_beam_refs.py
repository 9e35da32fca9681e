"""DIVERSE beam search (include/scnattn.h: "DIVERSE beam search") restated in plain torch / Python from the
header's text, not from the kernels, on the pieces of tests/beam_refs.py, tests/beam_options_refs.py and
tests/ensemble_refs.py.  The reference project has no such search: this file is what the GPU tests judge against.

    refusal(groups, K, penalty)            why a search in groups is refused, or None
    merge_groups(...)                      one step's merge of ONE image from the row candidates: the groups in order, each
                                           ranking by a = r - penalty * c and recording raw values
    search(...)                            a whole search of N images, M >= 1 members, G groups of Kg beams, with options:
                                           per image the G results, and one trace entry per (step, group) in the form
                                           beam_refs.decidable takes

`search` ranks ALL nsrc_g x V candidates of a group, not the K per row the kernels exchange: that the two agree is the
top-K argument of the header, which the GPU tests thereby check."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import beam_options_refs as OR
import beam_refs as BR
import ensemble_refs as ER

MAX_BEAM = 8


def refusal(groups, K, penalty):
    """groups >= 1, K in [1, 8] a multiple of groups, penalty finite and >= 0"""
    if groups < 1:
        return "groups"
    if not 1 <= K <= MAX_BEAM:
        return "beam_size"
    if K % groups:
        return "multiple"
    if not (math.isfinite(penalty) and penalty >= 0.0):
        return "penalty"
    return None


def selection_value(r, c, penalty, dtype):
    """a = fmaf(-penalty, c, r) in `dtype`.  fp32: the product of an fp32 penalty and a count <= 8 is exact in fp64 and so is
    its sum with an fp32 r unless the exponents lie more than 2**28 apart, so rounding the fp64 result once to fp32 IS the
    fused multiply-add; fp64: the plain expression."""
    if dtype == torch.float32:
        return float(np.float32(np.float64(np.float32(r)) - np.float64(np.float32(penalty)) * c))
    return r - penalty * c if c else r


class GroupState(BR.ImageState):
    """what the merge keeps per (image, group): beam_refs.ImageState with Kg slots"""


def rank_group(cands, kk):
    """cands: [(a, flat, r)] -> the kk first under (a descending, flat ascending)"""
    return sorted(cands, key=lambda x: (-x[0], x[1]))[:kk]


def merge_groups(candv, candi, V, Kg, penalty, nsrc, kk):
    """candv / candi [K, K] of ONE image (row g*Kg + j: the K candidates of slot j of group g, best first; rows of dead slots
    are not looked at); nsrc / kk: G numbers.  -> per group None (finished: kk == 0) or the kk picks
    [(raw value, slot j IN THE GROUP, word)] in rank order of a"""
    K = candv.shape[1]
    G = K // Kg
    count = {}
    out = []
    for g in range(G):
        if kk[g] <= 0:
            out.append(None)
            continue
        cands = []
        for j in range(nsrc[g]):
            for r in range(K):
                v, w = float(candv[g * Kg + j, r]), int(candi[g * Kg + j, r])
                cands.append((selection_value(v, count.get(w, 0), penalty, candv.dtype), j * V + w, v))
        picks = [(v, flat // V, flat % V) for _, flat, v in rank_group(cands, kk[g])]
        for _, _, w in picks:
            count[w] = count.get(w, 0) + 1
        out.append(picks)
    return out


STATE = ("open_images", "nsrc", "kk", "ncomp", "best_idx", "best_score", "scores", "comp_score", "comp_step", "comp_parent",
         "token", "parent")


def merge_state(st, candv, candi, N, K, Kg, V, end, t, penalty):
    """What the merge of step t leaves of the state `st` (a dict of host tensors by the names of scnattn_beam_layout, the
    per-group arrays [N*G], token / parent [T][N*K]) given candv / candi [N*K, K]: a new dict.  Per open group: <end> picks
    recorded at n*K + g*Kg + ncomp (score raw, step t, parent a slot of the IMAGE; best replaced on strictly greater), the
    others compacted to the group's slots in rank order, dead slots a copy of the group's slot 0 (zeros when nothing is
    open) with score 0; a finished group untouched; open_images loses the images whose last open group closed."""
    out = {k: v.clone() for k, v in st.items()}
    G = K // Kg
    for n in range(N):
        sl = slice(n * G, (n + 1) * G)
        nsrc, kk = st["nsrc"][sl].tolist(), st["kk"][sl].tolist()
        if not any(k > 0 for k in kk):
            continue
        picks = merge_groups(candv[n * K:(n + 1) * K], candi[n * K:(n + 1) * K], V, Kg, penalty, nsrc, kk)
        for g, pk in enumerate(picks):
            if pk is None:
                continue
            sg, r0 = n * G + g, n * K + g * Kg
            opened = []
            for v, j, w in pk:
                if w == end:
                    nc = int(out["ncomp"][sg])
                    out["comp_score"][r0 + nc], out["comp_step"][r0 + nc], out["comp_parent"][r0 + nc] = v, t, g * Kg + j
                    if int(out["best_idx"][sg]) < 0 or v > float(out["best_score"][sg]):
                        out["best_idx"][sg], out["best_score"][sg] = nc, v
                    out["ncomp"][sg] = nc + 1
                else:
                    opened.append((w, g * Kg + j, v))
            fill = (opened[0][0], opened[0][1], 0.0) if opened else (0, 0, 0.0)
            for s, (w, p, v) in enumerate(opened + [fill] * (Kg - len(opened))):
                out["token"][t, r0 + s], out["parent"][t, r0 + s], out["scores"][r0 + s] = w, p, v
            out["nsrc"][sg] = out["kk"][sg] = len(opened)
        if not bool((out["kk"][sl] > 0).any()):
            out["open_images"][0] -= 1
    return out


def hand_made():
    """(V, Kg, end, penalty, candv [6,6], candi [6,6]) for (G, Kg) = (3, 2) with exactly representable values:
    group 0 (slot 0 live) picks word 3 (-1.0) and <end> (-1.5);
    group 1 (slots 0, 1 live): slot 0's word 3 at -1.0 is penalised to -1.5 and TIES its word 5 at -1.5 -- flat index 3 < 5,
    the penalised one first; slot 1's word 3 at -0.25 -> -0.75 comes first of all; it picks word 3 twice;
    group 2 (slot 0 live): word 3 has c = 3 (-0.5 -> -2.0), <end> c = 1 (-1.0 -> -1.5): it picks <end>, then word 4 (-1.75);
    with group 1 finished instead, word 3 has c = 1 (-0.5 -> -1.0) and group 2 picks word 3, then <end>."""
    V, Kg, K = 8, 2, 6
    v = torch.full((K, K), -99.0)
    i = torch.arange(K, dtype=torch.int32).repeat(K, 1)
    v[0, :3], i[0, :3] = torch.tensor([-1.0, -1.5, -2.0]), torch.tensor([3, 7, 1], dtype=torch.int32)
    v[2, :3], i[2, :3] = torch.tensor([-1.0, -1.5, -3.0]), torch.tensor([3, 5, 2], dtype=torch.int32)
    v[3, :3], i[3, :3] = torch.tensor([-0.25, -4.0, -5.0]), torch.tensor([3, 6, 0], dtype=torch.int32)
    v[4, :4], i[4, :4] = torch.tensor([-0.5, -1.0, -1.75, -2.5]), torch.tensor([3, 7, 4, 6], dtype=torch.int32)
    return V, Kg, 7, 0.5, v, i


# ---- the whole search ---------------------------------------------------------------------------------------------------
def search(kinds, params_list, w, mode, kg, G, penalty, word_map, encoder_out, tag_out, options=OR.Opts(), alpha_member=None,
           max_steps=BR.MAX_STEPS):
    """beam_options_refs.search in G groups of kg beams (K = G * kg rows per image, group g in rows n*K + g*kg ..).
    -> (results, traces): results[n][g] = (out, [(sequence, score)]) as beam_refs.search returns them for an image, scores
    raw, out chosen by options.length_penalty within the group; traces[n] = one entry per (step, group) the group took part
    in: (picked flat indices j_in_group*V + v, picked RAW values, the top kk+1 selection values a AFTER exclusion and
    penalty)."""
    from oracle import scnattn_ref as R
    mode = ER.MODES.get(mode, mode)
    M, K, V = len(kinds), kg * G, len(word_map)
    assert refusal(G, K, penalty) is None, refusal(G, K, penalty)
    start, end = word_map["<start>"], word_map["<end>"]
    assert OR.refusal(options, V, K, max_steps, end) is None, OR.refusal(options, V, K, max_steps, end)
    N, hh, ww, E = encoder_out.shape
    enc = encoder_out.reshape(N, hh * ww, E)
    rows = N * K
    att = [kind != "pure_scn" for kind in kinds]
    if alpha_member is None:
        alpha_member = att.index(True) if True in att else -1
    mean = enc.mean(1)
    h, c, emb, att1 = [], [], [], []
    for kind, Pm in zip(kinds, params_list):
        h.append(F.linear(mean, Pm["init_h.weight"], Pm["init_h.bias"]).repeat_interleave(K, 0))
        c.append(F.linear(mean, Pm["init_c.weight"], Pm["init_c.bias"]).repeat_interleave(K, 0))
        emb.append(Pm["embedding.weight"][start].expand(rows, -1))
        att1.append(F.linear(enc, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
                    if kind != "pure_scn" else None)
    tags = tag_out.repeat_interleave(K, 0) if tag_out is not None else None
    st = [[GroupState(kg) for _ in range(G)] for _ in range(N)]
    hist = [[[] for _ in range(K)] for _ in range(N)]       # the words of the beam in every slot of the image
    token, parent, alpha = [], [], []
    traces = [[] for _ in range(N)]
    for t in range(max_steps):
        if all(s.kk == 0 for gs in st for s in gs):
            break
        logits, h2, c2 = [], [], []
        for m, (kind, Pm) in enumerate(zip(kinds, params_list)):
            if att[m]:
                att2 = F.linear(h[m], Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
                e = BR.attn_scores(att1[m], att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                                   Pm["attention.full_att.bias"], K)["e"]
                gpre = F.linear(h[m], Pm["f_beta.weight"], Pm["f_beta.bias"])
                ctx = BR.attn_context(enc, e, gpre.unsqueeze(0), None, K)
                if m == alpha_member:
                    alpha.append(ctx["alpha"])
                step_in = torch.cat([emb[m], ctx["z"]], dim=1)
            else:
                step_in = emb[m]
            if kind == "pure_attention":
                hm, cm = R.lstm_cell_forward(Pm, "decode_step.", step_in, (h[m], c[m]))
            else:
                hm, cm = R.scn_cell_forward(Pm, "decode_step.", step_in, tags, (h[m], c[m]))
            h2.append(hm)
            c2.append(cm)
            logits.append(F.linear(hm, Pm["fc.weight"], Pm["fc.bias"]))
        scores = torch.tensor([x for gs in st for s in gs for x in s.scores], dtype=logits[0].dtype)
        val = scores.unsqueeze(1) + ER.combine(logits, w, mode)         # raw values r; the log-sum-exp over all V words
        dtype = val.dtype
        tok_t, par_t = [], []
        for n, gs in enumerate(st):
            count = {}                                  # word -> picks of the groups before, at this step
            new_hist = list(hist[n])
            for g, s in enumerate(gs):
                s0 = g * kg
                if s.kk == 0:                           # finished: the device leaves the zero-filled records alone
                    tok_t += [0] * kg
                    par_t += [0] * kg
                    continue
                cands = []
                for j in range(s.nsrc):
                    raw = val[n * K + s0 + j]
                    a = raw.clone()                     # the selection values of ALL V words of the row
                    for v, cnt in count.items():
                        a[v] = selection_value(float(raw[v]), cnt, penalty, dtype)
                    ex = OR.excluded(hist[n][s0 + j], t, V, end, options)
                    if ex:
                        a[sorted(ex)] = -float("inf")
                    # the row's first kk+1 under the search order hold whatever of the row is among the group's first kk+1
                    for v in torch.sort(-a, stable=True)[1][:s.kk + 1].tolist():
                        if v not in ex:
                            cands.append((float(a[v]), j * V + v, float(raw[v])))
                top = rank_group(cands, s.kk + 1)
                picks = [(r, flat // V, flat % V) for _, flat, r in top[:s.kk]]
                traces[n].append(([j * V + wd for _, j, wd in picks], [r for r, _, _ in picks], [a for a, _, _ in top]))
                for _, _, wd in picks:
                    count[wd] = count.get(wd, 0) + 1
                tk, pr = s.step(picks, t, end)
                for j in range(kg):                     # dead slots: the group's slot 0's parent and word
                    new_hist[s0 + j] = hist[n][s0 + pr[j]] + [tk[j]]
                tok_t += tk
                par_t += [s0 + p for p in pr] if s.nsrc else [0] * kg     # parents are slots of the IMAGE; none open: zeros
            hist[n] = new_hist
        token.append(tok_t)
        parent.append(par_t)
        for m, Pm in enumerate(params_list):
            h[m], c[m], emb[m] = BR.advance(h2[m], c2[m], par_t, tok_t, Pm["embedding.weight"], K)
    steps = len(token)
    ones = torch.ones(1, hh, ww, dtype=enc.dtype)

    def chain(n, t, slot):
        words, arows = [], []
        while t >= 0:
            r = n * K + slot
            words.append(token[t][r])
            slot = parent[t][r]
            arows.append((t, n * K + slot))
            t -= 1
        return [start] + words[::-1], arows[::-1]

    out = []
    for n, gs in enumerate(st):
        per_group = []
        for g, s in enumerate(gs):
            s0 = g * kg
            done = []
            for v, t, j in s.comp:
                words, arows = chain(n, t - 1, s0 + j)
                done.append((words + [end], arows + [(t, n * K + s0 + j)], v))
            i = s.best
            if not done:
                for slot in range(s.nsrc):
                    words, arows = chain(n, steps - 1, s0 + slot)
                    assert words[1:] == hist[n][s0 + slot]          # the history IS the parent chain
                    done.append((words, arows, s.scores[slot]))
                sc = [x[2] for x in done]
                i = sc.index(max(sc))
            if options.length_penalty != 0.0:
                i = OR.pick([(x[0], x[2]) for x in done], options.length_penalty)
            seq, arows, _ = done[i]
            if alpha_member >= 0:
                maps = torch.cat([ones] + [alpha[t][r].view(1, hh, ww) for t, r in arows]).tolist()
                one = (seq, maps)
            else:
                one = seq
            per_group.append((one, [(x[0], x[2]) for x in done]))
        out.append(per_group)
    return out, traces


def search_one(kind, Pm, kg, G, penalty, word_map, encoder_out, tag_out, options=OR.Opts(), max_steps=BR.MAX_STEPS):
    """`search` for one decoder: what decoder.sample_groups(kg, G, penalty, ...) restates"""
    return search([kind], [Pm], [1.0], 0, kg, G, penalty, word_map, encoder_out, tag_out if kind != "pure_attention" else None,
                  options, max_steps=max_steps)


# ---- the tables of tests/test_gpu_diverse_beam_search.py ------------------------------------------------------------------
# The inputs of the option tables (beam_options_refs.inputs: E=256, A=D=F=128, M=64, S=40, 7x7, V=1003, N=3).  A table is
# (G, Kg, options, [(kind, seed, penalty)]); its cases are (kind, seed, image).  Seeds and penalties were chosen on the CPU
# so that this restatement meets the caps that tests/test_diverse_beam_refs.py asserts.
# The random decoders like an early <end>; a minimum length (which also shows that options compose) keeps the groups of
# three tables searching for some steps, the first table runs without options (the _div calls with opt = NULL).
MIN4 = OR.Opts(min_length=4)
NGRAM = OR.Opts(min_length=4, no_repeat_ngram=2, banned_tokens=(OR.UNK,))
_ROWS = [("attention_scn", 2, 0.5), ("attention_scn", 6, 0.5), ("pure_scn", 78, 0.5)]
TABLES = {
    "g2x2": (2, 2, OR.Opts(), _ROWS),
    "g3x2_min4": (3, 2, MIN4, _ROWS),
    "g4x2_min4": (4, 2, MIN4, _ROWS),
    "g3x2_ngram_unk": (3, 2, NGRAM, _ROWS),
}
_CASES = {}


def seq_of(one, kind):
    return one[0] if kind != "pure_scn" else one


def cases(table, idx):
    """cases[image] = (the fp64 results of the G groups, decidable, some group's caption differs from its penalty-0
    caption); once per process"""
    if (table, idx) in _CASES:
        return _CASES[(table, idx)]
    from helpers import params_from
    G, kg, options, rows = TABLES[table]
    kind, seed, lam = rows[idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    r64, t64 = search_one(kind, P64, kg, G, lam, wm, enc.double(), tags.double(), options)
    _, t32 = search_one(kind, P32, kg, G, lam, wm, enc, tags, options)
    zero, _ = search_one(kind, P64, kg, G, 0.0, wm, enc.double(), tags.double(), options)
    out = {}
    for b in range(enc.shape[0]):
        differs = any(seq_of(r64[b][g][0], kind) != seq_of(zero[b][g][0], kind) for g in range(G))
        out[b] = (r64[b], BR.decidable(t64[b], t32[b]), differs)
    _CASES[(table, idx)] = out
    return out


def table_counts(table):
    """(cases, left out, compared cases in which the penalty changes some group's caption) of a table"""
    total = left = changed = 0
    for idx in range(len(TABLES[table][3])):
        for _, ok, differs in cases(table, idx).values():
            total += 1
            left += not ok
            changed += bool(ok and differs)
    return total, left, changed
