"""CONSTRAINED beam search (include/scnattn.h: "CONSTRAINED beam search") restated in plain torch / Python from
the header's text, not from the kernels, on the pieces of tests/beam_refs.py, tests/beam_options_refs.py and
tests/ensemble_refs.py.  The reference project has no such search: this file is what the GPU tests judge against.

    refusal(...)                           why a constrained search is refused, or None
    row_select(val, sets, reqs, mets, ..)  per row the top K ORDINARY candidates and the 4 REQUIRED candidates
    merge_banks(...)                       one step's merge of ONE image from the row candidates: banks, round-robin
    merge_state(...)                       what that merge leaves of the state arrays, met included
    search(...)                            a whole search of N images, M >= 1 members, with options and required words:
                                           results, the mask of the returned caption, and one trace entry per (step, bank)
                                           plus one per step for the picked set, in the form beam_refs.decidable takes

`search` ranks ALL candidates of a bank, not the K + 4 per row the kernels exchange: that the two agree is the top-K argument
of the header, which the GPU tests thereby check."""
import torch
import torch.nn.functional as F

import beam_options_refs as OR
import beam_refs as BR
import ensemble_refs as ER

MAX_REQUIRED, MAX_BEAM = 4, 8
NEG = -float("inf")


def popcount(m):
    return bin(int(m)).count("1")


def full_mask(req):
    return (1 << len(req)) - 1


def refusal(required, V, K, max_steps, start, end, pad, options=OR.Opts()):
    """required: one list per image.  More than 4 words, an id outside [0, V), a duplicate, <start> / <end> / <pad>, a banned
    word, K outside [1, 8], what the options refuse, and the candidate-count rule
    V - |B| - 1 - (g >= 1 ? max_steps : 0) - 4 >= K"""
    if not 1 <= K <= MAX_BEAM:
        return "beam_size"
    why = OR.refusal(options, V, K, max_steps, end)
    if why:
        return why
    B = set(options.banned_tokens)
    for req in required:
        if len(req) > MAX_REQUIRED:
            return "count"
        if any(not 0 <= w < V for w in req):
            return "vocabulary"
        if len(set(req)) != len(req):
            return "duplicate"
        if set(req) & {start, end, pad}:
            return "special"
        if set(req) & B:
            return "banned"
    if V - len(B) - 1 - (max_steps if options.no_repeat_ngram >= 1 else 0) - MAX_REQUIRED < K:
        return "candidates"
    return None


# ---- the row selection --------------------------------------------------------------------------------------------------
def row_select(val, sets, reqs, mets, K, end):
    """val [R,V] = score + log-probability; per row r: sets[r] the words the options exclude, reqs[r] the required words of
    the row's image, mets[r] the row's mask.  -> (values [R,K], words [R,K], reqv [R,4], reqi [R,4]): the top K of the
    ORDINARY candidates (not excluded, not an unmet required word, not <end> while the mask is incomplete), and entry c
    (val[r, req[c]], req[c]) when c < C, c is unmet and the options do not exclude the word, else (-inf, -1)."""
    R = val.shape[0]
    ordinary = []
    reqv = torch.full((R, MAX_REQUIRED), NEG, dtype=val.dtype)
    reqi = torch.full((R, MAX_REQUIRED), -1, dtype=torch.long)
    for r in range(R):
        req, met = list(reqs[r]), int(mets[r])
        out = set(sets[r])
        for c, w in enumerate(req):
            if not (met >> c) & 1:
                if w not in sets[r]:
                    reqv[r, c], reqi[r, c] = val[r, w], w
                out.add(w)
        if met != full_mask(req):
            out.add(end)
        ordinary.append(out)
    cv, ci = OR.row_topk_excl(val, ordinary, K)
    return cv, ci, reqv, reqi


# ---- the merge ----------------------------------------------------------------------------------------------------------
def round_robin(banks, C, kk):
    """banks[b]: a list in the search order -> the kk picks: visit b = C .. 0 again and again, the bank's next each time"""
    at = [0] * (C + 1)
    picks = []
    while len(picks) < kk:
        took = False
        for b in range(C, -1, -1):
            if len(picks) < kk and at[b] < len(banks[b]):
                picks.append(banks[b][at[b]])
                at[b] += 1
                took = True
        if not took:
            break
    return picks, at


def merge_banks(candv, candi, reqv, reqi, mets, V, C, kk):
    """candv / candi [nsrc,K], reqv / reqi [nsrc,4], mets [nsrc] of ONE image with C required words -> the kk picks
    [(value, source slot, word, the child's mask)] in the search order"""
    ns, K = candv.shape
    banks = [[] for _ in range(C + 1)]
    for j in range(ns):
        m = int(mets[j])
        for r in range(K):
            banks[popcount(m)].append((float(candv[j, r]), j * V + int(candi[j, r]), m))
        for c in range(MAX_REQUIRED):
            if int(reqi[j, c]) >= 0:
                banks[popcount(m) + 1].append((float(reqv[j, c]), j * V + int(reqi[j, c]), m | (1 << c)))
    banks = [sorted(b, key=lambda x: (-x[0], x[1])) for b in banks]
    picks, _ = round_robin(banks, C, kk)
    picks.sort(key=lambda x: (-x[0], x[1]))
    return [(v, flat // V, flat % V, m) for v, flat, m in picks]


STATE = ("open_images", "nsrc", "kk", "ncomp", "best_idx", "best_score", "scores", "comp_score", "comp_step", "comp_parent",
         "token", "parent")


def merge_state(st, candv, candi, reqv, reqi, req, N, K, V, end, t):
    """What the merge of step t leaves of the state `st` (a dict of host tensors by the names of scnattn_beam_layout, token /
    parent [T][N*K], and "met" [N*K]) given candv / candi [N*K,K], reqv / reqi [N*K,4] and the table req [N,4]: a new dict.
    <end> picks recorded as beam_merge does, the others compacted in the search order with their masks, dead slots a copy of
    slot 0 (zeros when nothing is open); a finished image untouched; open_images loses the images that closed."""
    out = {k: v.clone() for k, v in st.items()}
    for n in range(N):
        ns, kk = int(st["nsrc"][n]), int(st["kk"][n])
        if kk <= 0:
            continue
        C = int((req[n] >= 0).sum())
        r0 = n * K
        picks = merge_banks(candv[r0:r0 + ns], candi[r0:r0 + ns], reqv[r0:r0 + ns], reqi[r0:r0 + ns], st["met"][r0:r0 + ns], V,
                            C, kk)
        opened = []
        for v, j, w, m in picks:
            if w == end:
                nc = int(out["ncomp"][n])
                if nc < K:
                    out["comp_score"][r0 + nc], out["comp_step"][r0 + nc], out["comp_parent"][r0 + nc] = v, t, j
                    if int(out["best_idx"][n]) < 0 or v > float(out["best_score"][n]):
                        out["best_idx"][n], out["best_score"][n] = nc, v
                    out["ncomp"][n] = nc + 1
            else:
                opened.append((w, j, v, m))
        fill = (opened[0][0], opened[0][1], 0.0, opened[0][3]) if opened else (0, 0, 0.0, 0)
        for s, (w, p, v, m) in enumerate(opened + [fill] * (K - len(opened))):
            out["token"][t, r0 + s], out["parent"][t, r0 + s], out["scores"][r0 + s], out["met"][r0 + s] = w, p, v, m
        out["nsrc"][n] = out["kk"][n] = len(opened)
        if not opened:
            out["open_images"][0] -= 1
    return out


class ConState(BR.ImageState):
    """what the merge keeps per image: beam_refs.ImageState and the masks of the K slots"""

    def __init__(self, K):
        super().__init__(K)
        self.met = [0] * K

    def step_con(self, picks, t, end):
        tok, par = self.step([(v, j, w) for v, j, w, _ in picks], t, end)
        masks = [m for _, _, w, m in picks if w != end]
        self.met = masks + [masks[0] if masks else 0] * (self.K - len(masks))
        return tok, par


# ---- the whole search ---------------------------------------------------------------------------------------------------
def search(kinds, params_list, w, mode, k, word_map, encoder_out, tag_out, required, options=OR.Opts(), alpha_member=None,
           max_steps=BR.MAX_STEPS):
    """beam_options_refs.search with required[n], the words the caption of image n must contain.
    -> (results, traces, masks): results[n] = (out, [(sequence, score)]) as beam_refs.search returns them, out chosen by
    options.length_penalty among the finished beams -- or, when none finished, among the open beams with the largest
    popcount(met) (the higher score, then the lower slot); masks[n] = the mask of the caption returned;
    traces[n] = per step the image took part in one entry per bank that was picked from (picked flat indices j*V + v in pick
    order, their values, the bank's first picks + 1 values AFTER exclusion), then one for the picked set as it is arranged
    (its flat indices and values in the search order, the values again)."""
    from oracle import scnattn_ref as R
    mode = ER.MODES.get(mode, mode)
    M, K, V = len(kinds), k, len(word_map)
    start, end, pad = word_map["<start>"], word_map["<end>"], word_map["<pad>"]
    why = refusal(required, V, K, max_steps, start, end, pad, options)
    assert why is None, why
    N, hh, ww, E = encoder_out.shape
    assert len(required) == N
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
    st = [ConState(K) for _ in range(N)]
    hist = [[[] for _ in range(K)] for _ in range(N)]       # the words of the beam in every slot
    token, parent, alpha = [], [], []
    traces = [[] for _ in range(N)]
    for t in range(max_steps):
        if all(s.kk == 0 for s in st):
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
        scores = torch.tensor([x for s in st for x in s.scores], dtype=logits[0].dtype)
        val = scores.unsqueeze(1) + ER.combine(logits, w, mode)         # the log-sum-exp over all V words
        tok_t, par_t = [], []
        for n, s in enumerate(st):
            if s.kk == 0:                       # finished: the device leaves the zero-filled records alone
                tok_t += [0] * K
                par_t += [0] * K
                continue
            r0, ns, kk = n * K, s.nsrc, s.kk
            req = list(required[n])
            C = len(req)
            banks = [[] for _ in range(C + 1)]
            for j in range(ns):
                ex = OR.excluded(hist[n][j], t, V, end, options)
                met = s.met[j]
                a = val[r0 + j].clone()
                for cc, wd in enumerate(req):                   # the required candidates, then out of the ordinary ones
                    if not (met >> cc) & 1:
                        if wd not in ex:
                            banks[popcount(met) + 1].append((float(a[wd]), j * V + wd, met | (1 << cc)))
                        a[wd] = NEG
                if met != full_mask(req):
                    a[end] = NEG
                if ex:
                    a[sorted(ex)] = NEG
                # a bank takes at most kk picks: the row's first kk + 1 hold whatever of it is among the bank's first kk + 1
                for v in torch.sort(-a, stable=True)[1][:kk + 1].tolist():
                    if float(a[v]) > NEG:
                        banks[popcount(met)].append((float(a[v]), j * V + v, met))
            banks = [sorted(b, key=lambda x: (-x[0], x[1])) for b in banks]
            picked, at = round_robin(banks, C, kk)
            for b in range(C, -1, -1):
                if at[b]:
                    head = banks[b][:at[b] + 1]
                    traces[n].append(([f for _, f, _ in head[:at[b]]], [v for v, _, _ in head[:at[b]]], [v for v, _, _ in head]))
            picked.sort(key=lambda x: (-x[0], x[1]))
            traces[n].append(([f for _, f, _ in picked], [v for v, _, _ in picked], [v for v, _, _ in picked]))
            picks = [(v, f // V, f % V, m) for v, f, m in picked]
            tk, pr = s.step_con(picks, t, end)
            hist[n] = [hist[n][pr[j]] + [tk[j]] for j in range(K)]       # dead slots: slot 0's parent and word
            tok_t += tk
            par_t += pr
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

    out, masks = [], []
    for n, s in enumerate(st):
        done, mk = [], []
        for v, t, j in s.comp:
            words, arows = chain(n, t - 1, j)
            done.append((words + [end], arows + [(t, n * K + j)], v))
            mk.append(full_mask(required[n]))
        among = list(range(len(done)))
        i = s.best
        if not done:
            for slot in range(s.nsrc):
                words, arows = chain(n, steps - 1, slot)
                assert words[1:] == hist[n][slot]           # the history IS the parent chain
                done.append((words, arows, s.scores[slot]))
                mk.append(s.met[slot])
            most = max(popcount(m) for m in mk)
            among = [q for q in range(len(done)) if popcount(mk[q]) == most]
            sc = [done[q][2] for q in among]
            i = among[sc.index(max(sc))]
        if options.length_penalty != 0.0:
            i = among[OR.pick([(done[q][0], done[q][2]) for q in among], options.length_penalty)]
        seq, arows, _ = done[i]
        implied = sum(1 << cc for cc, wd in enumerate(required[n]) if wd in seq)
        assert mk[i] == implied, "met is not what the history implies"
        if alpha_member >= 0:
            maps = torch.cat([ones] + [alpha[t][r].view(1, hh, ww) for t, r in arows]).tolist()
            one = (seq, maps)
        else:
            one = seq
        out.append((one, [(x[0], x[2]) for x in done]))
        masks.append(mk[i])
    return out, traces, masks


def search_one(kind, Pm, k, word_map, encoder_out, tag_out, required, options=OR.Opts(), max_steps=BR.MAX_STEPS):
    """`search` for one decoder: what decoder.sample_constrained(k, required, ...) restates"""
    return search([kind], [Pm], [1.0], 0, k, word_map, encoder_out, tag_out if kind != "pure_attention" else None, required,
                  options, max_steps=max_steps)


# ---- the tables of tests/test_gpu_constrained_beam_search.py ---------------------------------------------------------------
# The inputs of the option tables (beam_options_refs.inputs: E=256, A=D=F=128, M=64, S=40, 7x7, V=1003, N=3, beams 1/3/5).
# A table is (options, ranks, [(kind, seed)]); its cases are (kind, seed, image, beam size).
# THE WORD RULE: image b requires the words at the 0-based ranks `ranks` of its own first-step distribution (the fp64
# restatement's log-probabilities of the <start> row, stable order), counted over the words that may be required at all:
# not <pad>, <start>, <end>, <unk> (banned in one table).  So every required word is reachable at step 0, and the lower
# ranks are words the plain caption would rather not use.  Ranks were chosen on the CPU so that this restatement meets the
# caps that tests/test_constrained_beam_refs.py asserts; they are the same for every image of a table.
MIN6 = OR.Opts(min_length=6)
NGRAM = OR.Opts(min_length=4, no_repeat_ngram=2, banned_tokens=(OR.UNK,))
TABLES = {
    "two_words": (OR.Opts(), (4, 11), OR.SEEDS),
    "four_words_min6": (MIN6, (3, 6, 10, 15), OR.SEEDS),
    "one_word_ngram_unk": (NGRAM, (8,), OR.SEEDS),
}
_FIRST, _CASES = {}, {}


def first_logp(kinds, params_list, w, mode, wm, enc4, tags):
    """the combined fp64 log-probabilities [N,V] of the first step (the <start> row of every image)"""
    from oracle import scnattn_ref as R
    N, hh, ww, E = enc4.shape
    enc = enc4.reshape(N, hh * ww, E)
    mean = enc.mean(1)
    logits = []
    for kind, Pm in zip(kinds, params_list):
        h = F.linear(mean, Pm["init_h.weight"], Pm["init_h.bias"])
        c = F.linear(mean, Pm["init_c.weight"], Pm["init_c.bias"])
        emb = Pm["embedding.weight"][wm["<start>"]].expand(N, -1)
        if kind != "pure_scn":
            att1 = F.linear(enc, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
            att2 = F.linear(h, Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
            e = BR.attn_scores(att1, att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                               Pm["attention.full_att.bias"], 1)["e"]
            gpre = F.linear(h, Pm["f_beta.weight"], Pm["f_beta.bias"])
            emb = torch.cat([emb, BR.attn_context(enc, e, gpre.unsqueeze(0), None, 1)["z"]], dim=1)
        if kind == "pure_attention":
            h2, _ = R.lstm_cell_forward(Pm, "decode_step.", emb, (h, c))
        else:
            h2, _ = R.scn_cell_forward(Pm, "decode_step.", emb, tags, (h, c))
        logits.append(F.linear(h2, Pm["fc.weight"], Pm["fc.bias"]))
    return ER.combine(logits, w, ER.MODES.get(mode, mode))


def order_of(logp, wm):
    """per image the words by descending log-probability (stable), the words that may not be required left out"""
    never = {wm["<pad>"], wm["<start>"], wm["<end>"], wm["<unk>"]}
    return [[v for v in row if v not in never] for row in torch.sort(-logp, dim=1, stable=True)[1].tolist()]


def first_step_order(kind, seed):
    """per image the words in the order of the first step's fp64 distribution, the words that may not be required left out"""
    if (kind, seed) not in _FIRST:
        from helpers import params_from
        d, V, enc4, tags = OR.inputs(kind, seed)
        wm = BR.word_map(V)
        logp = first_logp([kind], [params_from(d, dtype=torch.float64)], [1.0], 0, wm, enc4.double(), tags.double())
        _FIRST[(kind, seed)] = order_of(logp, wm)
    return _FIRST[(kind, seed)]


def required_words(kind, seed, ranks):
    """the word rule -> one list per image"""
    return [[row[r] for r in ranks] for row in first_step_order(kind, seed)]


def seq_of(one, kind):
    return one[0] if kind != "pure_scn" else one


def cases(table, idx):
    """cases[(image, k)] = (fp64 result (out, done), decidable, the mask of the caption, the requirement changes the caption
    and is satisfied, the required words); once per process"""
    if (table, idx) in _CASES:
        return _CASES[(table, idx)]
    from helpers import params_from
    options, ranks, rows = TABLES[table]
    kind, seed = rows[idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    req = required_words(kind, seed, ranks)
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    out = {}
    for k in BR.BEAMS:
        r64, t64, m64 = search_one(kind, P64, k, wm, enc.double(), tags.double(), req, options)
        _, t32, _ = search_one(kind, P32, k, wm, enc, tags, req, options)
        plain = OR.cases(kind, seed, options)
        for b in range(enc.shape[0]):
            seq = seq_of(r64[b][0], kind)
            satisfied = m64[b] == full_mask(req[b]) and all(wd in seq for wd in req[b])
            changed = seq != seq_of(plain[(b, k)][0][0], kind)
            out[(b, k)] = (r64[b], BR.decidable(t64[b], t32[b]), m64[b], bool(changed and satisfied), req[b])
    _CASES[(table, idx)] = out
    return out


def table_counts(table):
    """(cases, left out, compared cases in which the requirement changes the caption and is satisfied) of a table"""
    total = left = changed = 0
    for idx in range(len(TABLES[table][2])):
        for _, ok, _, ch, _ in cases(table, idx).values():
            total += 1
            left += not ok
            changed += bool(ok and ch)
    return total, left, changed


# ---- the two-member ensemble: the inputs and options of beam_options_refs.ENSEMBLE, the words at ranks (4, 11) -------------
ENSEMBLE_RANKS = (4, 11)
_ENS = {}


def ensemble_cases(mode):
    """cases[(image, k)] = (fp64 result, decidable, mask, the requirement changes the caption and is satisfied, the words);
    "required": the lists; once per process"""
    if mode in _ENS:
        return _ENS[mode]
    from helpers import params_from
    I, o = OR.ensemble_inputs(), OR.ENSEMBLE[2]
    wm = BR.word_map(I["V"])
    P64 = [params_from(d, dtype=torch.float64) for d in I["dicts"]]
    P32 = [params_from(d, dtype=torch.float32) for d in I["dicts"]]
    enc, tags = I["enc"], I["tags"]
    order = order_of(first_logp(I["kinds"], P64, I["w"], mode, wm, enc.double(), tags.double()), wm)
    req = [[row[r] for r in ENSEMBLE_RANKS] for row in order]
    plain = OR.ensemble_cases(mode)
    out = {"required": req}
    for k in BR.BEAMS:
        r64, t64, m64 = search(I["kinds"], P64, I["w"], mode, k, wm, enc.double(), tags.double(), req, o)
        _, t32, _ = search(I["kinds"], P32, I["w"], mode, k, wm, enc, tags, req, o)
        for b in range(enc.shape[0]):
            seq = r64[b][0][0]
            ok = m64[b] == full_mask(req[b])
            out[(b, k)] = (r64[b], BR.decidable(t64[b], t32[b]), m64[b], bool(ok and seq != plain[(b, k)][0][0][0]), req[b])
    _ENS[mode] = out
    return out
