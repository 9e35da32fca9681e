"""The search OPTIONS of the batched beam search restated in plain torch / Python (include/scnattn.h: "search OPTIONS";
DESIGN.md 5n), from the pieces of tests/beam_refs.py and tests/ensemble_refs.py and written from the header's text, not from
the kernels.  The reference project has no such options: this file is what the GPU tests judge against.

    excluded(hist, t, V, end, options)     the words candidate (j, .) may not pick at 0-based step t, hist = the words the
                                           beam in slot j has emitted (at least t of them; <start> is not among them)
    row_topk_excl(val, sets, K)            per row the top K of val under the search order with the row's set left out
    search(...)                            a whole search of N images, M >= 1 members, with options: results in the form of
                                           beam_refs.search plus one trace per image in the form beam_refs.decidable takes
    pick(done, alpha)                      the length-normalised choice among (sequence, score) pairs

`Opts` is this file's own statement of the options (the tests hand the same numbers to models.decoders.SearchOptions)."""
import collections

import torch
import torch.nn.functional as F

import beam_refs as BR
import ensemble_refs as ER

Opts = collections.namedtuple("Opts", "min_length no_repeat_ngram banned_tokens length_penalty", defaults=(0, 0, (), 0.0))
MAX_BANNED, MAX_NGRAM = 64, 8


# ---- the rules ----------------------------------------------------------------------------------------------------------
def excluded(hist, t, V, end, options):
    """-> the set of excluded words.  1. banned; 2. <end> while t < min_length; 3. g = no_repeat_ngram >= 1 and t >= g: every
    w_{i+g-1} with 0 <= i <= t-g and w_i .. w_{i+g-2} == w_{t-g+1} .. w_{t-1} (g = 1: every word of the history)."""
    w = list(hist[:t])
    assert len(w) == t
    out = {int(b) for b in options.banned_tokens}
    if t < options.min_length:
        out.add(end)
    g = options.no_repeat_ngram
    if g >= 1 and t >= g:
        tail = w[t - g + 1:t]
        for i in range(t - g + 1):
            if w[i:i + g - 1] == tail:
                out.add(w[i + g - 1])
    assert all(0 <= v < V for v in out)
    return out


def refusal(options, V, K, max_steps, end):
    """why a search with these options is refused, or None: the ranges, a banned <end>, and the candidate-count rule
    V - |B| - 1 - (g >= 1 ? max_steps : 0) >= K"""
    g, B = options.no_repeat_ngram, set(options.banned_tokens)
    if not 0 <= options.min_length <= max_steps - 1:
        return "min_length"
    if not 0 <= g <= MAX_NGRAM:
        return "no_repeat_ngram"
    if len(B) > MAX_BANNED or end in B or any(not 0 <= b < V for b in B):
        return "banned"
    if V - len(B) - 1 - (max_steps if g >= 1 else 0) < K:
        return "candidates"
    return None


def row_topk_excl(val, sets, K):
    """val [R,V] = score + log-probability (NOT renormalised); sets: R sets of excluded words -> (values [R,K], words [R,K]):
    per row the top K of the remaining candidates, the lower word first among equal values"""
    v = val.clone()
    for r, s in enumerate(sets):
        if s:
            v[r, sorted(s)] = -float("inf")
    order = torch.sort(-v, dim=1, stable=True)[1][:, :K]
    got = v.gather(1, order)
    assert bool(torch.isfinite(got).all()), "a row offers fewer than K candidates"
    return got, order


def pick(done, alpha):
    """done: [(sequence with <start>, score)] in completion order -> index of the first maximum of score / L**alpha,
    L = len(sequence) - 1 (the decoded tokens, <end> included)"""
    norm = [float(s) / float(len(seq) - 1) ** alpha for seq, s in done]
    return norm.index(max(norm))


# ---- the whole search ---------------------------------------------------------------------------------------------------
def search(kinds, params_list, w, mode, k, word_map, encoder_out, tag_out, options=Opts(), alpha_member=None,
           max_steps=BR.MAX_STEPS):
    """beam_refs.search for M = len(kinds) members under one search state (ensemble_refs.combine; M = 1, w = [1.0], mode 0
    is the single decoder) with `options`.  encoder_out [N,h,w,E], tag_out [N,S] or None.
    -> (results, traces): results[n] = (out, [(sequence, score)]) as beam_refs.search returns them, out chosen by
    options.length_penalty; traces[n] = per step the image took part in (picked flat indices j*V + v, picked values, the top
    kk+1 values of the step's candidates AFTER exclusion)."""
    from oracle import scnattn_ref as R
    mode = ER.MODES.get(mode, mode)
    M, K, V = len(kinds), k, len(word_map)
    start, end = word_map["<start>"], word_map["<end>"]
    assert refusal(options, V, K, max_steps, end) is None, refusal(options, V, K, max_steps, end)
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
    st = [BR.ImageState(K) for _ in range(N)]
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
            sets = [excluded(hist[n][j], t, V, end, options) for j in range(ns)]
            cv, ci = row_topk_excl(val[r0:r0 + ns], sets, K)
            picks = BR.merge(cv, ci, V, kk)
            cand = val[r0:r0 + ns].clone()
            for j, ex in enumerate(sets):
                if ex:
                    cand[j, sorted(ex)] = -float("inf")
            cand = cand.reshape(-1)
            more = torch.sort(cand, descending=True)[0][:min(kk + 1, int(torch.isfinite(cand).sum()))]
            traces[n].append(([j * V + wd for _, j, wd in picks], [v for v, _, _ in picks], more.tolist()))
            tk, pr = s.step(picks, t, end)
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

    out = []
    for n, s in enumerate(st):
        done = []
        for v, t, j in s.comp:
            words, arows = chain(n, t - 1, j)
            done.append((words + [end], arows + [(t, n * K + j)], v))
        i = s.best
        if not done:
            for slot in range(s.nsrc):
                words, arows = chain(n, steps - 1, slot)
                assert words[1:] == hist[n][slot]           # the history IS the parent chain
                done.append((words, arows, s.scores[slot]))
            sc = [x[2] for x in done]
            i = sc.index(max(sc))
        if options.length_penalty != 0.0:
            i = pick([(x[0], x[2]) for x in done], options.length_penalty)
        seq, arows, _ = done[i]
        if alpha_member >= 0:
            maps = torch.cat([ones] + [alpha[t][r].view(1, hh, ww) for t, r in arows]).tolist()
            one = (seq, maps)
        else:
            one = seq
        out.append((one, [(x[0], x[2]) for x in done]))
    return out, traces


def search_one(kind, Pm, k, word_map, encoder_out, tag_out, options=Opts(), max_steps=BR.MAX_STEPS):
    """`search` for one decoder: what decoder.sample_batch(..., options=...) restates"""
    return search([kind], [Pm], [1.0], 0, k, word_map, encoder_out, tag_out if kind != "pure_attention" else None, options,
                  max_steps=max_steps)


# ---- the tables of tests/test_gpu_beam_options_search.py ----------------------------------------------------------------
# The shapes and seeds of test_gpu_beam_search.test_vector_width_shapes_vs_oracle (E=256, A=D=F=128, M=64, S=40, 7x7,
# V=1003, N=3, beams 1/3/5).  A table is a list of (kind, seed, options); its cases are (kind, seed, image, beam size).
UNK = 1003 - 3
SEEDS = [("attention_scn", 2), ("attention_scn", 6), ("pure_scn", 78)]
TABLES = {
    "min8_ngram": [("attention_scn", 2, Opts(min_length=8, no_repeat_ngram=2)),
                   ("attention_scn", 6, Opts(min_length=8, no_repeat_ngram=2)),
                   ("pure_scn", 78, Opts(min_length=8, no_repeat_ngram=4))],
    "min6_unigram_unk": [(kind, seed, Opts(min_length=6, no_repeat_ngram=1, banned_tokens=(UNK,))) for kind, seed in SEEDS],
    "min3_trigram": [(kind, seed, Opts(min_length=3, no_repeat_ngram=3)) for kind, seed in SEEDS],
}
_INPUTS, _CASES = {}, {}


def inputs(kind, seed):
    """the decoder weights and the three images of that test, from its own recipe"""
    if (kind, seed) not in _INPUTS:
        from test_gpu_beam_search import _uniform_params
        g = torch.Generator().manual_seed(seed)
        d, V, E, S = _uniform_params(kind, g)
        enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
        _INPUTS[(kind, seed)] = (d, V, enc, tags)
    return _INPUTS[(kind, seed)]


def _seq(one, kind):
    return one[0] if kind != "pure_scn" else one


def cases(kind, seed, options):
    """cases[(image, k)] = (fp64 result (out, done), decidable, the caption differs from the same options with
    no_repeat_ngram = 0); once per process"""
    key = (kind, seed, options)
    if key in _CASES:
        return _CASES[key]
    from helpers import params_from
    d, V, enc, tags = inputs(kind, seed)
    wm = BR.word_map(V)
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    out = {}
    for k in BR.BEAMS:
        r64, t64 = search_one(kind, P64, k, wm, enc.double(), tags.double(), options)
        _, t32 = search_one(kind, P32, k, wm, enc, tags, options)
        plain = None
        if options.no_repeat_ngram:
            plain, _ = search_one(kind, P64, k, wm, enc.double(), tags.double(), options._replace(no_repeat_ngram=0))
        for b in range(enc.shape[0]):
            differs = plain is not None and _seq(plain[b][0], kind) != _seq(r64[b][0], kind)
            out[(b, k)] = (r64[b], BR.decidable(t64[b], t32[b]), differs)
    _CASES[key] = out
    return out


# ---- the two-member ensemble of that file: the recipe of ensemble_refs.table (seed 3, "A+S") -----------------------------
ENSEMBLE = (3, "A+S", Opts(min_length=6, no_repeat_ngram=2))
_ENS = {}


def ensemble_inputs():
    """-> dict(kinds, weights, w, dicts, V, enc, tags): members drawn in order from one generator, then enc and tags, then
    fc.bias[<end>] += ensemble_refs.END_BIAS for every member"""
    if "in" not in _ENS:
        seed, name, _ = ENSEMBLE
        kinds, weights = ER.ENSEMBLES[name]
        g = torch.Generator().manual_seed(seed)
        dicts = []
        for kind in kinds:
            d, V, E, S = ER.uniform_params(kind, g)
            dicts.append(d)
        enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
        for d in dicts:
            d["p.fc.bias"][V - 1] += ER.END_BIAS
        _ENS["in"] = dict(kinds=kinds, weights=weights, w=ER.member_weights(weights, len(kinds)), dicts=dicts, V=V, enc=enc,
                          tags=tags)
    return _ENS["in"]


def ensemble_cases(mode):
    """cases[(image, k)] = (fp64 result, decidable, the caption differs from no_repeat_ngram = 0); once per process"""
    if mode in _ENS:
        return _ENS[mode]
    from helpers import params_from
    I, o = ensemble_inputs(), ENSEMBLE[2]
    wm = BR.word_map(I["V"])
    P64 = [params_from(d, dtype=torch.float64) for d in I["dicts"]]
    P32 = [params_from(d, dtype=torch.float32) for d in I["dicts"]]
    enc, tags = I["enc"], I["tags"]
    out = {}
    for k in BR.BEAMS:
        r64, t64 = search(I["kinds"], P64, I["w"], mode, k, wm, enc.double(), tags.double(), o)
        _, t32 = search(I["kinds"], P32, I["w"], mode, k, wm, enc, tags, o)
        plain, _ = search(I["kinds"], P64, I["w"], mode, k, wm, enc.double(), tags.double(), o._replace(no_repeat_ngram=0))
        for b in range(enc.shape[0]):
            out[(b, k)] = (r64[b], BR.decidable(t64[b], t32[b]), plain[b][0][0] != r64[b][0][0])
    _ENS[mode] = out
    return out


def table_counts(name):
    """(cases, left out, compared cases whose caption the n-gram rule changes) of a table"""
    total = left = changed = 0
    for kind, seed, options in TABLES[name]:
        for _, ok, differs in cases(kind, seed, options).values():
            total += 1
            left += not ok
            changed += bool(ok and differs)
    return total, left, changed
