"""Plain-torch references of the ensemble beam search (csrc/beam.hip: beam_row_topk_ens; csrc/beam_search.cpp:
scnattn_ensemble_*), written from the description in include/scnattn.h, not from the kernels.  Every function computes in
the dtype of its inputs (fp64: the reference).  M decoders share one search state; with l_mv = x_mv - logsumexp(x_m) the
candidates of a step are ranked by score + c_v,

    mode 0 ("logprob")   c_v = sum_m w_m l_mv                                  summed in member order
    mode 1 ("prob")      c_v = a_v + log(sum_m w_m exp(l_mv - a_v)),  a_v = max_m l_mv

in the search order of tests/beam_refs.py (value descending, flat index ascending among equal values).  `search` assembles
a whole search of ONE image from beam_refs' pieces and oracle/scnattn_ref's cells and records, per step, what the
decidability rule of the GPU tests needs (beam_refs.decidable).

THE BOUND of the fp32 kernel (u = 2^-24, V words, M members; `value_bounds` below).
  Member.  tests/test_gpu_beam_kernels.py::_value_bound gives, for score + (x - lse) in fp32,
      u ((V + 8) + 2 (|score| + |x| + |lse|)):
  V positive terms in the sum of exponentials, 2-ulp expf, three roundings.  Without the score that is the bound of one
  member's l_mv:   b_m = u ((V + 8) + 2 (|x_mv| + |lse_m|)).
  Mode 0.  c = fl(w_0 l_0) followed by M - 1 fused multiply-adds: the errors of the l_m pass through with their weights,
  sum_m w_m b_m, and each of the M operations rounds once, relative u on a partial sum that is at most sum_m w_m |l_m| in
  magnitude:   B0 = sum_m w_m b_m + M u sum_m w_m |l_mv|.
  Mode 1.  c = log(sum_m w_m exp(l_m)) whatever `a` is, so an error in `a` itself costs nothing; dc/dl_m = p_m, the
  members' shares of the mean, which are positive and sum to 1.  Hence the l_m (error b_m) and the rounded differences
  d_m = l_m - a (u |d_m|) cost at most max_m (b_m + u |d_m|).  expf is good to 2 ulp (relative 2 u on every term, so on s),
  the M products / fused multiply-adds of the sum round once each on positive terms (relative M u on s, doubled: 2 M u, to
  cover the first-order treatment), a term flushed to zero changes s by less than 2^-126 / min(w) (one more u); a relative
  error of s is an absolute error of log s; logf is good to 2 ulp (2 u |log s|) and a + log s rounds once (u |c|):
               B1 = max_m (b_m + u |d_m|) + (2 M + 3) u + 2 u |log s| + u |c|.
  Value.  score + c rounds once, u |score + c| <= u (|score| + |c|), doubled as _value_bound doubles its magnitudes:
               |d value| <= B + 2 u (|score| + |c|).
The weights are the fp32 numbers the kernel is given (normalised in fp64, then rounded), taken as exact by both sides."""
import collections

import torch
import torch.nn.functional as F

import beam_refs as BR

U = 2.0 ** -24
MODES = {"logprob": 0, "prob": 1}


def member_weights(weights, M):
    """what scnattn.functional.normalise_member_weights does, restated: fp64 normalisation, then one rounding to fp32"""
    w = torch.tensor([1.0] * M if weights is None else [float(x) for x in weights], dtype=torch.float64)
    return [float(x) for x in (w / w.sum()).float()]


def log_probs(logits_list):
    return [x - torch.logsumexp(x, dim=1, keepdim=True) for x in logits_list]


def combine(logits_list, w, mode):
    """logits_list: M tensors [R,V]; w: M floats -> c [R,V]"""
    ls = log_probs(logits_list)
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


def row_topk_ens(logits_list, w, mode, scores, K):
    """-> (values [R,K], words [R,K], c [R,V]): per row the top K of score + c_v, the lower word first among equal values"""
    c = combine(logits_list, w, mode)
    val = scores.unsqueeze(1) + c
    order = torch.sort(-val, dim=1, stable=True)[1][:, :K]
    return val.gather(1, order), order, c


def value_bounds(logits_list, w, mode, scores):
    """(bound of c_v, bound of score + c_v) per element [R,V], from fp64 inputs: the derivation at the top of this file"""
    M, V = len(logits_list), logits_list[0].shape[1]
    xs = [x.double() for x in logits_list]
    lse = [torch.logsumexp(x, dim=1, keepdim=True) for x in xs]
    ls = [x - s for x, s in zip(xs, lse)]
    b = [U * ((V + 8) + 2 * (x.abs() + s.abs())) for x, s in zip(xs, lse)]
    c = combine(xs, w, mode)
    if mode == 0:
        bc = sum(wm * bm for wm, bm in zip(w, b)) + M * U * sum(wm * l.abs() for wm, l in zip(w, ls))
    else:
        a = torch.stack(ls).max(0)[0]
        worst = torch.stack([bm + U * (l - a).abs() for bm, l in zip(b, ls)]).max(0)[0]
        bc = worst + (2 * M + 3) * U + 2 * U * (c - a).abs() + U * c.abs()
    return bc, bc + 2 * U * (scores.double().abs().unsqueeze(1) + c.abs())


# ---- the whole search of ONE image ------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "done seq alphas trace completed")


def search(kinds, params_list, w, mode, k, word_map, enc, tags, alpha_member=None, max_steps=BR.MAX_STEPS):
    """One image: enc [1,h,w,E], tags [1,S] (or None when no member uses tags); kinds / params_list one entry per member.
    -> Result(done = [(sequence, score)] in completion order (the open beams in slot order where nothing completed),
    seq = the chosen sequence, alphas = the maps of alpha_member along it (None: no member with attention; default the
    first one), trace = per step (picked flat indices j*V + v, picked values, the top kk+1 values of the step's
    candidates), completed = whether anything reached <end>)."""
    from oracle import scnattn_ref as R
    mode = MODES.get(mode, mode)
    M, K, V = len(kinds), k, len(word_map)
    start, end = word_map["<start>"], word_map["<end>"]
    _, hh, ww, E = enc.shape
    encf = enc.reshape(1, hh * ww, E)
    att = [kind != "pure_scn" for kind in kinds]
    if alpha_member is None:
        alpha_member = att.index(True) if True in att else -1
    mean = encf.mean(1)
    h, c, emb, att1 = [], [], [], []
    for kind, Pm in zip(kinds, params_list):
        h.append(F.linear(mean, Pm["init_h.weight"], Pm["init_h.bias"]).repeat_interleave(K, 0))
        c.append(F.linear(mean, Pm["init_c.weight"], Pm["init_c.bias"]).repeat_interleave(K, 0))
        emb.append(Pm["embedding.weight"][start].expand(K, -1))
        att1.append(F.linear(encf, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
                    if kind != "pure_scn" else None)
    tagsK = tags.repeat_interleave(K, 0) if tags is not None else None
    st = BR.ImageState(K)
    token, parent, alpha, trace = [], [], [], []
    for t in range(max_steps):
        if st.kk == 0:
            break
        logits, h2, c2 = [], [], []
        for m, (kind, Pm) in enumerate(zip(kinds, params_list)):
            if att[m]:
                att2 = F.linear(h[m], Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
                e = BR.attn_scores(att1[m], att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                                   Pm["attention.full_att.bias"], K)["e"]
                gpre = F.linear(h[m], Pm["f_beta.weight"], Pm["f_beta.bias"])
                ctx = BR.attn_context(encf, e, gpre.unsqueeze(0), None, K)
                if m == alpha_member:
                    alpha.append(ctx["alpha"])
                step_in = torch.cat([emb[m], ctx["z"]], dim=1)
            else:
                step_in = emb[m]
            if kind == "pure_attention":
                hm, cm = R.lstm_cell_forward(Pm, "decode_step.", step_in, (h[m], c[m]))
            else:
                hm, cm = R.scn_cell_forward(Pm, "decode_step.", step_in, tagsK, (h[m], c[m]))
            h2.append(hm)
            c2.append(cm)
            logits.append(F.linear(hm, Pm["fc.weight"], Pm["fc.bias"]))
        scores = torch.tensor(st.scores, dtype=logits[0].dtype)
        cv, ci, cmat = row_topk_ens(logits, w, mode, scores, K)
        ns, kk = st.nsrc, st.kk
        picks = BR.merge(cv[:ns], ci[:ns], V, kk)
        cand = (scores[:ns].unsqueeze(1) + cmat[:ns]).reshape(-1)
        more = torch.sort(cand, descending=True)[0][:min(kk + 1, cand.numel())]
        trace.append(([j * V + wd for _, j, wd in picks], [v for v, _, _ in picks], more.tolist()))
        tok_t, par_t = st.step(picks, t, end)
        token.append(tok_t)
        parent.append(par_t)
        for m, Pm in enumerate(params_list):
            h[m], c[m], emb[m] = BR.advance(h2[m], c2[m], par_t, tok_t, Pm["embedding.weight"], K)
    steps = len(token)

    def chain(t, slot):
        words, arows = [], []
        while t >= 0:
            words.append(token[t][slot])
            slot = parent[t][slot]
            arows.append((t, slot))
            t -= 1
        return [start] + words[::-1], arows[::-1]

    done = []
    for v, t, j in st.comp:
        words, arows = chain(t - 1, j)
        done.append((words + [end], arows + [(t, j)], v))
    completed = bool(done)
    i = st.best
    if not done:
        for slot in range(st.nsrc):
            words, arows = chain(steps - 1, slot)
            done.append((words, arows, st.scores[slot]))
        sc = [x[2] for x in done]
        i = sc.index(max(sc))
    seq, arows, _ = done[i]
    maps = None
    if alpha_member >= 0:
        ones = torch.ones(1, hh, ww, dtype=enc.dtype)
        maps = torch.cat([ones] + [alpha[t][r].view(1, hh, ww) for t, r in arows]).tolist()
    return Result([(x[0], x[2]) for x in done], seq, maps, trace, completed)


# ---- the ensembles of tests/test_gpu_ensemble_search.py ---------------------------------------------------------------
def uniform_params(kind, g):
    """the `_uniform_params` recipe of tests/test_gpu_beam_search.py (E=256, A=128, D=F=128, M=64, S=40, V=1003) without the
    <end> bias, extended to pure_attention: weight_ih [4D, M+E] with r = (M+E)^-1/2, weight_hh [4D, D] with r = D^-1/2,
    both biases with r = 0.1, then the attention block"""
    E, A, D, Fd, M, S, V = 256, 128, 128, 128, 64, 40, 1003

    def u(*shape, r):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * r).numpy()

    d = {"p.embedding.weight": u(V, M, r=1.0), "p.fc.weight": u(V, D, r=1.0), "p.fc.bias": u(V, r=0.1),
         "p.init_h.weight": u(D, E, r=E ** -0.5), "p.init_h.bias": u(D, r=0.1),
         "p.init_c.weight": u(D, E, r=E ** -0.5), "p.init_c.bias": u(D, r=0.1)}
    if kind == "pure_attention":
        d.update({"p.decode_step.weight_ih": u(4 * D, M + E, r=(M + E) ** -0.5), "p.decode_step.weight_hh": u(4 * D, D, r=D ** -0.5),
                  "p.decode_step.bias_ih": u(4 * D, r=0.1), "p.decode_step.bias_hh": u(4 * D, r=0.1)})
    else:
        I = M + E if kind == "attention_scn" else M
        d.update({"p.decode_step.weight_ia": u(I, 4 * Fd, r=I ** -0.5), "p.decode_step.weight_ib": u(S, 4 * Fd, r=1.0),
                  "p.decode_step.weight_ic": u(D, 4 * Fd, r=Fd ** -0.5), "p.decode_step.weight_ha": u(D, 4 * Fd, r=D ** -0.5),
                  "p.decode_step.weight_hb": u(S, 4 * Fd, r=1.0), "p.decode_step.weight_hc": u(D, 4 * Fd, r=Fd ** -0.5),
                  "p.decode_step.bias_ih": u(4 * D, r=0.1), "p.decode_step.bias_hh": u(4 * D, r=0.1)})
    if kind != "pure_scn":
        d.update({"p.attention.encoder_att.weight": u(A, E, r=E ** -0.5), "p.attention.encoder_att.bias": u(A, r=0.1),
                  "p.attention.decoder_att.weight": u(A, D, r=D ** -0.5), "p.attention.decoder_att.bias": u(A, r=0.1),
                  "p.attention.full_att.weight": u(1, A, r=1.0), "p.attention.full_att.bias": u(1, r=0.1),
                  "p.f_beta.weight": u(E, D, r=D ** -0.5), "p.f_beta.bias": u(E, r=0.1)})
    return d, V, E, S


END_BIAS = 1.4
ENSEMBLES = {"A+S": (("attention_scn", "pure_scn"), (0.625, 0.375)),
             "A+S+P": (("attention_scn", "pure_scn", "pure_attention"), (0.5, 0.25, 0.25))}
_TABLES = {}


def table(seed, name):
    """The members, inputs and fp64 cases of one table: members drawn in order from ONE generator seeded with `seed`, then
    enc = rand(3,7,7,E) and tags = rand(3,S) from the same generator, then fc.bias[<end>] += 1.4 for every member.
    -> dict(kinds, w, dicts, V, enc, tags, cases), cases[(mode, image, k)] = (fp64 Result, decidable); once per process."""
    from helpers import params_from
    if (seed, name) in _TABLES:
        return _TABLES[(seed, name)]
    kinds, weights = ENSEMBLES[name]
    g = torch.Generator().manual_seed(seed)
    dicts = []
    for kind in kinds:
        d, V, E, S = uniform_params(kind, g)
        dicts.append(d)
    N = 3
    enc, tags = torch.rand(N, 7, 7, E, generator=g), torch.rand(N, S, generator=g)
    for d in dicts:
        d["p.fc.bias"][V - 1] += END_BIAS
    w = member_weights(weights, len(kinds))
    wm = BR.word_map(V)
    P64 = [params_from(d, dtype=torch.float64) for d in dicts]
    P32 = [params_from(d, dtype=torch.float32) for d in dicts]
    cases = {}
    for mode in (0, 1):
        for b in range(N):
            for k in BR.BEAMS:
                r64 = search(kinds, P64, w, mode, k, wm, enc[b:b + 1].double(), tags[b:b + 1].double())
                r32 = search(kinds, P32, w, mode, k, wm, enc[b:b + 1], tags[b:b + 1])
                cases[(mode, b, k)] = (r64, BR.decidable(r64.trace, r32.trace))
    out = dict(kinds=kinds, w=w, weights=weights, dicts=dicts, V=V, enc=enc, tags=tags, cases=cases)
    _TABLES[(seed, name)] = out
    return out
