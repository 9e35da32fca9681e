"""Plain-torch references of the batched beam search (csrc/beam.hip, `scnattn_beam_*` of include/scnattn.h), written from
the header's description, not from the kernels: K slots per image, rows n*K + j, `nsrc` live source beams and `kk` beams
still to fill per image, candidates ordered by (value descending, flat index j*V + v ascending).  Every function computes
in the dtype of its inputs (fp64: the reference).  `search` assembles a whole search from them, `trace_oracle` runs
oracle/beam_ref.beam_search and records what its `topk` calls saw (the decidability rule of the GPU tests).

tests/test_beam_refs.py pins the pieces against oracle/scnattn_ref.attention_forward / F.log_softmax / topk and `search`
against oracle/beam_ref.beam_search."""
from unittest import mock

import torch
import torch.nn.functional as F

import decoder_kernel_refs as KR

MAX_STEPS = 51      # the reference leaves its loop when `step > 50` holds after a step


# ---- kernels 1 and 2: the K rows of image n attend over att1[n] / enc[n] ----------------------------------------------
def attn_scores(att1, att2_slabs, dec_bias, w, b0, K):
    """att1 [N,P,A]; att2_slabs [n,N*K,A] -> the dict of decoder_kernel_refs.attn_scores over the N*K rows"""
    return KR.attn_scores(att1.repeat_interleave(K, 0), att2_slabs, dec_bias, w, b0)


def attn_context(enc, e, gpre_slabs, gate_bias, K):
    """enc [N,P,E]; e [N*K,P]; gpre_slabs [n,N*K,E] or None -> alpha, awe, z over the N*K rows"""
    return KR.attn_context(enc.repeat_interleave(K, 0), e, gpre_slabs, gate_bias)


# ---- kernel 3 ---------------------------------------------------------------------------------------------------------
def ordered(values, flat):
    """positions of the candidates in search order: value descending, flat index ascending among equal values"""
    return sorted(range(len(values)), key=lambda i: (-float(values[i]), int(flat[i])))


def row_topk(logits, scores, K):
    """logits [R,V]; scores [R] -> (values [R,K], words [R,K], lse [R]): per row the top K of score + logit - lse"""
    lse = torch.logsumexp(logits, dim=1)
    val = scores.unsqueeze(1) + (logits - lse.unsqueeze(1))
    order = torch.sort(-val, dim=1, stable=True)[1][:, :K]        # stable: the lower word first among equal values
    return val.gather(1, order), order, lse


# ---- kernel 4 ---------------------------------------------------------------------------------------------------------
def merge(candv, candi, V, kk):
    """candv / candi [nsrc,K] of ONE image -> the kk picks [(value, source slot, word)] in rank order"""
    ns, K = candv.shape
    vals = [float(candv[j, r]) for j in range(ns) for r in range(K)]
    flat = [j * V + int(candi[j, r]) for j in range(ns) for r in range(K)]
    return [(vals[i], flat[i] // V, flat[i] % V) for i in ordered(vals, flat)[:kk]]


class ImageState:
    """what beam_merge keeps per image"""

    def __init__(self, K):
        self.K, self.nsrc, self.kk = K, 1, K
        self.scores = [0.0] * K
        self.comp = []                  # (score, step, source slot) in completion order
        self.best = -1                  # index into comp, replaced on strictly greater

    def step(self, picks, t, end):
        """-> (token, parent) of the K slots after step t: non-<end> picks compacted in rank order, dead slots a copy of
        slot 0 (zeros when nothing stays open)"""
        tok, par, sc = [], [], []
        for v, j, w in picks:
            if w == end:
                self.comp.append((v, t, j))
                if self.best < 0 or v > self.comp[self.best][0]:
                    self.best = len(self.comp) - 1
            else:
                tok.append(w)
                par.append(j)
                sc.append(v)
        n = len(tok)
        self.nsrc = self.kk = n
        self.scores = sc + [0.0] * (self.K - n)
        return tok + [tok[0] if n else 0] * (self.K - n), par + [par[0] if n else 0] * (self.K - n)


# ---- kernel 5 ---------------------------------------------------------------------------------------------------------
def advance(h, c, parent_t, token_t, table, K):
    """rows n*K + s take h / c of row n*K + parent_t and the embedding of token_t"""
    R = h.shape[0]
    src = (torch.arange(R) // K) * K + torch.as_tensor(parent_t)
    return h[src], c[src], table[torch.as_tensor(token_t)]


# ---- the whole search -------------------------------------------------------------------------------------------------
def search(kind, Pm, k, word_map, encoder_out, tag_out, max_steps=MAX_STEPS):
    """N images at once from the pieces above -> per image (out, [(sequence, score)]) as
    oracle/beam_ref.beam_search(..., return_all=True) returns them, with this build's fallback (best open beam) where the
    oracle raises.  encoder_out [N,h,w,E], tag_out [N,S] or None."""
    from oracle import scnattn_ref as R
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    K, V = k, len(word_map)
    start, end = word_map["<start>"], word_map["<end>"]
    N, hh, ww, E = encoder_out.shape
    enc = encoder_out.reshape(N, hh * ww, E)
    rows = N * K
    mean = enc.mean(1)
    h = F.linear(mean, Pm["init_h.weight"], Pm["init_h.bias"]).repeat_interleave(K, 0)
    c = F.linear(mean, Pm["init_c.weight"], Pm["init_c.bias"]).repeat_interleave(K, 0)
    tags = tag_out.repeat_interleave(K, 0) if use_tags else None
    emb = Pm["embedding.weight"][start].expand(rows, -1)
    if use_att:
        att1 = F.linear(enc, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
    st = [ImageState(K) for _ in range(N)]
    token, parent, alpha = [], [], []
    for t in range(max_steps):
        if all(s.kk == 0 for s in st):
            break
        if use_att:
            att2 = F.linear(h, Pm["attention.decoder_att.weight"], Pm["attention.decoder_att.bias"])
            e = attn_scores(att1, att2.unsqueeze(0), None, Pm["attention.full_att.weight"].reshape(-1),
                            Pm["attention.full_att.bias"], K)["e"]
            gpre = F.linear(h, Pm["f_beta.weight"], Pm["f_beta.bias"])
            ctx = attn_context(enc, e, gpre.unsqueeze(0), None, K)
            alpha.append(ctx["alpha"])
            step_in = torch.cat([emb, ctx["z"]], dim=1)
        else:
            step_in = emb
        if kind == "pure_attention":
            h2, c2 = R.lstm_cell_forward(Pm, "decode_step.", step_in, (h, c))
        else:
            h2, c2 = R.scn_cell_forward(Pm, "decode_step.", step_in, tags, (h, c))
        logits = F.linear(h2, Pm["fc.weight"], Pm["fc.bias"])
        scores = torch.tensor([x for s in st for x in s.scores], dtype=logits.dtype)
        cv, ci, _ = row_topk(logits, scores, K)
        tok_t, par_t = [], []
        for n, s in enumerate(st):
            if s.kk == 0:                       # finished: the device leaves the zero-filled records alone
                tok_t += [0] * K
                par_t += [0] * K
                continue
            r0 = n * K
            tk, pr = s.step(merge(cv[r0:r0 + s.nsrc], ci[r0:r0 + s.nsrc], V, s.kk), t, end)
            tok_t += tk
            par_t += pr
        token.append(tok_t)
        parent.append(par_t)
        h, c, emb = advance(h2, c2, par_t, tok_t, Pm["embedding.weight"], K)
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
                done.append((words, arows, s.scores[slot]))
            sc = [x[2] for x in done]
            i = sc.index(max(sc))
        seq, arows, _ = done[i]
        if use_att:
            maps = torch.cat([ones] + [alpha[t][r].view(1, hh, ww) for t, r in arows]).tolist()
            one = (seq, maps)
        else:
            one = seq
        out.append((one, [(x[0], x[2]) for x in done]))
    return out


# ---- the oracle, watched ----------------------------------------------------------------------------------------------
def trace_oracle(kind, Pm, k, word_map, encoder_out, tag_out):
    """oracle/beam_ref.beam_search on ONE image, with every `topk` call of the search recorded:
    -> (result or None when the oracle raises ValueError (nothing completed), [(picked flat indices, picked values,
    the top len+1 values of that step's candidates)])."""
    from oracle import beam_ref as BR
    trace = []
    real = torch.Tensor.topk

    def spy(self, kk, *a, **kw):
        vals, idx = real(self, kk, *a, **kw)
        more = real(self.reshape(-1), min(kk + 1, self.numel()))[0]
        trace.append((idx.tolist(), vals.tolist(), more.tolist()))
        return vals, idx

    with mock.patch.object(torch.Tensor, "topk", spy):
        try:
            res = BR.beam_search(kind, Pm, k, word_map, encoder_out, tag_out, return_all=True)
        except ValueError:
            res = None
    return res, trace


def decidable(trace64, trace32):
    """The rule of tests/test_gpu_beam_search.py: (1) the fp32 oracle picks the same indices as the fp64 oracle at every
    step; (2) every fp64 gap between consecutive entries of each step's top k+1 is at least
    max(8 x the worst fp32-vs-fp64 running-score difference of the case, 1e-5)."""
    if len(trace64) != len(trace32) or any(a[0] != b[0] for a, b in zip(trace64, trace32)):
        return False
    worst = max(abs(x - y) for a, b in zip(trace64, trace32) for x, y in zip(a[1], b[1]))
    need = max(8.0 * worst, 1e-5)
    return all(m[i] - m[i + 1] >= need for _, _, m in trace64 for i in range(len(m) - 1))


# ---- the fixtures of test_sample_beam_search_vs_oracle ----------------------------------------------------------------
FIXTURES = [("attention_scn_odd", "attention_scn"), ("attention_scn_distinct", "attention_scn"),
            ("pure_scn_distinct", "pure_scn"), ("pure_attention_distinct", "pure_attention")]
BEAMS = (1, 3, 5)


def word_map(V):
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    for i in range(1, V - 3):
        wm["w%d" % i] = i
    return wm


def sharpened(name):
    """the golden decoder with that test's sharpening: fc.weight x 10, fc.bias[<end>] += 0.2"""
    from helpers import load_golden
    d = dict(load_golden(name))
    V = d["p.embedding.weight"].shape[0]
    d["p.fc.weight"] = d["p.fc.weight"] * 10.0
    fb = d["p.fc.bias"].copy()
    fb[V - 1] += 0.2
    d["p.fc.bias"] = fb
    return d, V


_CASES = {}


def oracle_cases(name, kind):
    """per (image, beam size) of a fixture: the fp64 oracle's result (None: it raised) and whether the case is decidable;
    computed once per process"""
    if name in _CASES:
        return _CASES[name]
    from helpers import params_from, t
    d, V = sharpened(name)
    wm = word_map(V)
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    use_tags = kind != "pure_attention"
    cases = {}
    for b in range(d["enc"].shape[0]):
        enc = t(d["enc"])[b:b + 1]
        tags = t(d["tags"])[b:b + 1] if use_tags else None
        for k in BEAMS:
            r64, t64 = trace_oracle(kind, P64, k, wm, enc.double(), None if tags is None else tags.double())
            _, t32 = trace_oracle(kind, P32, k, wm, enc.float(), None if tags is None else tags.float())
            cases[(b, k)] = (r64, decidable(t64, t32))
    _CASES[name] = cases
    return cases
