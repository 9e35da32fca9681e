"""tests/beam_refs.py (the fp64 restatements the batched beam search is tested against on the GPU) against the oracle:
the attention pieces against oracle/scnattn_ref.attention_forward, the row selection against F.log_softmax + topk, and a
whole search assembled from the pieces against oracle/beam_ref.beam_search on the four beam-search fixtures -- which
pins the slot / counter semantics (K fixed slots, nsrc, kk, compaction in rank order) before any GPU runs."""
import pytest
import torch
import torch.nn.functional as F

import beam_refs as BR
from helpers import params_from, t


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_attention_pieces_vs_oracle():
    from oracle import scnattn_ref as R
    g = _gen(1)
    N, K, P, E, A, D = 3, 3, 7, 12, 10, 6
    Pm = {"attention.encoder_att.weight": torch.randn(A, E, generator=g, dtype=torch.float64),
          "attention.encoder_att.bias": torch.randn(A, generator=g, dtype=torch.float64),
          "attention.decoder_att.weight": torch.randn(A, D, generator=g, dtype=torch.float64),
          "attention.decoder_att.bias": torch.randn(A, generator=g, dtype=torch.float64),
          "attention.full_att.weight": torch.randn(1, A, generator=g, dtype=torch.float64),
          "attention.full_att.bias": torch.randn(1, generator=g, dtype=torch.float64)}
    enc = torch.randn(N, P, E, generator=g, dtype=torch.float64)
    h = torch.randn(N * K, D, generator=g, dtype=torch.float64)
    awe_r, alpha_r = R.attention_forward(Pm, "attention.", enc.repeat_interleave(K, 0), h)
    att1 = F.linear(enc, Pm["attention.encoder_att.weight"], Pm["attention.encoder_att.bias"])
    att2 = F.linear(h, Pm["attention.decoder_att.weight"])
    e = BR.attn_scores(att1, att2.unsqueeze(0), Pm["attention.decoder_att.bias"], Pm["attention.full_att.weight"].reshape(-1),
                       Pm["attention.full_att.bias"], K)["e"]
    ctx = BR.attn_context(enc, e, None, None, K)
    assert float((ctx["alpha"] - alpha_r).abs().max()) <= 1e-13
    assert float((ctx["awe"] - awe_r).abs().max()) <= 1e-12


@pytest.mark.parametrize("V,K", [(37, 1), (37, 5), (1003, 8)])
def test_row_topk_and_merge_vs_topk(V, K):
    """no ties in these inputs: the per-row top K and the merged top kk are what log_softmax + topk give"""
    g = _gen(V + K)
    ns, kk = max(K - 1, 1), max(K - 2, 1)
    logits = torch.randn(ns, V, generator=g, dtype=torch.float64) * 3
    scores = torch.randn(ns, generator=g, dtype=torch.float64)
    cv, ci, lse = BR.row_topk(logits, scores, K)
    full = scores.unsqueeze(1) + F.log_softmax(logits, dim=1)
    tv, ti = full.topk(K, 1, True, True)
    assert torch.equal(ci, ti) and float((cv - tv).abs().max()) <= 1e-12
    assert float((lse - torch.logsumexp(logits, 1)).abs().max()) == 0.0
    picks = BR.merge(cv, ci, V, kk)
    fv, fi = full.view(-1).topk(kk, 0, True, True)
    assert [j * V + w for _, j, w in picks] == fi.tolist()
    assert max(abs(p[0] - float(v)) for p, v in zip(picks, fv)) <= 1e-12


def test_tie_rule_and_compaction():
    """equal values: the lower flat index j*V + v first; <end> picks are recorded, the rest compacted in rank order"""
    V, K = 6, 4
    logits = torch.tensor([[0.0, 1.0, 1.0, -1.0, 1.0, 0.0]] * 2, dtype=torch.float64)
    cv, ci, _ = BR.row_topk(logits, torch.zeros(2, dtype=torch.float64), K)
    assert ci.tolist() == [[1, 2, 4, 0]] * 2
    picks = BR.merge(cv, ci, V, 4)
    assert [(j, w) for _, j, w in picks] == [(0, 1), (0, 2), (0, 4), (1, 1)]
    s = BR.ImageState(K)
    s.nsrc = 2
    tok, par = s.step([(-0.5, 1, 5), (-0.6, 0, 2), (-0.6, 1, 5), (-0.7, 0, 3)], 4, end=5)
    assert tok == [2, 3, 2, 2] and par == [0, 0, 0, 0] and s.nsrc == 2 and s.kk == 2
    assert s.comp == [(-0.5, 4, 1), (-0.6, 4, 1)] and s.best == 0 and s.scores == [-0.6, -0.7, 0.0, 0.0]
    s.step([(-0.5, 0, 5), (-0.4, 1, 5)], 5, end=5)          # an equal score does not replace the best, a greater one does
    assert s.best == 3 and s.kk == 0 and s.nsrc == 0


def test_advance_is_a_gather():
    K = 2
    h = torch.arange(8.0).view(4, 2)
    c = -h
    table = torch.arange(12.0).view(6, 2)
    h2, c2, emb = BR.advance(h, c, [1, 1, 0, 1], [5, 0, 3, 3], table, K)
    assert h2.tolist() == [[2, 3], [2, 3], [4, 5], [6, 7]] and torch.equal(c2, -h2)
    assert emb.tolist() == [[10, 11], [0, 1], [6, 7], [6, 7]]


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_search_vs_oracle_beam_search(name, kind):
    """all images of a fixture as one batch, k in {1, 3, 5}, fp64: chosen sequence, every completed sequence in order,
    scores and alphas as the oracle's; where the oracle raises (nothing completed) the fallback is the best open beam"""
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    P64 = params_from(d, dtype=torch.float64)
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    enc = t(d["enc"]).double()
    tags = t(d["tags"]).double() if use_tags else None
    cases = BR.oracle_cases(name, kind)
    compared = 0
    for k in BR.BEAMS:
        got = BR.search(kind, P64, k, wm, enc, tags)
        for b, (one, done) in enumerate(got):
            ref = cases[(b, k)][0]
            seq = one[0] if use_att else one
            if ref is None:
                assert seq[0] == V - 2 and len(seq) == 52 and V - 1 not in seq
                continue
            (r_one, r_all) = ref
            assert seq == (r_one[0] if use_att else r_one), (b, k)
            assert [s for s, _ in done] == [s for s, _ in r_all], (b, k)
            assert max(abs(x[1] - y[1]) for x, y in zip(done, r_all)) <= 1e-12
            if use_att:
                assert float((torch.tensor(one[1]) - torch.tensor(r_one[1])).abs().max()) <= 1e-12
            compared += 1
    assert compared >= 4


def test_decidable_counts():
    """the caps the GPU tests assert, checked where the rule is computed: at most 1/4 of the 54 cases and at most 1/2 of any
    fixture's cases are left out"""
    left = []
    for name, kind in BR.FIXTURES:
        cases = BR.oracle_cases(name, kind)
        out = sum(1 for _, ok in cases.values() if not ok)
        assert 2 * out <= len(cases), (name, out, len(cases))
        left.append((out, len(cases)))
    print("left out per fixture:", left)
    assert sum(n for _, n in left) == 54 and 4 * sum(o for o, _ in left) <= 54
