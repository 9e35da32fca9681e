"""tests/ensemble_refs.py (the fp64 restatements the ensemble beam search is tested against on the GPU) pinned on the CPU:
a one-member ensemble is beam_refs.search exactly, both modes against a direct log_softmax computation, mode 1 on rows
whose probabilities all underflow, the derived bound against CPU fp32 arithmetic, and every host-side refusal of
DecoderEnsemble (none of which needs a device)."""
import math

import pytest
import torch
import torch.nn.functional as F

import beam_refs as BR
import ensemble_refs as ER
from helpers import params_from, t

DISTINCT = [f for f in BR.FIXTURES if f[0].endswith("_distinct")]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("name,kind", DISTINCT)
def test_one_member_search_is_beam_refs_search(name, kind):
    """sequences, completed lists, scores and alphas EQUAL, in fp64 and in fp32, image by image"""
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    for dtype in (torch.float64, torch.float32):
        Pm = params_from(d, dtype=dtype)
        enc = t(d["enc"]).to(dtype)
        tags = t(d["tags"]).to(dtype) if use_tags else None
        for k in BR.BEAMS:
            for b in range(enc.shape[0]):
                tg = None if tags is None else tags[b:b + 1]
                (one, done), = BR.search(kind, Pm, k, wm, enc[b:b + 1], tg)
                got = ER.search((kind,), [Pm], [1.0], "logprob", k, wm, enc[b:b + 1], tg)
                assert got.done == done, (b, k)
                if use_att:
                    assert got.seq == one[0] and got.alphas == one[1], (b, k)
                else:
                    assert got.seq == one and got.alphas is None, (b, k)
                assert len(got.trace) >= 1 and all(len(m) <= k + 1 for _, _, m in got.trace)


@pytest.mark.parametrize("M", [1, 2, 4])
def test_modes_vs_log_softmax(M):
    g = _gen(M)
    R, V, K = 5, 203, 4
    logits = [torch.randn(R, V, generator=g, dtype=torch.float64) * 3 for _ in range(M)]
    scores = torch.randn(R, generator=g, dtype=torch.float64)
    w = ER.member_weights([1.0 + m for m in range(M)], M)
    assert abs(sum(w) - 1.0) <= M * 2.0 ** -24 and all(x == float(torch.tensor(x).float()) for x in w)
    lp = torch.stack([F.log_softmax(x, dim=1) for x in logits])
    wt = torch.tensor(w, dtype=torch.float64).view(M, 1, 1)
    want = {0: (wt * lp).sum(0), 1: torch.log((wt * lp.exp()).sum(0))}
    for mode in (0, 1):
        cv, ci, c = ER.row_topk_ens(logits, w, mode, scores, K)
        assert float((c - want[mode]).abs().max()) <= 1e-12
        tv, ti = (scores.unsqueeze(1) + want[mode]).topk(K, 1, True, True)
        assert torch.equal(ci, ti) and float((cv - tv).abs().max()) <= 1e-12
    # Jensen: the log of the mean is at least the mean of the logs, with equality for one member
    assert bool((want[1] >= want[0] - 1e-12).all()) and (M > 1 or float((want[1] - want[0]).abs().max()) <= 1e-12)


def test_mode1_is_finite_where_every_probability_underflows():
    """rows where l_mv < -200 for every member and most words: exp(l_mv) is 0 in fp32, a + log(sum w exp(l - a)) is not"""
    g = _gen(7)
    R, V, M = 3, 64, 3
    logits = [torch.randn(R, V, generator=g) * 2 - 300.0 for _ in range(M)]
    for x in logits:
        x[:, 0] = 0.0           # one word holds all the mass: every other l_mv is about -300
    w = ER.member_weights(None, M)
    for dtype in (torch.float32, torch.float64):
        ls = ER.log_probs([x.to(dtype) for x in logits])
        assert all(float(l[:, 1:].max()) < -200 for l in ls)
        c = ER.combine([x.to(dtype) for x in logits], w, 1)
        assert bool(torch.isfinite(c).all()) and float(c[:, 1:].max()) < -200
        if dtype == torch.float32:
            assert float(torch.exp(ls[0][:, 1:]).max()) == 0.0
            naive = torch.log(sum(wm * torch.exp(l) for wm, l in zip(w, ls)))
            assert bool(torch.isinf(naive[:, 1:]).all())
    ties = ER.row_topk_ens([torch.zeros(1, 6, dtype=torch.float64)] * 2, [0.5, 0.5], 1, torch.zeros(1, dtype=torch.float64), 3)
    assert ties[1].tolist() == [[0, 1, 2]]          # equal values: the lower word first


@pytest.mark.parametrize("mode", [0, 1])
def test_bound_covers_cpu_fp32(mode):
    """the derived bound is a bound of fp32 arithmetic: torch's own fp32 evaluation of the same formula stays inside it"""
    g = _gen(11 + mode)
    R, V, M = 6, 1003, 4
    logits = [(torch.randn(R, V, generator=g) * (3 + m)).float() for m in range(M)]
    scores = (torch.randn(R, generator=g) * 2).float()
    w = ER.member_weights([4, 3, 2, 1], M)
    c32 = ER.combine(logits, w, mode)
    c64 = ER.combine([x.double() for x in logits], w, mode)
    bc, bv = ER.value_bounds([x.double() for x in logits], w, mode, scores.double())
    assert bool(((c32.double() - c64).abs() <= bc).all())
    v32 = scores.unsqueeze(1) + c32
    assert bool(((v32.double() - (scores.double().unsqueeze(1) + c64)).abs() <= bv).all())
    assert float(bv.max()) < 1e-3           # ... and is no licence: about V u


def _tiny(kind, V=12):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    if kind == "attention_scn":
        return AttentionSCN(5, 4, 6, 7, 3, V, encoder_dim=8)
    if kind == "pure_scn":
        return PureSCN(4, 6, 7, 3, V, encoder_dim=8)
    return PureAttention(5, 4, 6, V, encoder_dim=8)


def test_decoder_ensemble_refusals_and_shape():
    from models.decoders import DecoderEnsemble
    a, s, p = _tiny("attention_scn"), _tiny("pure_scn"), _tiny("pure_attention")
    ens = DecoderEnsemble([s, a, p], weights=[2, 1, 1], combine="prob")
    assert ens.alpha_member == 1 and ens.needs_tags and ens.has_alphas and len(ens.decoders) == 3
    assert ens.member_weights == [0.5, 0.25, 0.25]
    assert DecoderEnsemble([a, s]).member_weights == [0.5, 0.5]
    assert set(dict(ens.named_parameters())) >= {"decoders.0.fc.weight", "decoders.2.fc.weight"}
    ens.train()
    assert not ens.eval().decoders[1].training
    only_s = DecoderEnsemble([s, s])
    assert only_s.alpha_member is None and not only_s.has_alphas
    assert not DecoderEnsemble([p]).needs_tags
    assert DecoderEnsemble([a, p], alpha_member=1).alpha_member == 1
    for bad in ([], [a] * 5):
        with pytest.raises(ValueError):
            DecoderEnsemble(bad)
    with pytest.raises(ValueError):
        DecoderEnsemble([a, _tiny("pure_scn", V=13)])
    for badw in ([1.0], [1.0, 0.0], [1.0, -1.0], [1.0, math.inf], [1.0, math.nan]):
        with pytest.raises(ValueError):
            DecoderEnsemble([a, s], weights=badw)
    with pytest.raises(ValueError):
        DecoderEnsemble([a, s], combine="mean")
    with pytest.raises(ValueError):
        DecoderEnsemble([a, s], alpha_member=1)         # PureSCN has no maps
    with pytest.raises(ValueError):
        DecoderEnsemble([a, torch.nn.Linear(2, 2)])
    wm = BR.word_map(12)
    enc, tags = torch.zeros(2, 2, 2, 8), torch.zeros(2, 3)
    for k in (0, 9):
        with pytest.raises(ValueError):
            ens.sample_batch(k, wm, enc, tags)
    with pytest.raises(ValueError):
        ens.sample_batch(3, BR.word_map(13), enc, tags)
    with pytest.raises(ValueError):
        ens.sample_batch(3, wm, enc)                    # a member uses tags
    with pytest.raises(RuntimeError):
        ens.sample_batch(3, wm, enc, tags)              # host tensors: there is no CPU path


def test_member_weights_restatement_matches_the_library():
    from scnattn import functional as SF
    for ws in (None, [1, 2], [0.3, 0.3, 0.3], [5, 3], [1e-3, 1, 7, 2]):
        M = 2 if ws is None else len(ws)
        assert SF.normalise_member_weights(ws, M) == ER.member_weights(ws, M)
