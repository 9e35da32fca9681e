"""GPU tests (``-m gpu``) of the caption text metrics above the kernels: scnattn.textmetrics.CaptionScorer,
validate(fused=True, device_bleu=True) and trains.harness.evaluate_captions.

1. CaptionScorer.score on a 40-image corpus (V = 25, five references, some slots absent, special tokens skipped on both
   sides) against tests/textmetrics_refs.py: the BLEU values are EQUAL (same integers, same host arithmetic), ROUGE_L and
   CIDEr within 1e-12 * max(1, |ref|) (the bar of tests/test_gpu_textmetrics_kernels.py); the per_image=True tensors element by
   element, integers exactly; the document-frequency tables equal the restatement's.
2. validate(fused=True, device_bleu=True) returns the same three values, bit for bit, as device_bleu=False, on the fake-encoder
   batches of tests/test_gpu_caption_metrics_step.py, for the three decoders.
3. evaluate_captions on a random-weight AttentionSCN / PureSCN / PureAttention (B = 4 per batch, a 2x2 feature map, V = 30,
   beam 3) equals the restatements applied to sample_batch's own output."""
import pytest
import torch

import textmetrics_refs as T

pytestmark = pytest.mark.gpu

TOL = 1e-12
BLEU_KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "bleu4_nltk")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _close(got, want):
    return abs(got - want) <= TOL * max(1.0, abs(want))


def _same_scores(got, want):
    assert set(want) <= set(got)
    for k in BLEU_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("ROUGE_L", "CIDEr"):
        assert _close(got[k], want[k]), (k, got[k], want[k])


def test_scorer_against_the_restatements(dev):
    from scnattn import textmetrics as TM
    START, END, PAD = 27, 28, 0
    hyps, refs = T.random_corpus(5, 40, 25, cpi=5, lo=3, hi=20, noise=0.3)
    refs[3][2] = None                                                      # an absent slot in the middle
    refs[9] = [refs[9][0], None, None, None, None]
    hyps[11] = []
    raw_h = [[START] + h + [END] + [PAD] * (i % 3) for i, h in enumerate(hyps)]
    raw_r = [[None if r is None else [START] + r + [END] + [PAD] * 2 for r in per] for per in refs]
    special = (START, END, PAD)
    scorer = TM.CaptionScorer(raw_r, skip_ref=special, device=dev)
    out = scorer.score(raw_h, skip_hyp=special, per_image=True)
    _same_scores(out, T.score_all(hyps, refs))
    assert 0.0 < out["Bleu_4"] < out["Bleu_1"] < 1.0 and out["CIDEr"] > 0.1 and out["ROUGE_L"] > 0.1
    for (keys, df), off0, off1 in zip(T.df_tables(refs), scorer.table_off[:-1], scorer.table_off[1:]):
        assert scorer.table_keys[off0:off1].tolist() == keys and scorer.table_df[off0:off1].tolist() == df
    stats, lcs, rouge, cider = (out[k].tolist() for k in ("stats", "lcs", "rouge_l", "cider"))
    want_cider = T.cider_scores(hyps, refs)
    for i, (h, r) in enumerate(zip(hyps, refs)):
        ls, sc = T.rouge_l(h, r)
        assert stats[i] == T.ngram_stats(h, r) and lcs[i] == ls, i
        assert _close(rouge[i], sc) and _close(cider[i], want_cider[i]), i
    assert out["stats"].dtype == out["lcs"].dtype == torch.int32 and out["cider"].dtype == out["rouge_l"].dtype == torch.float64
    assert out["stats"].is_cuda and out["cider"].is_cuda
    plain = scorer.score(raw_h, skip_hyp=special)
    assert set(plain) == set(BLEU_KEYS) | {"ROUGE_L", "CIDEr"} and all(plain[k] == out[k] for k in plain)     # deterministic
    with pytest.raises(ValueError):
        scorer.score(raw_h[:5], skip_hyp=special)


@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn", "pure_attention"))
def test_validate_device_bleu_bit_for_bit(dev, kind):
    import test_gpu_caption_metrics_step as S
    from trains.harness import validate
    dec = S._decoder(kind).to(dev)
    batches = S._batches(dev)
    crit = torch.nn.CrossEntropyLoss()
    host = validate(batches, S._Encoder(), lambda imgs: imgs[1], dec, crit, S.WM, alpha_c=0.7, fused=True)
    devb = validate(batches, S._Encoder(), lambda imgs: imgs[1], dec, crit, S.WM, alpha_c=0.7, fused=True, device_bleu=True)
    assert len(host) == len(devb) == 3
    for a, b in zip(host, devb):
        assert isinstance(b, float) and a == b and a.hex() == b.hex(), (host, devb)
    with pytest.raises(ValueError):
        validate(batches, S._Encoder(), lambda imgs: imgs[1], dec, crit, S.WM, fused=False, device_bleu=True)


def test_validate_device_bleu_counts_matches(dev):
    """BLEU-4 of random-weight decoders is 0 either way; here the decoder is replaced by one that returns the targets, so that
    the equality above is also checked on a non-zero value"""
    import test_gpu_caption_metrics_step as S
    from trains.harness import validate
    inner = S._decoder("attention_scn").to(dev).eval()

    class Echo(torch.nn.Module):
        def forward(self, encoder_out, tags, caps, caplens):
            scores, caps_sorted, dl, alphas, sort_ind = inner(encoder_out, tags, caps, caplens)
            onehot = torch.nn.functional.one_hot(caps_sorted[:, 1:1 + scores.shape[1]], S.V).float() * 20.0
            flip = torch.zeros_like(onehot)
            flip[:, 5::6, 5] = 40.0                                        # every sixth prediction is token 5 instead
            return scores * 0.01 + onehot + flip, caps_sorted, dl, alphas, sort_ind

    batches = S._batches(dev)
    crit = torch.nn.CrossEntropyLoss()
    dec = Echo()
    host = validate(batches, S._Encoder(), lambda imgs: imgs[1], dec, crit, S.WM, alpha_c=0.7, fused=True)
    devb = validate(batches, S._Encoder(), lambda imgs: imgs[1], dec, crit, S.WM, alpha_c=0.7, fused=True, device_bleu=True)
    assert host[0] > 0.05 and all(a == b for a, b in zip(host, devb)), (host, devb)


@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn", "pure_attention"))
def test_evaluate_captions_equals_the_restatements_on_its_own_beams(dev, kind):
    import beam_refs as BR
    import test_gpu_caption_metrics_step as S
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    from trains.harness import evaluate_captions
    V, B, R, L = 30, 4, 3, 9
    wm = BR.word_map(V)
    torch.manual_seed(9)
    if kind == "attention_scn":
        dec = AttentionSCN(24, 20, 28, 36, 14, V, encoder_dim=40, dropout=0.5)
    elif kind == "pure_scn":
        dec = PureSCN(20, 28, 36, 14, V, encoder_dim=40, dropout=0.5)
    else:
        dec = PureAttention(24, 20, 28, V, encoder_dim=40, dropout=0.5)
    dec = dec.to(dev)
    g = torch.Generator().manual_seed(10)
    batches = []
    for _ in range(2):
        allcaps = torch.zeros(B, R, L, dtype=torch.long)
        for b in range(B):
            for r in range(R):
                n = int(torch.randint(3, L + 1, (1,), generator=g))
                allcaps[b, r, 0] = wm["<start>"]
                allcaps[b, r, 1:n - 1] = torch.randint(1, 8, (n - 2,), generator=g)
                allcaps[b, r, n - 1] = wm["<end>"]
        imgs = (torch.rand(B, 2, 2, 40, generator=g).to(dev), torch.rand(B, 14, generator=g).to(dev))
        batches.append((imgs, allcaps.to(dev)))
    got = evaluate_captions(batches, S._Encoder(), lambda imgs: imgs[1], dec, wm, beam_size=3)
    assert not dec.training
    special = {wm["<start>"], wm["<end>"], wm["<pad>"]}
    hyps, refs = [], []
    with torch.no_grad():
        for imgs, allcaps in batches:
            res = dec.sample_batch(3, wm, imgs[0]) if kind == "pure_attention" else dec.sample_batch(3, wm, imgs[0], imgs[1])
            for one in res:
                seq = one[0] if isinstance(one, tuple) else one
                assert seq[0] == wm["<start>"]
                hyps.append(T.strip(seq, special))
            refs.extend([[T.strip(c, special) for c in per] for per in allcaps.tolist()])
    assert len(hyps) == 2 * B and any(hyps)
    _same_scores(got, T.score_all(hyps, refs))
