"""GPU tests (``-m gpu``) of the self-critical training surface above the kernels: CaptionScorer.score_rows and
trains.harness.SCSTTrainStep.

score_rows must give the bits of score(per_image=True)['cider'] for image_index = arange(N), and a permuted or repeated
index the matching rows.  A step is checked from what it reports in `last` (the sampled captions, their lengths, the
advantages): its loss and every parameter gradient against decoder.forward on those captions followed by the weighted
cross-entropy in plain torch fp64 (the tolerances of tests/test_gpu_parity.py for decoder outputs and gradients), its
rewards against score_rows on those tokens, the advantages against the baseline's definition.  The decoders are the golden
fixtures' (tests/test_gpu_parity._build_decoder's weights, sharpened as in tests/beam_refs.py so that captions end)."""
import copy
import types

import pytest
import torch

import beam_refs as BR
import textmetrics_refs as T
from helpers import params_from, rel_err, t
from test_gpu_parity import TOL_GRAD, TOL_OUT, _check_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- score_rows ---------------------------------------------------------------------------------------------------------
def test_score_rows_is_score_per_image_gathered(dev):
    from scnattn import textmetrics as TM
    START, END, PAD = 27, 28, 0
    hyps, refs = T.random_corpus(5, 12, 25, cpi=4, lo=3, hi=15, noise=0.3)
    refs[3][2] = None
    hyps[7] = []
    raw_h = [[START] + h + [END] + [PAD] * (i % 3) for i, h in enumerate(hyps)]
    raw_r = [[None if r is None else [START] + r + [END] + [PAD] * 2 for r in per] for per in refs]
    special = (START, END, PAD)
    scorer = TM.CaptionScorer(raw_r, skip_ref=special, device=dev)
    want = scorer.score(raw_h, skip_hyp=special, per_image=True)["cider"]
    hyp, hyp_len = TM.pack_captions(raw_h, dev)
    got, flag = scorer.score_rows(torch.arange(12, device=dev), hyp, hyp_len, skip_hyp=special)
    assert got.dtype == torch.float64 and got.is_cuda and flag.is_cuda and int(flag) == 0
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "score_rows(arange) is not score()'s per-image CIDEr-D"
    assert float(got.max()) > 0.1
    # a permuted and repeated index with the matching hypotheses gives the matching rows, whatever the number of rows
    idx = torch.tensor([11, 0, 0, 5, 7, 3, 3, 3, 9, 1, 2, 4, 6, 8, 10, 11, 5])
    got2, _ = scorer.score_rows(idx, hyp[idx.to(dev)], hyp_len[idx.to(dev)], skip_hyp=special)      # a host index is uploaded
    assert torch.equal(got2.view(torch.int64), want[idx.to(dev)].view(torch.int64))
    # another image's references: the score of that pairing, i.e. what score() gives when the hypotheses are swapped
    swap = list(range(12))
    swap[2], swap[6] = 6, 2
    want_sw = scorer.score([raw_h[i] for i in swap], skip_hyp=special, per_image=True)["cider"]
    got3, _ = scorer.score_rows(torch.tensor([6, 2], device=dev), hyp[[2, 6]], hyp_len[[2, 6]], skip_hyp=special)
    assert torch.equal(got3.view(torch.int64), want_sw[[6, 2]].view(torch.int64))
    empty, _ = scorer.score_rows(torch.zeros(0, dtype=torch.long), hyp[:0], hyp_len[:0])
    assert tuple(empty.shape) == (0,)
    _, flag = scorer.score_rows(torch.tensor([0]), torch.full((1, 4), 70000, dtype=torch.int32, device=dev),
                                torch.tensor([4], dtype=torch.int32, device=dev))
    assert int(flag) != 0                                                       # a token outside CIDEr-D's range is flagged


# ---- SCSTTrainStep ------------------------------------------------------------------------------------------------------
N_IMG, SAMPLES = 3, 2
FIX = {"attention_scn": "attention_scn_distinct", "pure_scn": "pure_scn_distinct", "pure_attention": "pure_attention_distinct"}


def _cfg_of(kind, d):
    V, M = d["p.embedding.weight"].shape
    D, E = d["p.init_h.weight"].shape
    cfg = dict(emb_dim=M, decoder_dim=D, encoder_dim=E, vocab_size=V, dropout=0.0, attention_dim=8, factored_dim=8, semantic_dim=1)
    if kind != "pure_scn":
        cfg["attention_dim"] = d["p.attention.encoder_att.weight"].shape[0]
    if kind != "pure_attention":
        S, F4 = d["p.decode_step.weight_ib"].shape
        cfg.update(semantic_dim=S, factored_dim=F4 // 4)
    return cfg


def _scorer(dev, V, n_images=5):
    """references over the fixture's vocabulary (words 1 .. V-4), four per image"""
    from scnattn import textmetrics as TM
    g = torch.Generator().manual_seed(17)
    refs = [[[V - 2] + torch.randint(1, V - 3, (int(torch.randint(3, 9, (1,), generator=g)),), generator=g).tolist() + [V - 1]
             for _ in range(4)] for _ in range(n_images)]
    return TM.CaptionScorer(refs, skip_ref=(V - 2, V - 1, 0), device=dev)


def _step_object(kind, baseline, dev, scorer=None, cls=None, **kw):
    from trains.harness import SCSTTrainStep
    d, V = BR.sharpened(FIX[kind])
    args = dict(kind=kind, device=dev, encoder=False, seed=3, decoder_lr=1e-3, **_cfg_of(kind, d))
    args.update(kw)
    if cls is None:
        ts = SCSTTrainStep(scorer=scorer or _scorer(dev, V), samples=SAMPLES, baseline=baseline, temperature=1.0,
                           word_map=BR.word_map(V), rollout_seed=77, **args)
    else:
        ts = cls(**args)
    ts.decoder.load_state_dict(params_from(d))
    enc = t(d["enc"])[:N_IMG].to(dev)
    tags = t(d["tags"])[:N_IMG].to(dev) if kind != "pure_attention" else torch.zeros(N_IMG, 1, device=dev)
    return ts, d, V, enc, tags


def _reference(ts, state, enc, tags, last):
    """decoder.forward on the reported captions + the weighted cross-entropy in plain torch fp64 -> (loss, module)"""
    m = copy.deepcopy(ts.decoder)
    m.load_state_dict(state)
    m.zero_grad(set_to_none=True)
    S = ts.samples
    caps, caplens, adv = last["caps"], last["caplens"], last["advantage"]
    e, tg = enc.repeat_interleave(S, 0), tags.repeat_interleave(S, 0)
    if ts.kind == "attention_scn":
        scores, caps_s, dl, alphas, si = m(e, tg, caps, caplens)
    elif ts.kind == "pure_scn":
        scores, caps_s, dl, si = m(e, tg, caps, caplens)
        alphas = None
    else:
        scores, caps_s, dl, alphas, si = m(e, caps, caplens)
    s64, w = scores.double(), adv[si].float().double()       # the step hands the advantage over in fp32
    n = sum(dl)
    total = s64.new_zeros(())
    for b, l in enumerate(dl):
        lp = torch.log_softmax(s64[b, :l], dim=1)
        total = total - w[b] * lp.gather(1, caps_s[b, 1:l + 1].unsqueeze(1)).sum()
    loss = total / n
    if alphas is not None:
        loss = loss + ts.cfg["alpha_c"] * ((1.0 - alphas.double().sum(dim=1)) ** 2).mean()
    loss.backward()
    return loss.detach(), m, dl


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
@pytest.mark.parametrize("kind", sorted(FIX))
def test_scst_step(dev, kind, baseline):
    ts, d, V, enc, tags = _step_object(kind, baseline, dev)
    index = torch.tensor([4, 0, 2])
    K = SAMPLES + (1 if baseline == "greedy" else 0)
    assert ts.K == K
    seen = []
    for step in range(2):
        state = copy.deepcopy(ts.decoder.state_dict())
        loss = ts.step(None, tags, index, encoder_out=enc)
        last = ts.last
        caps, caplens, adv, reward = last["caps"], last["caplens"], last["advantage"], last["reward"]
        assert tuple(caps.shape) == (N_IMG * SAMPLES, caps.shape[1]) and tuple(caplens.shape) == (N_IMG * SAMPLES, 1)
        assert caps.dtype == torch.int64 and caps.is_cuda and adv.dtype == torch.float64 and ts.draw == step + 1
        assert bool((caps[:, 0] == V - 2).all())
        lens = caplens.reshape(-1).tolist()
        for r, l in enumerate(lens):            # <start>, tokens, <end> (unless cut off), <pad> behind
            row = caps[r].tolist()
            assert all(x == 0 for x in row[l:]) and (row[l - 1] == V - 1 or l == caps.shape[1]) and V - 1 not in row[1:l - 1]
        # rewards: score_rows on those tokens
        rows_image = index.repeat_interleave(SAMPLES)
        want_r, _ = ts.scorer.score_rows(rows_image, caps[:, 1:].to(torch.int32), (caplens.reshape(-1) - 1).to(torch.int32),
                                         skip_hyp=(V - 2, V - 1, 0))
        assert torch.equal(reward.view(torch.int64), want_r.view(torch.int64))
        ra = last["reward_all"]
        assert tuple(ra.shape) == (N_IMG, K)
        if baseline == "greedy":
            assert torch.equal(ra[:, 1:].reshape(-1), reward)
            assert torch.equal(adv.view(N_IMG, SAMPLES), ra[:, 1:] - ra[:, :1])
            assert float((last["mean_baseline"] - ra[:, 0].mean()).abs()) <= 1e-12
        else:
            assert torch.equal(ra.reshape(-1), reward)
            sums = adv.view(N_IMG, SAMPLES).sum(dim=1).abs()
            assert float(sums.max()) <= 1e-12 * max(1.0, float(reward.abs().max())), sums
        assert float((last["mean_reward"] - reward.mean()).abs()) <= 1e-12 and last["mean_advantage"].dim() == 0
        # loss and gradients
        grads = {k: p.grad.detach().clone() for k, p in ts.decoder.named_parameters()}
        want, m, dl = _reference(ts, state, enc, tags, last)
        e = rel_err(loss.detach(), want) if float(want.abs()) > 1e-6 else float((loss.detach().double() - want).abs())
        print("%s %s step %d: lengths %s rewards %s loss %.6f vs %.6f" % (
            kind, baseline, step, lens, [round(float(x), 3) for x in reward], float(loss.detach()), float(want)))
        assert e <= TOL_OUT, (float(loss.detach()), float(want))
        ref_g = {k: p.grad.cpu() for k, p in m.named_parameters()}
        _check_grads([(k, types.SimpleNamespace(grad=g)) for k, g in grads.items()], lambda k: ref_g[k], TOL_GRAD)
        seen.append(caps.clone())
    # the second step drew other noise from the same seed
    assert seen[0].shape != seen[1].shape or not torch.equal(seen[0], seen[1])


def test_scst_rollout_repeats_for_the_same_draw_and_not_for_the_next(dev):
    ts, d, V, enc, tags = _step_object("attention_scn", "greedy", dev)
    wm = BR.word_map(V)
    with torch.no_grad():
        a = ts.decoder.rollout_batch(wm, enc, tags, samples=2, seed=77, draw=0, greedy_first=True)
        b = ts.decoder.rollout_batch(wm, enc, tags, samples=2, seed=77, draw=0, greedy_first=True)
        c = ts.decoder.rollout_batch(wm, enc, tags, samples=2, seed=77, draw=1, greedy_first=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    assert torch.equal(a[0][0::3, :min(a[0].shape[1], c[0].shape[1])], c[0][0::3, :min(a[0].shape[1], c[0].shape[1])])     # the arg-max slots do not depend on the draw


def test_cross_entropy_step_is_untouched_by_an_scst_object(dev):
    """TrainStep on the same model trains bit-identically before and after an SCSTTrainStep has been built and used"""
    from trains.harness import TrainStep, synthetic_batch

    def run():
        ts, d, V, enc, tags = _step_object("attention_scn", None, dev, cls=TrainStep)
        _, _, caps, caplens = synthetic_batch(N_IMG, V, 6, 8, 1, dev, 5, ragged=True)
        losses = [ts.step(None, tags, caps, caplens, encoder_out=enc).detach().clone() for _ in range(2)]
        return losses + [p.detach().clone() for p in ts.decoder.parameters()]
    before = run()
    sc, d, V, enc, tags = _step_object("attention_scn", "mean", dev)
    sc.step(None, tags, torch.tensor([1, 2, 3]), encoder_out=enc)
    after = run()
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
