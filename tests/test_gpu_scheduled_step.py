"""GPU tests (``-m gpu``) of scheduled sampling in the cross-entropy step (trains.harness.TrainStep(scheduled_sampling=p)), on
the decoder-only step with the `_distinct` fixtures' weights (sharpened as in tests/beam_refs.py), dropout 0 and three images,
in the manner of tests/test_gpu_scst_step.py.

A mixed step is checked from what it reports in `last_mix`: bit for bit against the same three calls made by hand on a copy of
the model (mix_batch, forward on its inputs, caption_loss against the GOLD captions), and within the tolerances of
tests/test_gpu_parity.py against forward on those inputs followed by the cross-entropy in plain torch fp64 -- against the gold
words; the same fp64 loss against the inputs themselves must be far away, which shows what the targets are."""
import copy
import types

import pytest
import torch

import beam_refs as BR
from helpers import params_from, rel_err, t
from test_gpu_parity import TOL_GRAD, TOL_OUT, _check_grads
from test_gpu_scst_step import FIX, _cfg_of

pytestmark = pytest.mark.gpu

N_IMG = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _step_object(kind, dev, cls=None, **kw):
    from trains.harness import TrainStep, synthetic_batch
    d, V = BR.sharpened(FIX[kind])
    args = dict(kind=kind, device=dev, encoder=False, seed=3, decoder_lr=1e-3, **_cfg_of(kind, d))
    args.update(kw)
    ts = (cls or TrainStep)(**args)
    ts.decoder.load_state_dict(params_from(d))
    enc = t(d["enc"])[:N_IMG].to(dev)
    tags = t(d["tags"])[:N_IMG].to(dev) if kind != "pure_attention" else torch.zeros(N_IMG, 1, device=dev)
    _, _, caps, caplens = synthetic_batch(N_IMG, V, 9, 8, 1, dev, 5, ragged=True)      # lengths 7 .. 11: 5 .. 9 inputs to mix
    return ts, V, enc, tags, caps, caplens


def _forward(kind, m, enc, tags, caps, caplens):
    if kind == "attention_scn":
        scores, caps_s, dl, alphas, si = m(enc, tags, caps, caplens)
    elif kind == "pure_scn":
        scores, caps_s, dl, si = m(enc, tags, caps, caplens)
        alphas = None
    else:
        scores, caps_s, dl, alphas, si = m(enc, caps, caplens)
    return scores, caps_s, dl, alphas, si


def _copy(ts, state):
    m = copy.deepcopy(ts.decoder)
    m.load_state_dict(state)
    m.zero_grad(set_to_none=True)
    return m


def _fp64_loss(ts, scores, targets_sorted, dl, alphas):
    s64 = scores.double()
    total = s64.new_zeros(())
    for b, l in enumerate(dl):
        lp = torch.log_softmax(s64[b, :l], dim=1)
        total = total - lp.gather(1, targets_sorted[b, 1:l + 1].unsqueeze(1)).sum()
    loss = total / sum(dl)
    if alphas is not None:
        loss = loss + ts.cfg["alpha_c"] * ((1.0 - alphas.double().sum(dim=1)) ** 2).mean()
    return loss


# ---- (a) probability 0 is the step as it was ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FIX))
def test_probability_zero_is_the_plain_step_bit_for_bit(dev, kind):
    def run(**kw):
        ts, V, enc, tags, caps, caplens = _step_object(kind, dev, **kw)
        losses = [ts.step(None, tags, caps, caplens, encoder_out=enc).detach().clone() for _ in range(2)]
        assert ts.last_mix is None and ts.steps_done == 2
        return losses + [p.detach().clone() for p in ts.decoder.parameters()]
    plain, zero = run(), run(scheduled_sampling=0.0, ss_temperature=0.7, ss_greedy=True, ss_seed=5)
    for x, y in zip(plain, zero):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- (b) a mixed step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", (1.0, 0.5))
@pytest.mark.parametrize("kind", sorted(FIX))
def test_mixed_step(dev, kind, prob):
    from scnattn import functional as SF
    ts, V, enc, tags, caps, caplens = _step_object(kind, dev, scheduled_sampling=prob, ss_seed=77, ss_temperature=0.7)
    wm = BR.word_map(V)
    seen = []
    for step in range(2):
        state = copy.deepcopy(ts.decoder.state_dict())
        loss = ts.step(None, tags, caps, caplens, encoder_out=enc)
        grads = {k: p.grad.detach().clone() for k, p in ts.decoder.named_parameters()}
        last = ts.last_mix
        assert sorted(last) == ["inputs", "n_replaced", "replaced"] and all(x.is_cuda for x in last.values())
        assert ts.steps_done == step + 1
        inputs, replaced = last["inputs"], last["replaced"]
        nmix = (caplens.view(-1) - 2).clamp_min(0)
        pos = torch.arange(caps.shape[1], device=dev).unsqueeze(0)
        can = (pos >= 1) & (pos <= nmix.unsqueeze(1))
        assert not bool((replaced & ~can).any()) and torch.equal(inputs[~replaced], caps[~replaced])
        assert torch.equal(last["n_replaced"].long(), replaced.sum(dim=1))
        if prob == 1.0:
            assert torch.equal(replaced, can)
        else:
            assert 0 < int(replaced.sum()) < int(can.sum())
        # by hand on a copy of the model, bit for bit
        m = _copy(ts, state)
        with torch.no_grad():
            mix = m.mix_batch(wm, enc, tags, caps, caplens, prob, seed=77, draw=step, temperature=0.7)
        assert torch.equal(mix["inputs"], inputs) and torch.equal(mix["replaced"], replaced)
        scores, caps_s, dl, alphas, si = _forward(kind, m, enc, tags, mix["inputs"], caplens)
        assert torch.equal(caps_s, inputs[si])
        gold_s = caps[si]
        by_hand = SF.caption_loss(scores, gold_s, dl, alphas, ts.cfg["alpha_c"], (caplens.reshape(-1)[si] - 1).to(torch.int32))
        by_hand.backward()
        assert torch.equal(loss.detach().view(torch.int32), by_hand.detach().view(torch.int32)), (float(loss), float(by_hand))
        for k, p in m.named_parameters():
            assert torch.equal(grads[k].view(torch.int32), p.grad.view(torch.int32)), k
        # plain torch fp64 on the same inputs, against the gold words -- and, to show the difference, against the inputs
        m = _copy(ts, state)
        scores, caps_s, dl, alphas, si = _forward(kind, m, enc, tags, inputs, caplens)
        want = _fp64_loss(ts, scores, gold_s, dl, alphas)
        want.backward()
        wrong = _fp64_loss(ts, scores.detach(), caps_s, dl, None if alphas is None else alphas.detach())
        print("%s p=%g step %d: %d of %d inputs replaced; loss %.6f, fp64 %.6f, fp64 with the inputs as targets %.6f" % (
            kind, prob, step, int(replaced.sum()), int(can.sum()), float(loss.detach()), float(want.detach()), float(wrong)))
        assert rel_err(loss.detach(), want.detach()) <= TOL_OUT, (float(loss), float(want))
        assert rel_err(wrong, want.detach()) > 10 * TOL_OUT, (float(wrong), float(want))
        ref_g = {k: p.grad.cpu() for k, p in m.named_parameters()}
        _check_grads([(k, types.SimpleNamespace(grad=g)) for k, g in grads.items()], lambda k: ref_g[k], TOL_GRAD)
        seen.append(replaced.clone() if prob < 1.0 else inputs.clone())
    assert not torch.equal(seen[0], seen[1])            # the second step flipped other coins / drew other noise


# ---- (c) the metrics count against the gold words ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn"))
def test_metrics_count_against_the_gold_words(dev, kind):
    ts, V, enc, tags, caps, caplens = _step_object(kind, dev, scheduled_sampling=0.5, ss_seed=77, metrics=True)
    state = copy.deepcopy(ts.decoder.state_dict())
    loss = ts.step(None, tags, caps, caplens, encoder_out=enc)
    got_loss, hits, n = ts.last_metrics
    m = _copy(ts, state)
    with torch.no_grad():
        scores, caps_s, dl, alphas, si = _forward(kind, m, enc, tags, ts.last_mix["inputs"], caplens)
    gold_s = caps[si]
    top5 = top1 = 0
    for b, l in enumerate(dl):
        s, tgt = scores[b, :l], gold_s[b, 1:l + 1]
        st = s.gather(1, tgt.unsqueeze(1))
        idx = torch.arange(V, device=dev).unsqueeze(0)
        rank = ((s > st) | ((s == st) & (idx < tgt.unsqueeze(1)))).sum(dim=1)
        top5, top1 = top5 + int((rank < 5).sum()), top1 + int((rank < 1).sum())
    assert n == sum(dl) and hits.tolist() == [top5, top1], (hits.tolist(), top5, top1)
    assert torch.equal(got_loss.view(torch.int32), loss.detach().view(torch.int32))
    assert ts.topk_percent() == pytest.approx(100.0 * top5 / n)


# ---- (d) the probability can be moved between steps; every step is a draw ---------------------------------------------------------
def test_set_sampling_prob_and_the_draw_counter(dev):
    kind = "attention_scn"
    ts, V, enc, tags, caps, caplens = _step_object(kind, dev, ss_seed=77)
    wm = BR.word_map(V)
    ts.step(None, tags, caps, caplens, encoder_out=enc)
    assert ts.last_mix is None and ts.steps_done == 1
    ts.set_sampling_prob(0.5)
    for draw in (1, 2):
        state = copy.deepcopy(ts.decoder.state_dict())
        ts.step(None, tags, caps, caplens, encoder_out=enc)
        m = _copy(ts, state)
        with torch.no_grad():
            mine = m.mix_batch(wm, enc, tags, caps, caplens, 0.5, seed=77, draw=draw)
            other = m.mix_batch(wm, enc, tags, caps, caplens, 0.5, seed=77, draw=draw - 1)
        assert torch.equal(ts.last_mix["inputs"], mine["inputs"]) and torch.equal(ts.last_mix["replaced"], mine["replaced"])
        assert not torch.equal(ts.last_mix["replaced"], other["replaced"])
    kept = ts.last_mix
    ts.set_sampling_prob(0.0)
    ts.step(None, tags, caps, caplens, encoder_out=enc)
    assert ts.last_mix is kept and ts.steps_done == 4   # a plain step leaves the record of the last mixed one alone


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from trains.harness import SCSTTrainStep
    from test_gpu_scst_step import _scorer
    kind = "attention_scn"
    d, V = BR.sharpened(FIX[kind])
    with pytest.raises(ValueError, match="scheduled_sampling"):
        SCSTTrainStep(scorer=_scorer(dev, V), scheduled_sampling=0.1, kind=kind, device=dev, encoder=False, **_cfg_of(kind, d))
    ts, V, enc, tags, caps, caplens = _step_object(kind, dev, scheduled_sampling=0.25)
    before = [p.detach().clone() for p in ts.decoder.parameters()]
    with pytest.raises(ValueError, match="prepool"):
        ts.step(None, tags, caps, caplens, prepool=enc)
    assert ts.steps_done == 0 and all(torch.equal(x, p) for x, p in zip(before, ts.decoder.parameters()))
