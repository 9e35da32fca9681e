"""GPU tests (``-m gpu``) of scnattn.tagmetrics.TagScorer and of the tagger validation / evaluation loops of trains/harness.py,
judged by the exact restatement of tests/tagmetrics_refs.py (its bounds; integers equal).

1. TagScorer end to end on synthetic probabilities: S = 1000, 70 images in batches of 32 + 32 + 6, about 1 % positives, two
   thresholds; the dict, per_image() and per_tag(); bool targets; a column slice of a wider tensor as probs; reset(); the
   ValueErrors (past the capacity, a bad score, nothing accumulated).
2. validate_tagger(..., scorer=) on a small EncoderTagger (one Bottleneck per stage, 64 x 64 images, semantic_size = 100, B = 2,
   three batches, the last one short): the accuracy meter and the losses are those of the call without a scorer, bit for bit;
   scorer.result() is the restatement on the probabilities encoder(imgs) returns for the same batches; binary_accuracy is
   100 * sum(agree) / (n * S) exactly.  evaluate_tagger returns the same dict."""
import numpy as np
import pytest
import torch

import tagmetrics_refs as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def judge_scorer(sc, res, probs, targets):
    """the dict, per_image() and per_tag() of a TagScorer against the restatement on (probs, targets) as numpy arrays"""
    ks, th = sc.ks, sc.thresholds
    ref = T.reference(probs, targets, ks, th)
    pi, pt = sc.per_image(), sc.per_tag()
    v = np.zeros(T.SUMMARY_LEN)
    v[0], v[1] = res["map_tags"], res["ap_images"]
    for q, k in enumerate(ks):
        v[2 + q], v[6 + q] = res["precision_at"][k], res["recall_at"][k]
    for t, x in enumerate(th):
        d = res["threshold_%g" % x]
        v[10 + 6 * t:16 + 6 * t] = [d["micro_precision"], d["micro_recall"], d["micro_f1"], d["macro_precision"], d["macro_recall"],
                                    d["macro_f1"]]
    v[58], v[59], v[60], v[61] = res["binary_accuracy"], res["n_images"], res["n_images_empty"], res["n_tags_empty"]
    assert isinstance(res["n_images"], int) and isinstance(res["n_tags_empty"], int) and isinstance(res["map_tags"], float)
    counts = torch.stack([pt["tp"], pt["fp"], pt["fn"]], dim=-1).cpu().numpy()
    got = dict(row_ap=pi["ap"].cpu().numpy(), row_npos=pi["npos"].cpu().numpy(), row_hits=pi["hits"].cpu().numpy(),
               col_ap=pt["ap"].cpu().numpy(), col_npos=pt["npos"].cpu().numpy(), col_counts=counts,
               col_agree=ref["col_agree"], summary=v)
    assert pi["ap"].is_cuda and pt["tp"].is_cuda
    bad = T.judge(got, ref, len(ks), len(th))
    assert not bad, bad[:8]
    return ref


def test_tagscorer_end_to_end(dev):
    from scnattn.tagmetrics import TagScorer
    rng = np.random.default_rng(5)
    n, S = 70, 1000
    p, t = T._random(rng, n, S, rate=0.01)
    p[t != 0] = np.sqrt(p[t != 0])                                      # a tagger better than chance
    t[11] = 0                                                           # an image without a tag
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    sc = TagScorer(S, 80, thresholds=(0.5, 0.3), device=dev)
    assert sc.ks == (1, 5, 10, 20)
    with pytest.raises(ValueError):
        sc.result()                                                     # nothing accumulated
    for a, b in ((0, 32), (32, 64), (64, 70)):
        sc.update(pd[a:b], td[a:b])
    res = sc.result()
    ref = judge_scorer(sc, res, p, t)
    assert res["n_images"] == 70 and res["n_images_empty"] >= 1 and res == sc.result()
    assert res["map_tags"] > 0.05 and res["binary_accuracy"] == ref["binary_accuracy"]
    with pytest.raises(ValueError):
        sc.update(pd[:11], td[:11])                                     # 70 + 11 > 80
    assert sc.n == 70 and sc.result() == res
    # bool and fp32 targets, and probs as a column slice of a wider tensor: the same bits
    wide = torch.full((n, S + 24), 7.0, device=dev)
    wide[:, 8:8 + S] = pd
    for targets in (td.bool(), td.float()):
        sc2 = TagScorer(S, 70, thresholds=(0.5, 0.3), device=dev)
        sc2.update(wide[:40, 8:8 + S], targets[:40])
        sc2.update(wide[40:, 8:8 + S], targets[40:])
        assert sc2.result() == res
        assert torch.equal(sc2.per_image()["ap"], sc.per_image()["ap"]) and torch.equal(sc2.per_tag()["ap"], sc.per_tag()["ap"])
    # reset, then other images
    sc.reset()
    sc.update(pd[:5], td[:5])
    judge_scorer(sc, sc.result(), p[:5], t[:5])
    # a bad score raises at result(), and reset() clears it
    bad = pd[:5].clone()
    bad[2, 999] = float("nan")
    sc.update(bad, td[:5])
    with pytest.raises(ValueError, match="finite"):
        sc.result()
    sc.reset()
    sc.update(pd[:5], td[:5])
    assert sc.result()["n_images"] == 5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.update(pd[:5].cpu(), td[:5].cpu())
    with pytest.raises(ValueError):
        sc.update(pd[:5, :999], td[:5, :999])


@pytest.fixture(scope="module")
def tagger(dev):
    """EncoderTagger on a one-block-per-stage trunk, and three batches of 64 x 64 images: 2 + 2 + 1"""
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    torch.manual_seed(3)
    S = 100
    m = EncoderTagger(semantic_size=S, channels_last=True)
    m.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    with torch.no_grad():
        m.linear.weight.mul_(10.0)                                      # spread the probabilities away from 0.5
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(b, 3, 64, 64, generator=g).to(dev), (torch.rand(b, S, generator=g) < 0.1).float().to(dev))
               for b in (2, 2, 1)]
    return m.to(dev), batches


def test_validate_tagger_with_a_scorer(dev, tagger):
    from scnattn.tagmetrics import TagScorer
    from trains.harness import evaluate_tagger, validate_tagger
    from utils.metric import AverageMeter
    m, batches = tagger
    S, n = 100, 5
    plain_l = AverageMeter()
    plain = validate_tagger(batches, m, losses=plain_l)
    sc = TagScorer(S, n, device=dev)
    with_l = AverageMeter()
    accs = validate_tagger(batches, m, losses=with_l, scorer=sc)
    assert not m.training
    assert (accs.val, accs.avg, accs.sum, accs.count) == (plain.val, plain.avg, plain.sum, plain.count) and accs.count == 3
    assert (with_l.val, with_l.avg, with_l.sum, with_l.count) == (plain_l.val, plain_l.avg, plain_l.sum, plain_l.count)
    res = sc.result()
    with torch.no_grad():
        probs = torch.cat([m(im) for im, _ in batches]).cpu().numpy()
        fused = torch.cat([m.tag_loss(im, tg)[0] for im, tg in batches]).cpu().numpy()
        agree = sum(int(m.tag_loss(im, tg)[2].item()) for im, tg in batches)
    tags = torch.cat([tg for _, tg in batches]).cpu().numpy()
    print("probabilities: forward() vs tag_loss() differ by at most %.3e; closest to 0.5: %.3e; closest pair in a row: %.3e"
          % (np.abs(probs - fused).max(), np.abs(probs - 0.5).min(), np.diff(np.sort(probs, axis=1), axis=1).min()))
    judge_scorer(sc, res, probs, tags)
    assert res["binary_accuracy"] == 100.0 * agree / (n * S) and res["n_images"] == n
    ev = evaluate_tagger(batches, m)
    assert ev == res
    assert evaluate_tagger(iter(batches), m, capacity=n) == res
