"""GPU tests (``-m gpu``) of the tagger loss family above the kernels: scnattn.functional.tag_head_loss(loss=TagLoss) against
the fp64 head reference (tagloss_refs.head_ref: taghead_refs.head_ref restated with the new term), loss=None and the identity
TagLoss against the call without the argument, one TaggerTrainStep under the asymmetric loss with the prior bias, and
validate_tagger under a loss.

Bars of the head, those of tests/test_gpu_tagger_step.py: probabilities and loss 1e-4 (max-norm relative), dW / db / the fp32
map gradient 2e-4 relative l2, the bf16 map gradient 5e-3; the agreement count exact on logits kept 1 away from 0 (asserted
on the fp64 side, as are max|z| <= 8 and, under a margin, |p - m| >= 1e-3 for every element).
The step's loss: against the fp64 recomputation from the step's own logits, within the kernel test's row-sum bound
((S + 8) 2^-24 + 4 yard) sum|parts| / (B S) plus the finalize's (B + 8) 2^-24 sum|row| / (B S)."""
import copy

import pytest
import torch

import tagloss_refs as R
from helpers import rel_err, rel_l2
from kernel_harness import U

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
KEEP = 1.0 / 0.85
# (gamma_pos, gamma_neg, margin, with weights): weighted BCE, focal, the asymmetric default, everything at once
_LOSSES = ((0.0, 0.0, 0.0, True), (2.0, 2.0, 0.0, False), (0.0, 4.0, 0.05, False), (1.0, 4.0, 0.05, True))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


_cache = {}


def _head_inputs(bf16):
    """a (3, 2048, 2, 2) map, a keep mask, W, b, targets and weights for 37 tags.  Channel 0 carries s_i r_j 4 into every logit,
    the other channels at most 2, the bias at most 1: 1 <= |z| <= 7 (test_gpu_tagger_step._head_case's construction)"""
    if bf16 in _cache:
        return _cache[bf16]
    B, H, Wd, C, S = 3, 2, 2, 2048, 37
    g = torch.Generator().manual_seed(24)
    x4 = torch.randn(B, C, H, Wd, generator=g)
    sgn_i = (torch.rand(B, generator=g) >= 0.5).float() * 2 - 1
    sgn_j = (torch.rand(S, generator=g) >= 0.5).float() * 2 - 1
    x4[:, 0] = sgn_i.view(B, 1, 1)
    if bf16:
        x4 = x4.to(BF).float()
    ks = (torch.rand(B, C, generator=g) >= 0.15).float() * torch.tensor(KEEP)
    ks[:, 0] = KEEP
    W = torch.randn(S, C, generator=g)
    W[:, 0] = 0.0
    b = torch.rand(S, generator=g) * 2 - 1
    t = (torch.rand(B, S, generator=g) >= 0.5).float()
    t = torch.where(torch.rand(B, S, generator=g) < 0.1, torch.rand(B, S, generator=g), t)
    w = (1.0 + 9.0 * torch.rand(S, generator=g)).float()
    w[0], w[1] = 0.0, 99.0
    xd = x4.double().mean(dim=(2, 3)) * ks.double()
    W = (W.double() * (2.0 / float((xd @ W.double().t()).abs().max()))).float()
    W[:, 0] = sgn_j * 4.0 / float(xd[0, 0].abs())
    _cache[bf16] = (x4, ks, W, b, t, w)
    return _cache[bf16]


def _head_ref(bf16, setting):
    key = (bf16, setting)
    if key not in _cache:
        x4, ks, W, b, t, w = _head_inputs(bf16)
        gp, gn, m, weights = setting
        B, C, H, Wd = x4.shape
        r = R.head_ref(x4.permute(0, 2, 3, 1).reshape(B, H * Wd, C), ks, W, b, t, w if weights else None, gp, gn, m)
        assert 1.0 - 1e-6 <= float(r["z"].abs().min()) and float(r["z"].abs().max()) <= 8.0
        if m > 0:
            assert float((r["probs"] - R.f32(m)).abs().min()) >= 1e-3, "a probability within 1e-3 of the margin"
        r["dx"] = r["dx"].reshape(B, H, Wd, C).permute(0, 3, 1, 2)
        _cache[key] = r
    return _cache[key]


def _tagloss(dev, setting, w):
    from scnattn.functional import TagLoss
    gp, gn, m, weights = setting
    return TagLoss(w.to(dev) if weights else None, gp, gn, m)


@pytest.mark.parametrize("setting", _LOSSES, ids=[R.setting_id(s) for s in _LOSSES])
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_tag_head_loss_under_a_tagloss_vs_fp64(dev, monkeypatch, bf16, setting):
    from scnattn import functional as SF
    x4, ks, W, b, t, w = _head_inputs(bf16)
    ref = _head_ref(bf16, setting)
    launched = []
    real = SF.call
    monkeypatch.setattr(SF, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    x = x4.to(dev, dtype=BF if bf16 else torch.float32).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    Wg, bg = W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    probs, loss, agree = SF.tag_head_loss(x, ks.to(dev), Wg, bg, t.to(dev), loss=_tagloss(dev, setting, w))
    assert loss.dim() == 0 and agree.dim() == 0 and not probs.requires_grad
    loss.backward()
    e = dict(probs=rel_err(probs, ref["probs"]), loss=rel_err(loss, ref["loss"]), dW=rel_l2(Wg.grad, ref["dW"]),
             db=rel_l2(bg.grad, ref["db"]), dx=rel_l2(x.grad.float(), ref["dx"]))
    print("tag_head_loss %s %s: %s  agree %d / %d" % (R.setting_id(setting), "bf16" if bf16 else "f32",
                                                       "  ".join("%s %.3e" % kv for kv in e.items()), int(agree), ref["agree"]))
    assert e["probs"] <= 1e-4 and e["loss"] <= 1e-4, e
    assert e["dW"] <= 2e-4 and e["db"] <= 2e-4, e
    assert e["dx"] <= (5e-3 if bf16 else 2e-4), e
    assert int(agree) == ref["agree"] and x.grad.dtype == x.dtype
    assert launched.count("scnattn_tagloss_fwd") == 1 and launched.count("scnattn_tagloss_bwd") == 1
    assert "scnattn_bce_fwd" not in launched and "scnattn_bce_bwd" not in launched


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_default_and_identity_are_the_bce_path_bit_for_bit(dev, monkeypatch, bf16):
    from scnattn import functional as SF
    x4, ks, W, b, t, _ = _head_inputs(bf16)
    launched = []
    real = SF.call
    monkeypatch.setattr(SF, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])

    def run(**kw):
        x = x4.to(dev, dtype=BF if bf16 else torch.float32).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        Wg, bg = W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        probs, loss, agree = SF.tag_head_loss(x, ks.to(dev), Wg, bg, t.to(dev), pooled_bf16=bf16, **kw)
        loss.backward()
        return probs, loss.detach(), agree, x.grad, Wg.grad, bg.grad

    base = run()
    for kw in (dict(loss=None), dict(loss=SF.TagLoss()), dict(loss=SF.TagLoss(None, 0.0, 0.0, 0.0))):
        for u, v in zip(base, run(**kw)):
            assert torch.equal(u, v)
    assert launched.count("scnattn_bce_fwd") == 4 and launched.count("scnattn_bce_bwd") == 4
    assert not [n for n in launched if "tagloss" in n]
    # ... and another loss leaves the probabilities and the count as they are, bit for bit
    other = run(loss=SF.TagLoss.asl())
    assert torch.equal(other[0], base[0]) and torch.equal(other[2], base[2]) and not torch.equal(other[1], base[1])


S_STEP = 50


@pytest.fixture(scope="module")
def base():
    """EncoderTagger on a one-block-per-stage trunk, a batch of 4 images of 64 x 64 (tests/test_gpu_tagger_step.py's size) and a
    long-tailed target matrix of 200 rows for the prior"""
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    torch.manual_seed(3)
    m = EncoderTagger(semantic_size=S_STEP, channels_last=True)
    m.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    prior = 0.5 / (1.0 + torch.arange(S_STEP).float())
    corpus = (torch.rand(200, S_STEP, generator=g) < prior).float()
    return m, imgs, corpus[:4].clone(), corpus


def test_step_under_asl_with_prior_bias(dev, base, monkeypatch):
    from scnattn import functional as SF
    from trains.harness import TaggerTrainStep
    m0, imgs, tags, corpus = base
    logits = []
    real = SF.gemm

    def gemm(*a, **kw):
        out = real(*a, **kw)
        if kw.get("bias") is not None and tuple(out.shape) == (4, S_STEP):
            logits.append(out.detach().clone())
        return out

    monkeypatch.setattr(SF, "gemm", gemm)
    loss = SF.TagLoss.asl()
    ts = TaggerTrainStep(device=dev, encoder=copy.deepcopy(m0), semantic_size=S_STEP, encoder_lr=1e-2, loss=loss,
                         prior_bias_from=corpus.to(dev))
    want_bias = SF.prior_bias(corpus)
    n = (corpus >= 0.5).sum(0).double()
    assert torch.allclose(want_bias.double(), torch.log((n + 1.0) / (200.0 - n + 1.0)), rtol=1e-6, atol=0)
    assert torch.equal(ts.encoder.linear.bias.detach().cpu(), want_bias)
    imgs, tags = imgs.to(dev), tags.to(dev)
    before = ts.encoder.linear.weight.detach().clone()
    got = [ts.step(imgs, tags) for _ in range(2)]
    torch.cuda.synchronize()
    assert len(logits) == 2 and not torch.equal(before, ts.encoder.linear.weight.detach())
    B, S = tags.shape
    for (l, agree), z in zip(got, logits):
        assert bool(torch.isfinite(l.detach())) and 0 <= int(agree) <= B * S
        zc, tc = z.cpu(), tags.cpu()
        r = R.fwd_ref(zc, tc, None, 0.0, 4.0, 0.05)
        yard = R.yard_terms(zc, tc, None, 0.0, 4.0, 0.05)
        bound = (((S + 8) * U + 4.0 * yard) * float(r["rows_abs"].sum()) + (B + 8) * U * float(r["rows"].abs().sum())) / (B * S)
        err = abs(float(l.detach()) - float(r["loss"]))
        print("step loss %.8f, fp64 from the step's logits %.8f: err %.3e, bound %.3e (yard %.3e)" % (float(l.detach()), float(r["loss"]),
                                                                                                     err, bound, yard))
        assert err <= bound
        assert int(agree) == int(((torch.sigmoid(zc.double()) >= 0.5) == (tc >= 0.5)).sum()) or float(zc.abs().min()) < 1e-4
    assert float(got[1][0].detach()) != float(got[0][0].detach())


def test_validate_tagger_under_a_loss(dev, base):
    from scnattn import functional as SF
    from scnattn.tagmetrics import TagScorer
    from trains.harness import validate_tagger
    from utils.metric import AverageMeter
    m0, imgs, tags, corpus = base
    m = copy.deepcopy(m0).to(dev)
    g = torch.Generator().manual_seed(9)
    batches = [(imgs.to(dev), tags.to(dev)), (torch.randn(4, 3, 64, 64, generator=g).to(dev), corpus[4:8].to(dev))]
    l0, l1 = AverageMeter(), AverageMeter()
    a0 = validate_tagger(batches, m, losses=l0)
    scorer = TagScorer(S_STEP, 8, device=dev)
    loss = SF.TagLoss.balanced(corpus.to(dev), gamma_neg=2.0, gamma_pos=1.0)
    a1 = validate_tagger(batches, m, losses=l1, scorer=scorer, loss=loss)
    assert not m.training and a0.count == a1.count == 2 and a0.avg == a1.avg and a0.sum == a1.sum
    assert l1.count == 2 and l1.avg > 0 and l1.avg != l0.avg
    res = scorer.result()
    assert res is not None
    # the validation loss is the fp64 loss of the module path's logits under the same TagLoss
    want = []
    with torch.no_grad():
        for im, tg in batches:
            p = m(im).double().cpu()
            z = torch.log(p) - torch.log1p(-p)
            want.append(float(R.fwd_ref(z, tg.cpu(), loss.pos_weight.cpu(), 1.0, 2.0, 0.0)["loss"]))
    assert abs(l1.avg - sum(want) / 2) <= 1e-4 * abs(sum(want) / 2)
