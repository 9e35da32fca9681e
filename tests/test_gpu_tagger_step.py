"""GPU tests (``-m gpu``) of the tagger step: scnattn.functional.tag_head_loss against the fp64 CPU composition
adaptive_avg_pool2d -> * ks -> linear -> sigmoid -> binary_cross_entropy and its autograd; one TaggerTrainStep.step against
the module path (EncoderTagger.forward + nn.BCELoss + backward + the same FusedClampAdam); learning on one batch;
validate_tagger against the reference's loop.

Bars: probabilities and loss 1e-4 (max-norm relative), dW / db / the fp32 map gradient 2e-4 relative l2 (the project's
module-level bars), the bf16 map gradient 5e-3 (its bar for bf16 maps); the agreement count exact on logits kept away from 0
(asserted on the fp64 side, as is max|z| <= 8).

Under bf16 autocast the module path's own AdaptiveAvgPool2d runs in bf16 and hands its mean on rounded to bf16;
EncoderTagger.tag_loss asks the head for the same (tag_head_loss(pooled_bf16=True), scnattn_tag_pool_fwd bf16 = 2), so
the two bf16 paths see the same pooled vector.  Without that rounding the fused head is closer to fp64 and 5.9e-4
(probabilities) / 1.8e-3 (dW) away from the module path, measured on an MI355X."""
import copy

import pytest
import torch
from torch import nn

from helpers import rel_err, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
KEEP = 1.0 / 0.85


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- head against fp64 --------------------------------------------------------------------------------------------------
_HEAD_SIZES = {"small": (3, 2, 2, 64, 37), "full": (32, 8, 8, 2048, 1000)}      # B, H, W, C, S
_head_cache = {}


def _head_case(size, bf16, with_ks):
    """inputs and the fp64 result, computed once per case.  Channel 0 carries s_i * r_j * 4 into every logit (s, r = +-1),
    the other channels at most 2, the bias at most 1: 1 <= |z| <= 7, so no probability is near 0.5 and none saturates."""
    key = (size, bf16, with_ks)
    if key in _head_cache:
        return _head_cache[key]
    B, H, Wd, C, S = _HEAD_SIZES[size]
    g = torch.Generator().manual_seed(11 + B)
    x4 = torch.randn(B, C, H, Wd, generator=g)
    sgn_i = (torch.rand(B, generator=g) >= 0.5).float() * 2 - 1
    sgn_j = (torch.rand(S, generator=g) >= 0.5).float() * 2 - 1
    x4[:, 0] = sgn_i.view(B, 1, 1)
    if bf16:
        x4 = x4.to(BF).float()
    ks = None
    if with_ks:
        ks = (torch.rand(B, C, generator=g) >= 0.15).float() * torch.tensor(KEEP)
        ks[:, 0] = KEEP
    W = torch.randn(S, C, generator=g)
    W[:, 0] = 0.0
    b = torch.rand(S, generator=g) * 2 - 1
    t = (torch.rand(B, S, generator=g) >= 0.5).float()
    t = torch.where(torch.rand(B, S, generator=g) < 0.1, torch.rand(B, S, generator=g), t)
    xd = x4.double().mean(dim=(2, 3)) * (1.0 if ks is None else ks.double())
    W = (W.double() * (2.0 / float((xd @ W.double().t()).abs().max()))).float()
    W[:, 0] = sgn_j * 4.0 / float(xd[0, 0].abs())
    # the fp64 composition of the functions the reference calls, and its autograd
    x64 = x4.double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
    p64 = torch.nn.functional.adaptive_avg_pool2d(x64, 1).flatten(1)
    p64 = p64 if ks is None else p64 * ks.double()
    z = torch.nn.functional.linear(p64, W64, b64)
    probs = torch.sigmoid(z)
    loss = torch.nn.functional.binary_cross_entropy(probs, t.double())
    loss.backward()
    assert float(z.abs().max()) <= 8.0, float(z.abs().max())
    assert float((probs - 0.5).abs().min()) >= 1e-3, "a probability within 1e-3 of 0.5: the agreement count is not decided"
    ref = dict(probs=probs.detach(), loss=loss.detach(), dx=x64.grad, dW=W64.grad, db=b64.grad,
               agree=int(((probs >= 0.5) == (t.double() >= 0.5)).sum()))
    _head_cache[key] = (x4, ks, W, b, t, ref)
    return _head_cache[key]


@pytest.mark.parametrize("need_dx", (True, False), ids=("dx", "nodx"))
@pytest.mark.parametrize("with_ks", (True, False), ids=("ks", "noks"))
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("size", ("small", "full"))
def test_tag_head_loss_vs_fp64(dev, monkeypatch, size, bf16, with_ks, need_dx):
    from scnattn import functional as SF
    x4, ks, W, b, t, ref = _head_case(size, bf16, with_ks)
    launched = []
    real = SF.call
    monkeypatch.setattr(SF, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    x = x4.to(dev, dtype=BF if bf16 else torch.float32)
    if size == "full":
        x = x.contiguous(memory_format=torch.channels_last)        # the layout the trunk returns: the vector kernels
    x.requires_grad_(need_dx)
    handed = []                 # the gradient as the head hands it over (a leaf's .grad is re-laid out to the leaf's own strides)
    if need_dx:
        x.register_hook(lambda g_: handed.append((g_.dtype, g_.is_contiguous(memory_format=torch.channels_last))))
    Wg, bg = W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    probs, loss, agree = SF.tag_head_loss(x, None if ks is None else ks.to(dev), Wg, bg, t.to(dev))
    assert loss.dim() == 0 and agree.dim() == 0 and loss.is_cuda and agree.is_cuda and not probs.requires_grad
    loss.backward()
    e = dict(probs=rel_err(probs, ref["probs"]), loss=rel_err(loss, ref["loss"]), dW=rel_l2(Wg.grad, ref["dW"]),
             db=rel_l2(bg.grad, ref["db"]))
    if need_dx:
        assert handed == [(x.dtype, True)] and x.grad.dtype == x.dtype
        e["dx"] = rel_l2(x.grad.float(), ref["dx"])
    print("tag_head_loss %s %s: %s  agree %d / %d" % (size, "bf16" if bf16 else "f32",
                                                       "  ".join("%s %.3e" % kv for kv in e.items()), int(agree), ref["agree"]))
    assert e["probs"] <= 1e-4 and e["loss"] <= 1e-4, e
    assert e["dW"] <= 2e-4 and e["db"] <= 2e-4, e
    assert int(agree) == ref["agree"]
    if need_dx:
        assert e["dx"] <= (5e-3 if bf16 else 2e-4), e
        assert launched.count("scnattn_tag_pool_bwd") == 1
    else:
        assert x.grad is None and "scnattn_tag_pool_bwd" not in launched
    assert launched.count("scnattn_tag_pool_fwd") == 1 and launched.count("scnattn_bce_fwd") == 1


def test_tag_head_loss_reads_any_strides(dev):
    """a map whose pixels have no common stride (a cropped NCHW window) is served, and equals its dense copy bit for bit"""
    from scnattn import functional as SF
    g = torch.Generator().manual_seed(2)
    big = torch.randn(2, 8, 5, 6, generator=g).to(dev)
    W, b, t = torch.randn(3, 8, generator=g).to(dev), torch.randn(3, generator=g).to(dev), torch.rand(2, 3, generator=g).to(dev)
    win = big[:, :, 1:4, 2:5]
    with torch.no_grad():
        a = SF.tag_head_loss(win, None, W, b, t)
        c = SF.tag_head_loss(win.contiguous(memory_format=torch.channels_last), None, W, b, t)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


# ---- one step against the module path -------------------------------------------------------------------------------------
class _FixedMask(nn.Module):
    """Stands in for nn.Dropout with a pinned, pre-scaled mask so both sides drop the same features."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.device)


S_STEP = 50


@pytest.fixture(scope="module")
def base():
    """EncoderTagger on a one-block-per-stage trunk, its pinned keep mask, and a batch of 4 images of 64 x 64"""
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    torch.manual_seed(3)
    m = EncoderTagger(semantic_size=S_STEP, channels_last=True)
    m.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    g = torch.Generator().manual_seed(4)
    m.dropout = _FixedMask((torch.rand(4, 2048, generator=g) >= 0.15).float() * KEEP)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    tags = (torch.rand(4, S_STEP, generator=g) >= 0.5).float()
    return m, imgs, tags


def _module_step(m, imgs, tags, bf16, lr=1e-4):
    """the path before the fused head: forward() + nn.BCELoss + backward + the same FusedClampAdam"""
    from utils.optimizer import FusedClampAdam
    opt = FusedClampAdam(filter(lambda p: p.requires_grad, m.parameters()), lr=lr, grad_clip=5.0)
    m.train()
    with torch.autocast("cuda", dtype=BF, enabled=bf16):
        probs = m(imgs)
    loss = nn.BCELoss()(probs, tags)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return probs.detach(), loss.detach()


@pytest.mark.parametrize("fine_tune", (False, True), ids=("frozen", "finetune"))
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_step_vs_module_path(dev, base, bf16, fine_tune):
    from trains.harness import TaggerTrainStep
    m0, imgs, tags = base
    imgs, tags = imgs.to(dev), tags.to(dev)
    ma, mb = copy.deepcopy(m0), copy.deepcopy(m0).to(dev)
    ts = TaggerTrainStep(fine_tune_encoder=fine_tune, device=dev, encoder=ma, encoder_dtype="bf16" if bf16 else "f32",
                         semantic_size=S_STEP)
    mb.fine_tune(fine_tune)
    loss_a, agree = ts.step(imgs, tags)
    probs_b, loss_b = _module_step(mb, imgs, tags, bf16)
    torch.cuda.synchronize()
    e_loss, e_probs = rel_err(loss_a, loss_b), rel_err(ts.probs, probs_b)
    print("step %s %s: loss %.6f vs %.6f (%.3e)  probs %.3e" % ("bf16" if bf16 else "f32", "finetune" if fine_tune else "frozen",
                                                                 float(loss_a), float(loss_b), e_loss, e_probs))
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    ga = {k: rel_l2(p.grad, pb[k].grad) for k, p in pa.items() if p.requires_grad}
    worst = max(ga, key=ga.get)
    print("  gradients: %d tensors, worst rel l2 %.3e (%s); linear.weight %.3e linear.bias %.3e"
          % (len(ga), ga[worst], worst, ga["linear.weight"], ga["linear.bias"]))
    pe = {k: rel_l2(p.detach(), pb[k].detach()) for k, p in pa.items() if p.requires_grad}
    print("  parameters after the step: worst rel l2 %.3e" % max(pe.values()))
    assert int(agree) == int(((probs_b >= 0.5) == (tags >= 0.5)).sum()) or float((probs_b - 0.5).abs().min()) < 1e-3
    assert e_loss <= 1e-4 and e_probs <= 1e-4, (e_loss, e_probs)
    assert ga[worst] <= 2e-4, (worst, ga[worst])
    trunk_trained = [k for k in ga if k.startswith("resnet.")]
    if fine_tune:
        kids = {"resnet.%d." % i for i in range(5, 8)}
        assert trunk_trained and all(any(k.startswith(c) for c in kids) for k in trunk_trained)
    else:
        assert not trunk_trained
        assert all(p.grad is None for k, p in pa.items() if k.startswith("resnet."))
        for (k, u), (_, v) in zip(ma.named_buffers(), mb.named_buffers()):
            assert torch.equal(u, v), "%s differs from the module path's" % k       # train-mode statistics, bit for bit
        assert any(k.endswith("running_var") and float((u - 1).abs().max()) > 0 for k, u in ma.named_buffers())
        assert max(pe.values()) <= 2e-4


def test_step_learns(dev, base):
    from trains.harness import TaggerTrainStep
    m0, imgs, tags = base
    ts = TaggerTrainStep(device=dev, encoder=copy.deepcopy(m0), semantic_size=S_STEP, encoder_lr=1e-2)
    imgs, tags = imgs.to(dev), tags.to(dev)
    losses = [float(ts.step(imgs, tags)[0]) for _ in range(10)]
    print("loss over 10 steps on one batch:", " ".join("%.4f" % v for v in losses))
    assert losses[9] < losses[0]


def test_validate_tagger(dev, base):
    from trains.harness import validate_tagger
    from utils.metric import AverageMeter, binary_accuracy
    m0, imgs, tags = base
    m = copy.deepcopy(m0)
    m.dropout = nn.Dropout(0.15)        # the pinned mask of `base` multiplies in eval mode too; nn.Dropout is the identity there
    m = m.to(dev)
    g = torch.Generator().manual_seed(9)
    batches = [(imgs.to(dev), tags.to(dev)),
               (torch.randn(4, 3, 64, 64, generator=g).to(dev), (torch.rand(4, S_STEP, generator=g) >= 0.5).float().to(dev))]
    losses = AverageMeter()
    accs = validate_tagger(batches, m, losses=losses)
    assert not m.training
    # the reference's loop (trains/tagger.py:206-233) on the module path
    ref_l, ref_a = AverageMeter(), AverageMeter()
    with torch.no_grad():
        for im, tg in batches:
            scores = m(im)
            ref_l.update(nn.BCELoss()(scores, tg).item())
            ref_a.update(float(binary_accuracy(scores, tg)))
    print("validate_tagger: loss %.6f vs %.6f, accuracy %.4f vs %.4f" % (losses.avg, ref_l.avg, accs.avg, ref_a.avg))
    assert accs.count == ref_a.count == 2 and losses.count == ref_l.count == 2
    assert abs(losses.avg - ref_l.avg) <= 1e-4 * abs(ref_l.avg)
    assert abs(accs.avg - ref_a.avg) <= 100.0 / (4 * S_STEP) + 1e-9
