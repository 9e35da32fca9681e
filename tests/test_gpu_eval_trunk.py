"""GPU tests (``-m gpu``) of the eval-mode trunk on the hand-written kernels: the eval BatchNorm epilogue of
csrc/cgemm.hip (EPI 3) through the C ABI against fp64 torch, the fused eval Bottleneck (scnattn/conv_eval.py) against
the fp64 CPU module, whole EncoderCaption / EncoderTagger in eval mode, grad-enabled eval (the reference's
inference.py), running statistics moved by training steps, validate(), and the fallbacks that keep the module path."""
import copy
import ctypes as C

import pytest
import torch
from torch import nn

from helpers import rel_err, rel_l2

pytestmark = pytest.mark.gpu

_BLOCKS = [  # (name, inplanes, planes, stride, H): the Bottleneck shapes of ResNet-152 at 256 x 256 input
    ("layer1.0", 64, 64, 1, 64), ("layer1.1", 256, 64, 1, 64), ("layer2.0", 256, 128, 2, 64), ("layer2.1", 512, 128, 1, 32),
    ("layer3.0", 512, 256, 2, 32), ("layer3.1", 1024, 256, 1, 16), ("layer4.0", 1024, 512, 2, 16), ("layer4.1", 2048, 512, 1, 8)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


class _ConvCalls:
    """Counts nn.Conv2d forwards (the module path) while active."""

    def __enter__(self):
        self.n = 0
        self._orig = nn.Conv2d._conv_forward
        outer = self

        def counting(mod, x, w, b):
            outer.n += 1
            return outer._orig(mod, x, w, b)
        nn.Conv2d._conv_forward = counting
        return self

    def __exit__(self, *a):
        nn.Conv2d._conv_forward = self._orig


def _bn_stats(C_, g):
    """Non-trivial eval BatchNorm: mean ~ N(0, 0.5), var ~ U(0.5, 2), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.5)."""
    return (torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.5, torch.randn(C_, generator=g) * 0.5,
            torch.rand(C_, generator=g) * 1.5 + 0.5)


def _ref_epilogue(z, gamma, beta, mean, var, eps, res, relu):
    z = z.double()
    sc = gamma.double() / torch.sqrt(var.double() + eps)
    y = z * sc + (beta.double() - mean.double() * sc)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def _bn_struct(L, vecs, eps, res, relu):
    gamma, beta, mean, var = vecs
    return L.BnEval(gamma=gamma.data_ptr(), beta=beta.data_ptr(), mean=mean.data_ptr(), var=var.data_ptr(), eps=eps,
                    res=None if res is None else res.data_ptr(), ldres=0 if res is None else res.shape[1],
                    relu=1 if relu else 0)


def test_bn_eval_epilogue_vs_fp64(dev):
    """scnattn_conv1x1_fwd_bn_eval / scnattn_conv3x3_fwd_bn_eval against fp64 torch: the 1x1 shapes of every Bottleneck
    (conv1; conv3 + residual; the downsample with its strided row gather), an odd shape (rows not a multiple of 64,
    96 -> 80 channels), ReLU on / off with and without the residual, forced split-K 1/2/4/8 (the in-launch combine),
    forced row tiles 1/2/4, and the 3x3 forward at stride 1 and 2 on 8x8, 7x7 and 3x3 maps.  Bar: 3e-6 max-norm
    relative error, the bar the plain products are held to (test_cgemm_variants_vs_fp64)."""
    from scnattn import _lib as L
    h = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = torch.empty(32 << 20, device=dev)
    g = torch.Generator().manual_seed(11)
    eps = 1e-5
    worst = [0.0]

    def run1x1(R, Cin, Cout, relu, with_res, split=0, mi=0, gather=None):
        if gather is not None:
            Nn, Hi, s = gather
            Ho = (Hi - 1) // s + 1
            x = torch.randn(Nn * Hi * Hi, Cin, generator=g)
            xg = x.view(Nn, Hi, Hi, Cin)[:, ::s, ::s].reshape(-1, Cin)
            R = xg.shape[0]
            ex = L.ConvExtra(stride=s, Hi=Hi, Wi=Hi, Ho=Ho, Wo=Ho, force_split=split, force_mi=mi)
        else:
            x = xg = torch.randn(R, Cin, generator=g)
            ex = L.ConvExtra(force_split=split, force_mi=mi)
        w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
        vecs = _bn_stats(Cout, g)
        res = torch.randn(R, Cout, generator=g) if with_res else None
        ref = _ref_epilogue(xg.double() @ w.double().t(), *vecs, eps, res, relu)
        xd, wd = x.to(dev), w.to(dev)
        vd = tuple(v.to(dev) for v in vecs)
        rd = None if res is None else res.to(dev)
        y = torch.full((R, Cout), float("nan"), device=dev)
        bn = _bn_struct(L, vd, eps, rd, relu)
        L.check(h.scnattn_conv1x1_fwd_bn_eval(st, R, Cin, Cout, xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(bn),
                                              C.byref(ex), ws.data_ptr(), ws.numel()), "scnattn_conv1x1_fwd_bn_eval")
        e = rel_err(y, ref)
        worst[0] = max(worst[0], e)
        assert e <= 3e-6, "1x1 R=%d %d->%d relu=%s res=%s split=%d mi=%d gather=%s: %.3e" % (
            R, Cin, Cout, relu, with_res, split, mi, gather, e)

    def run3x3(Nn, Hi, Cin, Cout, s, relu, with_res, split=0, mi=0):
        Ho = (Hi - 1) // s + 1
        x = torch.randn(Nn, Cin, Hi, Hi, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        vecs = _bn_stats(Cout, g)
        R = Nn * Ho * Ho
        res = torch.randn(R, Cout, generator=g) if with_res else None
        z = torch.nn.functional.conv2d(x.double(), w.double(), stride=s, padding=1).permute(0, 2, 3, 1).reshape(R, Cout)
        ref = _ref_epilogue(z, *vecs, eps, res, relu)
        xd = x.to(dev).contiguous(memory_format=torch.channels_last)
        wd = w.to(dev).contiguous(memory_format=torch.channels_last)
        vd = tuple(v.to(dev) for v in vecs)
        rd = None if res is None else res.to(dev)
        y = torch.full((R, Cout), float("nan"), device=dev)
        bn = _bn_struct(L, vd, eps, rd, relu)
        ex = L.ConvExtra(force_split=split, force_mi=mi)
        L.check(h.scnattn_conv3x3_fwd_bn_eval(st, Nn, Hi, Hi, Cin, Cout, s, xd.data_ptr(), wd.data_ptr(), y.data_ptr(),
                                              C.byref(bn), C.byref(ex), ws.data_ptr(), ws.numel()),
                "scnattn_conv3x3_fwd_bn_eval")
        e = rel_err(y, ref)
        worst[0] = max(worst[0], e)
        assert e <= 3e-6, "3x3 %dx%d s=%d %d->%d relu=%s res=%s split=%d mi=%d: %.3e" % (
            Hi, Hi, s, Cin, Cout, relu, with_res, split, mi, e)

    Nb = 2
    for name, cin, p, s, H in _BLOCKS:
        Ho = (H - 1) // s + 1
        run1x1(Nb * H * H, cin, p, True, False)                        # conv1
        run1x1(Nb * Ho * Ho, p, 4 * p, True, True)                     # conv3 + residual
        if s != 1 or cin != 4 * p:                                     # downsample (rows gathered at stride 2)
            run1x1(0, cin, 4 * p, False, False, gather=(Nb, H, s))
    run1x1(1000, 96, 80, True, True)                                   # odd rows / columns
    run1x1(1000, 96, 80, False, True)
    run1x1(1000, 96, 80, True, False)
    run1x1(1000, 96, 80, False, False)
    for split in (1, 2, 4, 8):                                         # in-launch split-K combine
        run1x1(512, 1024, 256, True, True, split=split)
        run1x1(1000, 512, 80, False, True, split=split)
    for mi in (1, 2, 4):
        run1x1(1000, 96, 80, True, True, mi=mi)
        run1x1(4096, 256, 64, True, False, mi=mi)
    run1x1(0, 64, 128, False, False, gather=(2, 7, 2))                 # gather on an odd map
    run1x1(0, 256, 512, True, True, gather=(3, 9, 2), split=4)
    for Hi in (8, 7, 3):
        for s in (1, 2):
            run3x3(2, Hi, 64, 64, s, True, False)
            run3x3(2, Hi, 128, 128, s, False, True)
    for split in (2, 4):
        run3x3(2, 8, 64, 64, 1, True, True, split=split)
        run3x3(2, 7, 128, 128, 2, True, False, split=split)
    for mi in (1, 2, 4):
        run3x3(2, 7, 64, 64, 1, True, True, mi=mi)
    torch.cuda.synchronize()
    print("bn_eval epilogue worst rel_err %.3e" % worst[0])


def _make_block(inplanes, planes, stride, seed):
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    torch.manual_seed(seed)
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                             FusedBatchNorm2d(planes * 4))
    m = Bottleneck(inplanes, planes, stride, down)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(mod, nn.BatchNorm2d):
            ga, be, mu, va = _bn_stats(mod.num_features, g)
            with torch.no_grad():
                mod.weight.copy_(ga)
                mod.bias.copy_(be)
                mod.running_mean.copy_(mu)
                mod.running_var.copy_(va)
    return m.eval()


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("name,inplanes,planes,stride,H", _BLOCKS)
def test_fused_eval_bottleneck_vs_fp64(dev, name, inplanes, planes, stride, H, channels_last):
    """One eval-mode Bottleneck through scnattn/conv_eval.py (3-4 launches, BatchNorm in the epilogues) against the same
    module in fp64 on the CPU: output within 2e-5 (the bar of test_fused_bottleneck_vs_fp64), no nn.Conv2d forward,
    running statistics and num_batches_tracked untouched.  channels_last=False: the module's weights and the input are
    NCHW (the reference's default EncoderCaption()), so conv2's weight takes the transient channels-last copy."""
    from scnattn import conv_eval as CE
    m = _make_block(inplanes, planes, stride, 2000 + [b[0] for b in _BLOCKS].index(name))
    x = torch.relu(torch.randn(2, inplanes, H, H)) + 0.1 * torch.randn(2, inplanes, H, H)
    ref = copy.deepcopy(m).double()
    with torch.no_grad():
        yr = ref(x.double())
    gm = copy.deepcopy(m).to(dev)
    xg = x.to(dev)
    if channels_last:
        gm = gm.to(memory_format=torch.channels_last)
        xg = xg.contiguous(memory_format=torch.channels_last)
    assert CE.eval_reason(gm, xg) is None
    bufs = {k: b.detach().clone() for k, b in gm.named_buffers()}
    with torch.no_grad(), _ConvCalls() as cc:
        y = gm(xg)
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    assert y.shape == yr.shape
    e = rel_err(y, yr)
    assert e <= 2e-5, "%s: rel_err %.3e" % (name, e)
    for k, b in gm.named_buffers():
        assert torch.equal(b, bufs[k]), k


_CALIBRATED = {}


def _calibrated_encoder(channels_last, depths=None, seed=5):
    """EncoderCaption whose running statistics come from one fp64 training-mode forward at momentum=None (the batch
    statistics themselves) on a separate batch: a well-conditioned eval trunk.  Built once per (depths, seed)."""
    key = (depths, seed)
    if key not in _CALIBRATED:
        _CALIBRATED[key] = _calibrate(depths, seed)
    enc = copy.deepcopy(_CALIBRATED[key])
    enc.channels_last = channels_last
    return enc


def _calibrate(depths, seed):
    # The construction of test_gpu_parity_r3.py::test_well_conditioned_trunk_gradients_vs_fp64: perturbations of a randomly
    # initialised 50-block trunk are amplified through 150 layers (measured: 1e-3 rel-l2 of the fp32 trunk map against
    # fp64 with plain calibrated statistics), so the last BatchNorm of every block gets gamma = 0.2
    # (the residual branch is a small correction) and the BatchNorms in front of a ReLU beta = 3.5 (few activations within
    # rounding of the threshold).
    from models.encoders.caption import EncoderCaption
    from scnattn.resnet import resnet152_trunk
    torch.manual_seed(seed)
    enc = EncoderCaption()
    if depths is not None:
        enc.resnet = resnet152_trunk(depths=depths)
        enc.fine_tune()
    with torch.no_grad():
        for name, mod in enc.resnet.named_modules():
            if name.endswith("bn3"):
                mod.weight.fill_(0.2)
                mod.bias.fill_(0.5)
            elif name.endswith(("bn1", "bn2", "downsample.1")) or name == "1":
                mod.bias.fill_(3.5)
    cal = copy.deepcopy(enc.resnet).double().train()
    for mod in cal.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.momentum = None
            mod.reset_running_stats()
    with torch.no_grad():
        cal(torch.randn(4, 3, 96, 96, dtype=torch.float64))
    with torch.no_grad():
        for (k, b), (_, bc) in zip(enc.resnet.named_buffers(), cal.named_buffers()):
            if k.endswith("running_mean") or k.endswith("running_var"):
                b.copy_(bc.float())
    return enc.eval()


_REF_MAPS = {}


def _ref_trunk(enc, x, key):
    if key not in _REF_MAPS:
        ref = copy.deepcopy(enc.resnet).double().eval()
        with torch.no_grad():
            _REF_MAPS[key] = ref(x.double()).permute(0, 2, 3, 1)
    return _REF_MAPS[key]


@pytest.mark.parametrize("shape", [(8, 128, 128), (1, 256, 256), (2, 100, 100)])
@pytest.mark.parametrize("channels_last", [True, False])
def test_encoder_caption_eval_vs_fp64(dev, shape, channels_last):
    """The whole EncoderCaption (ResNet-152) in eval mode under no_grad: trunk map within 1e-4 rel-l2 of the fp64 CPU
    module, and no nn.Conv2d forward at all (stem on csrc/stem.hip, every Bottleneck on the fused eval block).  The B=1
    case is the inference shape; 100 x 100 gives odd maps (13, 7) down to 4 x 4."""
    B, H, W = shape
    enc = _calibrated_encoder(channels_last)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 3, H, W, generator=g)
    yr = _ref_trunk(enc, x, shape)
    ge = copy.deepcopy(enc).to(dev).eval()
    with torch.no_grad(), _ConvCalls() as cc:
        pre = ge(x.to(dev), pooled=False)
        y = ge(x.to(dev))
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    assert pre.shape == yr.shape and y.shape == (B, 14, 14, 2048)
    e = rel_l2(pre, yr)
    assert e <= 1e-4, "trunk map rel-l2 %.3e" % e


def test_grad_enabled_eval_matches_no_grad_and_fp64_gradients(dev):
    """The reference's inference.py: encoder.eval() called WITH grad enabled, layer2-4 requiring grad.  The output is
    bit-identical to the no_grad call; backward of a weighted sum (recomputed through the module-path ops) gives
    parameter and input gradients within 1e-4 rel-l2 of the fp64 CPU module; running statistics and
    num_batches_tracked do not move."""
    enc = _calibrated_encoder(True, depths=(1, 2, 2, 1), seed=8)
    g = torch.Generator().manual_seed(9)
    imgs = torch.randn(2, 3, 96, 96, generator=g)
    ge = copy.deepcopy(enc).to(dev).eval()
    bufs = {k: b.detach().clone() for k, b in ge.named_buffers()}
    with torch.no_grad():
        y0 = ge(imgs.to(dev), pooled=False)
    y1 = ge(imgs.to(dev), pooled=False)            # grad enabled, images do not require grad (inference.py)
    assert y1.requires_grad and torch.equal(y0, y1)
    # gradients: the Bottleneck stack (layer1..4) on a map that requires grad, against fp64
    trunk = ge.resnet
    ref = copy.deepcopy(enc.resnet).double().eval()
    x = torch.relu(torch.randn(2, 64, 24, 24, generator=g))
    wgt = torch.randn(2, 2048, 3, 3, generator=g)
    xr = x.double().requires_grad_(True)
    yr = xr
    for child in list(ref.children())[4:]:
        yr = child(yr)
    (yr * wgt.double()).sum().backward()
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.no_grad():
        yn = xg
        for child in list(trunk.children())[4:]:
            yn = child(yn)
    yg = xg
    for child in list(trunk.children())[4:]:
        yg = child(yg)
    assert torch.equal(yg.detach(), yn)
    assert rel_l2(yg, yr) <= 1e-4
    (yg * wgt.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert rel_l2(xg.grad, xr.grad) <= 1e-4, "d x %.3e" % rel_l2(xg.grad, xr.grad)
    n = 0
    for (k, p), (_, pr) in zip(trunk.named_parameters(), ref.named_parameters()):
        if pr.grad is None:
            assert p.grad is None, k
            continue
        n += 1
        assert p.grad is not None, k
        assert rel_l2(p.grad, pr.grad) <= 1e-4, "%s: %.3e" % (k, rel_l2(p.grad, pr.grad))
    assert n > 0
    for k, b in ge.named_buffers():
        assert torch.equal(b, bufs[k]), k


def test_train_eval_train_eval_sees_new_running_statistics(dev):
    """Training steps move the running statistics in place (the raw-pointer BatchNorm finalize) and the optimizer moves
    the weights in place; the next eval forward must match the fp64 module evaluated with the NEW state (nothing is
    cached in the eval path)."""
    from utils.optimizer import FusedClampAdam
    enc = _calibrated_encoder(True, depths=(1, 1, 1, 1), seed=12)
    enc.fine_tune(True)
    ge = copy.deepcopy(enc).to(dev)
    opt = FusedClampAdam([p for p in ge.parameters() if p.requires_grad], lr=1e-3, grad_clip=5.0)
    g = torch.Generator().manual_seed(13)
    xe = torch.randn(2, 3, 64, 64, generator=g)
    prev = None
    for rnd in range(2):
        ge.train()
        opt.zero_grad()
        y = ge(torch.randn(4, 3, 64, 64, generator=g).to(dev), pooled=False)
        (y * y).mean().backward()
        opt.step()
        ge.eval()
        with torch.no_grad():
            ye = ge(xe.to(dev), pooled=False)
        torch.cuda.synchronize()
        ref = copy.deepcopy(enc.resnet)
        ref.load_state_dict({k: v.detach().cpu() for k, v in ge.resnet.state_dict().items()})
        ref = ref.double().eval()
        with torch.no_grad():
            yr = ref(xe.double()).permute(0, 2, 3, 1)
        e = rel_l2(ye, yr)
        assert e <= 1e-4, "round %d: rel-l2 %.3e against the module with the new statistics" % (rnd, e)
        rm = torch.cat([b.flatten() for k, b in ge.resnet.named_buffers() if k.endswith("running_mean")])
        if prev is not None:
            assert not torch.equal(rm, prev), "the training step did not move the running statistics"
        prev = rm.clone()


def test_validate_through_the_eval_trunk(dev):
    """trains/harness.py::validate() with a real (depth-reduced) EncoderCaption and EncoderTagger: loss, top-5 and
    BLEU-4 equal the same call on the module path (conv.ENABLED = False) within 1e-4 relative (BLEU exactly when the
    arg-max hypotheses agree), with no nn.Conv2d forward on the fused side."""
    from models.decoders.attention_scn import AttentionSCN
    from models.encoders.tagger import EncoderTagger
    from scnattn import conv as SC
    from scnattn.resnet import resnet152_trunk
    from trains.harness import validate
    enc = _calibrated_encoder(True, depths=(1, 1, 2, 1), seed=21).to(dev)
    torch.manual_seed(22)
    tag = EncoderTagger(semantic_size=12, channels_last=True)
    tag.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    tag.fine_tune()
    tag = tag.to(dev)
    V, L, B = 40, 9, 4
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    dec = AttentionSCN(32, 24, 32, 40, 12, V, encoder_dim=2048, dropout=0.0).to(dev)
    g = torch.Generator().manual_seed(23)
    batches = []
    for _ in range(2):
        lens = torch.randint(4, L + 1, (B,), generator=g)
        caps = torch.zeros(B, L, dtype=torch.long)
        for b in range(B):
            n = int(lens[b])
            caps[b, 0] = V - 2
            caps[b, 1:n - 1] = torch.randint(1, V - 3, (n - 2,), generator=g)
            caps[b, n - 1] = V - 1
        allcaps = torch.stack([caps, caps.roll(1, 0)], dim=1)
        batches.append((torch.randn(B, 3, 96, 96, generator=g).to(dev), caps.to(dev), lens.unsqueeze(1).to(dev),
                        allcaps.to(dev)))
    crit = nn.CrossEntropyLoss().to(dev)
    with _ConvCalls() as cc:
        fused = validate(batches, enc, tag, dec, crit, wm)
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    SC.ENABLED = False
    try:
        with _ConvCalls() as cc:
            plain = validate(batches, enc, tag, dec, crit, wm)
            torch.cuda.synchronize()
        assert cc.n > 0
    finally:
        SC.ENABLED = True
    bleu, loss, top5 = fused
    bleu_p, loss_p, top5_p = plain
    assert abs(loss - loss_p) <= 1e-4 * abs(loss_p), (loss, loss_p)
    assert abs(top5 - top5_p) <= 1e-4 * max(abs(top5_p), 1.0), (top5, top5_p)
    assert bleu == bleu_p, (bleu, bleu_p)


def test_fallbacks_keep_the_module_path(dev):
    """bf16 autocast and widths that are not multiples of 16 stay on the module path, with the reason given, and produce
    what the module path produces."""
    from scnattn import conv_eval as CE
    m = _make_block(256, 64, 1, 31).to(dev).to(memory_format=torch.channels_last)
    x = torch.randn(2, 256, 16, 16, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert "autocast" in CE.eval_reason(m, x)
        y = m(x)
        yp = m.module_forward(x)
    assert y.dtype == yp.dtype and rel_err(y.float(), yp.float()) <= 1e-6
    m2 = _make_block(48, 12, 1, 32).to(dev)          # 12 planes: a multiple of 4 (the BatchNorm kernels), not of 16
    x2 = torch.randn(2, 48, 9, 9, device=dev)
    r = CE.eval_reason(m2, x2)
    assert r is not None and "multiples of 16" in r
    with torch.no_grad(), _ConvCalls() as cc:
        y2 = m2(x2)
    assert cc.n == 3
    with torch.no_grad():
        assert torch.equal(y2, m2.module_forward(x2))
        yr = copy.deepcopy(m2).cpu().double()(x2.cpu().double())
    assert rel_err(y2, yr) <= 1e-4
