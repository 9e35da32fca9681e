"""GPU tests (``-m gpu``) of the eval-mode trunk on bf16 maps (scnattn/conv_eval16.py): what `encoder.eval()` runs under
`torch.autocast("cuda", dtype=torch.bfloat16)`.  One Bottleneck of every shape class and whole encoders against the fp64
CPU module, with the bf16 module path (conv.ENABLED = False under the same autocast: nn.Conv2d + the BatchNorm kernels,
which round every pre-BatchNorm map as well) as the yardstick on the same input; freshness after in-place updates; the
fallbacks; one validate() batch.  Constructions are those of tests/test_gpu_eval_trunk.py.

Every rel-l2 measured here goes to the run's parity report (test_gpu_parity._report)."""
import copy

import pytest
import torch
from torch import nn

from helpers import rel_l2
from test_gpu_eval_trunk import _BLOCKS, _ConvCalls, _calibrated_encoder, _make_block

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BF16_OUT = 5e-3         # the project's bar for bf16 maps (tests/test_gpu_parity_r3.py)
RATIO = 1.25            # fused rel-l2 <= RATIO x module-path rel-l2: fewer roundings, two realisations of rounding noise
_LINES = []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    del _LINES[:]
    yield
    if _LINES:
        from test_gpu_parity import _report
        _report(list(_LINES), "bf16 eval trunk vs the fp64 CPU module: rel-l2 of the fused path and of the bf16 module path")


def _note(line):
    print(line)
    _LINES.append(line)


def _autocast():
    return torch.autocast("cuda", dtype=BF)


def _module_path(fn):
    """fn() with the fused kernels disabled: the bf16 module path under the caller's autocast"""
    from scnattn import conv as SC
    SC.ENABLED = False
    try:
        return fn()
    finally:
        SC.ENABLED = True


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("name,inplanes,planes,stride,H", _BLOCKS)
def test_fused_eval16_bottleneck_vs_fp64(dev, name, inplanes, planes, stride, H, channels_last):
    """One eval-mode Bottleneck (fp32 weights, bf16 input) at N = 2, H <= 16 through scnattn/conv_eval16.py against the same
    module in fp64 on the CPU: no nn.Conv2d forward, a bf16 channels-last output, buffers untouched, rel-l2 <= 5e-3 and
    <= 1.25 x the rel-l2 of the bf16 module path on the same input.  channels_last=False: an NCHW module, whose conv2 has
    no bf16 copy and takes the transient one."""
    from scnattn import conv16 as C16, conv_eval16 as CE16
    H = min(H, 16)
    m = _make_block(inplanes, planes, stride, 3000 + [b[0] for b in _BLOCKS].index(name))
    x = (torch.relu(torch.randn(2, inplanes, H, H)) + 0.1 * torch.randn(2, inplanes, H, H)).to(BF)
    with torch.no_grad():
        yr = copy.deepcopy(m).double()(x.double())
    gm = copy.deepcopy(m).to(dev)
    xg = x.to(dev)
    if channels_last:
        gm = gm.to(memory_format=torch.channels_last)
        xg = xg.contiguous(memory_format=torch.channels_last)
    C16.refresh_weights(gm)
    assert hasattr(gm.conv2, "_w16") == channels_last
    bufs = {k: b.detach().clone() for k, b in gm.named_buffers()}
    with torch.no_grad(), _autocast():
        assert CE16.eval16_reason(gm, xg) is None
        with _ConvCalls() as cc:
            y = gm(xg)
        with _ConvCalls() as cm:
            ym = _module_path(lambda: gm(xg))
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    assert cm.n == (4 if gm.downsample is not None else 3)
    assert y.dtype == BF and y.shape == yr.shape and y.is_contiguous(memory_format=torch.channels_last)
    e, em = rel_l2(y.float(), yr), rel_l2(ym.float(), yr)
    _note("%-9s %s: fused %.3e  module path %.3e  ratio %.3f" % (name, "channels-last" if channels_last else "NCHW         ", e, em, e / em))
    assert e <= BF16_OUT, "%s: rel-l2 %.3e" % (name, e)
    assert e <= RATIO * em, "%s: fused %.3e against %.3e on the module path" % (name, e, em)
    for k, b in gm.named_buffers():
        assert torch.equal(b, bufs[k]), k


_REFS = {}


def _encoder_case(depths, shape):
    """(encoder, images, fp64 trunk map) built once per case"""
    key = (depths, shape)
    if key not in _REFS:
        enc = _calibrated_encoder(True, depths=depths)
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(17))
        with torch.no_grad():
            yr = copy.deepcopy(enc.resnet).double().eval()(x.double()).permute(0, 2, 3, 1)
        _REFS[key] = (enc, x, yr)
    return _REFS[key]


@pytest.mark.parametrize("depths,shape", [((1, 1, 1, 1), (2, 3, 64, 64)), (None, (1, 3, 100, 100))], ids=["depth1-2x64", "resnet152-1x100"])
def test_encoder_caption_eval16_vs_fp64(dev, depths, shape):
    """The whole EncoderCaption in eval mode under no_grad and bf16 autocast: no nn.Conv2d forward, an fp32
    (B, 14, 14, 2048) output, and the trunk map no further from fp64 than 1.25 x the bf16 module path is.  The full
    ResNet-152 at 100 x 100 has odd maps (25, 13, 7, 4), stride 2 on odd maps and the B = 1 splits of layer3 / layer4."""
    enc, x, yr = _encoder_case(depths, shape)
    ge = copy.deepcopy(enc).to(dev).eval()
    xg = x.to(dev)
    with torch.no_grad(), _autocast():
        with _ConvCalls() as cc:
            pre = ge(xg, pooled=False)
            y = ge(xg)
        prem = _module_path(lambda: ge(xg, pooled=False))
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    assert y.shape == (shape[0], 14, 14, 2048) and y.dtype == torch.float32 and pre.dtype == torch.float32
    assert pre.shape == yr.shape
    e, em = rel_l2(pre, yr), rel_l2(prem, yr)
    _note("EncoderCaption %s %s: fused %.3e  module path %.3e  ratio %.3f" % (depths or "(3, 8, 36, 3)", shape, e, em, e / em))
    assert e <= RATIO * em, "trunk map: fused %.3e against %.3e on the module path" % (e, em)


def test_encoder_tagger_eval16(dev):
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    torch.manual_seed(41)
    tag = EncoderTagger(semantic_size=12, channels_last=True)
    tag.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    tag.fine_tune()
    tag = tag.to(dev).eval()
    x = torch.randn(2, 3, 64, 64, device=dev)
    with torch.no_grad(), _autocast(), _ConvCalls() as cc:
        p = tag(x)
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    assert p.shape == (2, 12) and bool(torch.isfinite(p).all()) and bool(((p >= 0) & (p <= 1)).all())


def test_eval16_sees_in_place_updates(dev):
    """Nothing is cached across calls: after conv weights and running statistics change in place, the next forward equals,
    bit for bit, that of a freshly built module holding the new values."""
    enc, x, _ = _encoder_case((1, 1, 1, 1), (2, 3, 64, 64))
    ge = copy.deepcopy(enc).to(dev).eval()
    xg = x.to(dev)
    with torch.no_grad(), _autocast():
        y0 = ge(xg, pooled=False)
        g = torch.Generator(device=dev).manual_seed(3)
        for mod in ge.resnet.modules():
            if isinstance(mod, nn.Conv2d):
                mod.weight.mul_(1.0 + 0.1 * torch.randn(mod.weight.shape, device=dev, generator=g))
            elif isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.add_(0.1 * torch.randn(mod.running_mean.shape, device=dev, generator=g))
                mod.running_var.mul_(1.0 + 0.5 * torch.rand(mod.running_var.shape, device=dev, generator=g))
        y1 = ge(xg, pooled=False)
        fresh = copy.deepcopy(enc)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in ge.state_dict().items()})
        fresh = fresh.to(dev).eval()
        with _ConvCalls() as cc:
            y2 = fresh(xg, pooled=False)
        torch.cuda.synchronize()
    assert cc.n == 0
    assert not torch.equal(y0, y1), "the update changed nothing"
    assert torch.equal(y1, y2), "stale values: rel-l2 %.3e against the fresh module" % rel_l2(y1, y2)


def test_fallbacks_keep_their_paths(dev, monkeypatch):
    from scnattn import conv16 as C16, conv_eval as CE, conv_eval16 as CE16
    m = _make_block(256, 64, 1, 51).to(dev).to(memory_format=torch.channels_last)
    C16.refresh_weights(m)
    x = torch.randn(2, 256, 16, 16, device=dev).to(BF).contiguous(memory_format=torch.channels_last)
    # grad enabled and the parameters require it (the reference's inference.py): the module path, and backward works
    with _autocast():
        r = CE16.eval16_reason(m, x)
        assert r is not None and "gradient" in r
        with _ConvCalls() as cc:
            y = m(x)
        yp = m.module_forward(x)
        assert cc.n == 3 and y.requires_grad and torch.equal(y, yp)
        y.float().sum().backward()
    assert m.conv1.weight.grad is not None and bool(torch.isfinite(m.conv1.weight.grad).all())
    # a training-mode bf16 block still goes to scnattn/conv16.py
    calls = []
    orig = C16.bottleneck
    monkeypatch.setattr(C16, "bottleneck", lambda mod, t: calls.append(1) or orig(mod, t))
    monkeypatch.setattr(CE16, "bottleneck_eval16", lambda mod, t: pytest.fail("the eval block took a training-mode module"))
    m.train()
    with _autocast(), _ConvCalls() as cc:
        assert "training" in CE16.eval16_reason(m, x)
        yt = m(x)
    assert calls == [1] and cc.n == 0 and yt.dtype == BF
    monkeypatch.undo()
    # an fp32 map under autocast still answers "autocast" and keeps the module path
    m.eval()
    xf = x.float()
    with torch.no_grad(), _autocast():
        assert "autocast" in CE.eval_reason(m, xf)
        assert "bfloat16" in CE16.eval16_reason(m, xf)
        with _ConvCalls() as cc:
            yf = m(xf)
        assert cc.n == 3 and torch.equal(yf, m.module_forward(xf))


class _UnderAutocast(nn.Module):
    """An encoder run under bf16 autocast, as trains/harness.py runs it with --dtype bf16 (the decoder stays fp32)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, imgs):
        with _autocast():
            return self.inner(imgs)


def test_validate_batch_under_autocast(dev):
    """One validate() batch with both encoders under bf16 autocast: the trunks run on the fused path (no nn.Conv2d
    forward).  Loss and top-5 are printed next to the fp32 run's: recorded, not gated."""
    from models.decoders.attention_scn import AttentionSCN
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    from trains.harness import validate
    enc = _calibrated_encoder(True, depths=(1, 1, 1, 1)).to(dev)
    torch.manual_seed(22)
    tag = EncoderTagger(semantic_size=12, channels_last=True)
    tag.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    tag.fine_tune()
    tag = tag.to(dev)
    V, L, B = 40, 9, 4
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    dec = AttentionSCN(32, 24, 32, 40, 12, V, encoder_dim=2048, dropout=0.0).to(dev)
    g = torch.Generator().manual_seed(23)
    lens = torch.randint(4, L + 1, (B,), generator=g)
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        caps[b, 0] = V - 2
        caps[b, 1:n - 1] = torch.randint(1, V - 3, (n - 2,), generator=g)
        caps[b, n - 1] = V - 1
    allcaps = torch.stack([caps, caps.roll(1, 0)], dim=1)
    batches = [(torch.randn(B, 3, 64, 64, generator=g).to(dev), caps.to(dev), lens.unsqueeze(1).to(dev), allcaps.to(dev))]
    crit = nn.CrossEntropyLoss().to(dev)
    with _ConvCalls() as cc:
        bleu16, loss16, top16 = validate(batches, _UnderAutocast(enc), _UnderAutocast(tag), dec, crit, wm)
        torch.cuda.synchronize()
    assert cc.n == 0, "nn.Conv2d ran %d times" % cc.n
    bleu, loss, top5 = validate(batches, enc, tag, dec, crit, wm)
    _note("validate(): bf16 autocast loss %.6f top-5 %.3f BLEU-4 %.4f | fp32 loss %.6f top-5 %.3f BLEU-4 %.4f" % (
        loss16, top16, bleu16, loss, top5, bleu))
    assert loss16 == loss16 and abs(loss16) < float("inf")
