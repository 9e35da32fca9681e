"""GPU tests of the Bottleneck front end (scnattn/block.py) where it decides between the hand-written paths and the module
path: the scratch capacity of the statistics partials, 3x3 weights that are not channels-last under bf16 autocast, and
the bf16 weight copies when the fused stem does not run."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


def test_training_blocks_fall_back_when_the_partials_exceed_the_scratch(dev):
    """layer1.0 at 256 x 256 images: B = 64 fits the statistics partials, B = 65 would write past them, so both training
    paths name the reason and the block takes the module path."""
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    from scnattn import conv as SC, conv16 as C16
    torch.manual_seed(3)
    down = nn.Sequential(nn.Conv2d(64, 256, kernel_size=1, bias=False), FusedBatchNorm2d(256))
    m = Bottleneck(64, 64, 1, down).to(dev).to(memory_format=torch.channels_last).train()
    C16.refresh_weights(m)
    x64 = torch.randn(64, 64, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    x65 = torch.randn(65, 64, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    assert SC.train_reason(m, x64) is None and C16.bf16_reason(m, x64.to(torch.bfloat16)) is None
    assert SC.train_reason(m, x65) == "statistics partials exceed the scratch"
    assert C16.bf16_reason(m, x65.to(torch.bfloat16)) == "statistics partials exceed the scratch"
    m1, m2 = copy.deepcopy(m), copy.deepcopy(m)
    with torch.no_grad():
        y, yp = m1(x65), m2.module_forward(x65)
    torch.cuda.synchronize()
    assert torch.equal(y, yp)


def test_encoder_caption_nchw_under_bf16_autocast_runs(dev):
    """EncoderCaption(channels_last=False) keeps NCHW weights: under bf16 autocast the 3x3 convolutions get no bf16 copy,
    so their blocks take the module path instead of raising; the 1x1 convolutions keep theirs."""
    from models.encoders.caption import EncoderCaption
    torch.manual_seed(4)
    enc = EncoderCaption(channels_last=False).to(dev).train()
    images = torch.randn(2, 3, 256, 256, device=dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = enc(images)
    torch.cuda.synchronize()
    assert y.shape == (2, 14, 14, 2048) and bool(torch.isfinite(y).all())
    blk = enc.resnet[5][0]
    assert not hasattr(blk.conv2, "_w16") and hasattr(blk.conv1, "_w16") and hasattr(blk.conv3, "_w16")


def test_bf16_blocks_see_new_weights_when_the_stem_is_unusable(dev):
    """A bf16 step, an in-place change of the master weights, then a forward whose stem needs a gradient (the module path):
    the blocks must compute with the new weights, exactly as a run that refreshes the bf16 copies explicitly."""
    from scnattn.resnet import resnet152_trunk
    from scnattn.stem import run_trunk, usable as stem_usable
    from scnattn import conv16 as C16
    outs, calls = [], []
    for explicit in (False, True):
        torch.manual_seed(5)
        trunk = resnet152_trunk(depths=(1, 1, 1, 1)).to(dev).to(memory_format=torch.channels_last).train()
        for p in list(trunk[0].parameters()) + list(trunk[1].parameters()):
            p.requires_grad_(False)
        x = torch.randn(2, 3, 64, 64, device=dev)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert stem_usable(trunk, x)
            run_trunk(trunk, x).float().square().sum().backward()
        with torch.no_grad():
            for m in trunk.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.add_(0.5 * m.weight.std() * torch.randn_like(m.weight))      # in place: same pointers
        trunk[0].weight.requires_grad_(True)
        n = [0]
        fused = C16.bottleneck

        def counted(mod, x):
            n[0] += 1
            return fused(mod, x)
        C16.bottleneck = counted
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                assert not stem_usable(trunk, x)
                if explicit:
                    C16.refresh_weights(trunk)
                y = run_trunk(trunk, x)
        finally:
            C16.bottleneck = fused
        torch.cuda.synchronize()
        outs.append(y.detach().float())
        calls.append(n[0])
    assert calls == [4, 4]
    assert torch.equal(outs[0], outs[1])
