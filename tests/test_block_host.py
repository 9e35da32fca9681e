"""CPU tests of the Bottleneck front end shared by the fp32, bf16 and eval paths (scnattn/block.py): the structural check
accepts every block of the trunk and names what it rejects, the scratch capacity of the statistics partials, and the bf16
weight table that leaves out 3x3 weights the conversion kernel cannot read."""
import ctypes as C

import pytest
import torch
from torch import nn


def _block(inplanes=256, planes=64, stride=1):
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                             FusedBatchNorm2d(planes * 4))
    return Bottleneck(inplanes, planes, stride, down)


def _map(n, c, h, w=None):
    return torch.empty(n, c, h, h if w is None else w, device="meta")


def _trunk_blocks():
    from scnattn.resnet import Bottleneck, resnet152_trunk
    with torch.device("meta"):
        trunk = resnet152_trunk()
    return [m for m in trunk.modules() if isinstance(m, Bottleneck)]


@pytest.mark.parametrize("training", [True, False])
def test_structural_check_accepts_every_block_of_the_trunk(training):
    """All 50 Bottlenecks of resnet152_trunk() at the train step's geometry (B=32, 256 x 256 images: 64 x 64 maps after the
    stem), in training and in eval mode; their statistics partials fit the scratch."""
    from scnattn import block as B
    blocks = _trunk_blocks()
    assert len(blocks) == 50
    x = _map(32, 64, 64)
    for m in blocks:
        m.train(training)
        assert B.structural_reason(m, x) is None
        g = B.geometry(m, x)
        assert B.part_floats(g) <= B.PART_FLOATS
        x = _map(g.N, g.C4, g.Ho, g.Wo)
    assert tuple(x.shape) == (32, 2048, 8, 8)


def _rejections():
    """(description, block factory, input, expected words of the reason), one per term of the structural check."""
    from scnattn.resnet import FusedBatchNorm2d

    def with_(planes=64, stride=1, inplanes=256, **set_):
        def make():
            m = _block(inplanes, planes, stride)
            for k, v in set_.items():
                obj, attr = (m, k) if "." not in k else (m.get_submodule(k.rsplit(".", 1)[0]), k.rsplit(".", 1)[1])
                setattr(obj, attr, v() if callable(v) else v)
            return m
        return make
    x = _map(2, 256, 8)
    return [
        ("3-d input", with_(), torch.empty(2, 256, 8, device="meta"), "(N, C, H, W)"),
        ("downsample without BatchNorm", with_(128, 2, downsample=lambda: nn.Sequential(nn.Conv2d(256, 512, 1, 2, bias=False))),
         x, "downsample"),
        ("BatchNorm without affine parameters", with_(**{"bn2": lambda: FusedBatchNorm2d(64, affine=False)}), x, "not affine"),
        ("BatchNorm without running statistics", with_(**{"bn3": lambda: FusedBatchNorm2d(256, track_running_stats=False)}),
         x, "running statistics"),
        ("cumulative-average BatchNorm in training", with_(**{"bn1.momentum": None}), x, "momentum"),
        ("conv with a bias", with_(conv1=lambda: nn.Conv2d(256, 64, 1, bias=True)), x, "bias"),
        ("grouped conv2", with_(conv2=lambda: nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False)), x, "groups"),
        ("dilated conv2", with_(conv2=lambda: nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False)), x, "dilation"),
        ("3x3 conv1", with_(conv1=lambda: nn.Conv2d(256, 64, 3, padding=1, bias=False)), x, "conv1 / conv3"),
        ("strided conv3", with_(conv3=lambda: nn.Conv2d(64, 256, 1, stride=2, bias=False)), x, "conv1 / conv3"),
        ("5x5 conv2", with_(conv2=lambda: nn.Conv2d(64, 64, 5, padding=2, bias=False)), x, "conv2"),
        ("conv2 stride differs from the block's", with_(conv2=lambda: nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False)),
         x, "conv2"),
        ("block stride 3", with_(stride=3), x, "conv2"),
        ("12 planes", with_(12, inplanes=48), _map(2, 48, 8), "multiples of 16"),
        ("input channels differ from conv1's", with_(), _map(2, 128, 8), "input has 128 channels"),
        ("3x3 downsample", with_(128, 2, **{"downsample.0": lambda: nn.Conv2d(256, 512, 3, 2, padding=1, bias=False)}),
         x, "downsample"),
        ("downsample at stride 1 in a stride-2 block", with_(128, 2, **{"downsample.0": lambda: nn.Conv2d(256, 512, 1, bias=False)}),
         x, "downsample"),
        ("no downsample where the identity changes width", with_(64, inplanes=128, downsample=None), _map(2, 128, 8),
         "identity"),
    ]


@pytest.mark.parametrize("what,make,x,words", _rejections(), ids=[r[0] for r in _rejections()])
def test_structural_check_rejects_with_a_reason(what, make, x, words):
    from scnattn import block as B
    m = make().train()
    r = B.structural_reason(m, x)
    assert r is not None and words in r, (what, r)


def test_structural_check_has_no_device_or_dtype_terms():
    """A cumulative-average BatchNorm only matters in training; dtype and device never enter (bf16 CPU modules pass)."""
    from scnattn import block as B
    m = _block().eval()
    m.bn1.momentum = None
    assert B.structural_reason(m, _map(2, 256, 8)) is None
    assert B.structural_reason(m.to(torch.bfloat16), torch.empty(2, 256, 8, 8, dtype=torch.bfloat16)) is None


def test_scratch_capacity_of_the_statistics_partials():
    """layer1.0 at 256 x 256 images (64 x 64 maps, C4 = 256) fits the partials at B = 64 and not at B = 65; stat_ld is the
    library's own leading dimension."""
    from scnattn import _lib, block as B
    layer1_0 = _trunk_blocks()[0]
    assert B.part_floats(B.geometry(layer1_0, _map(64, 64, 64))) <= B.PART_FLOATS
    assert B.part_floats(B.geometry(layer1_0, _map(65, 64, 64))) > B.PART_FLOATS
    h = _lib.lib()
    for R in (1, 63, 64, 65, 255, 256, 257, 4096 * 64, 32 * 64 * 64 + 1, 65 * 64 * 64):
        assert B.stat_ld(R) == h.scnattn_cgemm_stat_ld(R), R


def test_training_paths_reject_cpu_maps_with_a_reason():
    from scnattn import conv as SC, conv16 as C16
    m = _block().train()
    x = torch.randn(2, 256, 8, 8)
    assert "GPU" in SC.train_reason(m, x) and not SC.usable(m, x)
    assert "GPU" in C16.bf16_reason(m, x.to(torch.bfloat16)) and not C16.usable(m, x)
    assert "eval mode" in C16.bf16_reason(m.eval(), x.to(torch.bfloat16))


def test_bf16_weight_table_leaves_out_3x3_weights_that_are_not_channels_last():
    """The conversion kernel reads a 3x3 weight as [Cout][3][3][Cin]: one that is not channels-last gets no bf16 copy (its
    block then takes the module path) instead of an error, and gets one once it is channels-last."""
    from scnattn import conv16 as C16
    trunk = nn.Sequential(_block(64, 64, 1), _block(256, 64, 1))
    w = C16._Weights(trunk, torch.device("cpu"))
    w._table(torch.device("cpu"))
    conv2s = [b.conv2 for b in trunk]
    assert len(w.convs) == 7 and w.n == 5
    assert not any(hasattr(c, "_w16") or hasattr(c, "_w16t") for c in conv2s)
    assert all(hasattr(c, "_w16") for b in trunk for c in (b.conv1, b.conv3))
    assert w.desc.numel() == 5 * C.sizeof(C16._WeightDesc)
    trunk.to(memory_format=torch.channels_last)
    w._table(torch.device("cpu"))
    assert w.n == 7 and all(c._w16.shape == (64, 9 * 64) for c in conv2s)
    assert w.total == (4 + 36 + 16 + 16) + (16 + 36 + 16)      # 32 x 32 tiles: taps * Cout/32 * Cin/32
    trunk[0].conv2.weight.data = trunk[0].conv2.weight.data.contiguous()
    w._table(torch.device("cpu"))
    assert w.n == 6 and not hasattr(trunk[0].conv2, "_w16") and hasattr(trunk[1].conv2, "_w16")
