"""What the four hand-written Bottleneck paths share (scnattn/resnet.py `Bottleneck.forward` tries them in this order):

    fp32 maps, training mode    scnattn/conv.py       train_reason / bottleneck
    fp32 maps, eval mode        scnattn/conv_eval.py  eval_reason / bottleneck_eval
    bf16 maps, training mode    scnattn/conv16.py     bf16_reason / bottleneck
    bf16 maps, eval mode        scnattn/conv_eval16.py  eval16_reason / bottleneck_eval16

Each `*_reason(mod, x)` returns None when its path applies, else a short reason: `reason` below, then its own terms.
These run on the host before every block call (the bf16 step is host-bound), so they read submodules from `_modules`:
`mod.conv1` through nn.Module.__getattr__ costs about a microsecond per name."""
from collections import namedtuple

import torch
from torch import nn

PART_FLOATS = 2 << 20       # floats of each statistics-partial scratch, `part` and `bnpart` (scnattn/conv.py _launch)

Geom = namedtuple("Geom", "N Cin Hi Wi p C4 s Ho Wo Rin Rout")


def bns(mod):
    """bn1, bn2, bn3 (+ downsample.1): the BatchNorm index order of the kernels (include/scnattn.h scnattn_block16)."""
    m = mod._modules
    d = m.get("downsample")      # a plain attribute when None
    return (m["bn1"], m["bn2"], m["bn3"]) + ((d[1],) if d is not None else ())


def convs(mod):
    """conv1, conv2, conv3 (+ downsample.0), in the same order."""
    m = mod._modules
    d = m.get("downsample")      # a plain attribute when None
    return (m["conv1"], m["conv2"], m["conv3"]) + ((d[0],) if d is not None else ())


def params(mod):
    """(w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd): what every block's autograd function takes after (mod, x)."""
    p = tuple(t for cv, bn in zip(convs(mod), bns(mod)) for t in (cv.weight, bn.weight, bn.bias))
    return p + (None,) * (12 - len(p))


def bump_counters(bns):
    """A training forward's num_batches_tracked += 1, unless the trunk bumps them all in one launch (counter_managed)."""
    for bn in bns:
        if not getattr(bn, "counter_managed", False) and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)


def geometry(mod, x):
    N, Cin, Hi, Wi = x.shape
    s = mod.stride
    Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
    m = mod._modules
    return Geom(N, Cin, Hi, Wi, m["conv1"].out_channels, m["conv3"].out_channels, s, Ho, Wo, N * Hi * Wi, N * Ho * Wo)


def channels_last(x):
    return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)


def stat_ld(R):
    """Leading dimension of the channel-major statistics partials [2][C][ld] a product of R rows writes: one entry per
    64-row block, rounded up to 4 (csrc/cgemm.hip cgemm_stat_ld)."""
    return ((R + 63) // 64 + 3) & ~3


def part_floats(g):
    """Floats of `part` / `bnpart` a training block writes at most: p channels over the input rows (conv1, conv2's d input)
    or C4 channels over the output rows (conv3, the downsample)."""
    return 2 * max(g.p * stat_ld(g.Rin), g.C4 * stat_ld(g.Rout))


def structural_reason(mod, x):
    """None when `mod` (a scnattn.resnet.Bottleneck) on an input of `x`'s shape is the block the kernels compute, else why
    not.  No device or dtype enters: CPU modules and meta tensors can be checked.  It reads the layers' configuration
    (plain attributes), not their parameters."""
    if x.dim() != 4:
        return "input is not an (N, C, H, W) map"
    m, s = mod._modules, mod.stride
    c1, c2, c3, d = m["conv1"], m["conv2"], m["conv3"], m.get("downsample")
    if d is not None and (len(d) != 2 or not isinstance(d[0], nn.Conv2d) or not isinstance(d[1], nn.BatchNorm2d)):
        return "downsample is not a 1x1 convolution at the block's stride + BatchNorm"
    for bn in bns(mod):
        if not bn.affine:
            return "a BatchNorm is not affine"
        if not bn.track_running_stats:
            return "a BatchNorm has no running statistics"
        if mod.training and bn.momentum is None:
            return "a BatchNorm has no momentum (cumulative average)"
    for cv in convs(mod):
        if cv.bias is not None or cv.groups != 1 or cv.dilation != (1, 1):
            return "a convolution has a bias, groups or dilation"
    if (c1.kernel_size, c1.stride, c1.padding) != ((1, 1), (1, 1), (0, 0)) \
            or (c3.kernel_size, c3.stride, c3.padding) != ((1, 1), (1, 1), (0, 0)):
        return "conv1 / conv3 are not 1x1 at stride 1"
    if s not in (1, 2) or (c2.kernel_size, c2.stride, c2.padding) != ((3, 3), (s, s), (1, 1)):
        return "conv2 is not 3x3 / padding 1 at stride 1 or 2"
    p, cin, c4 = c1.out_channels, c1.in_channels, c3.out_channels
    if p % 16 or cin % 16 or c4 % 16:
        return "widths (%d, %d, %d) are not multiples of 16" % (cin, p, c4)
    if x.shape[1] != cin:
        return "input has %d channels, conv1 takes %d" % (x.shape[1], cin)
    if d is not None:
        if (d[0].kernel_size, d[0].stride, d[0].padding, d[0].out_channels) != ((1, 1), (s, s), (0, 0), c4):
            return "downsample is not a 1x1 convolution at the block's stride + BatchNorm"
    elif s != 1 or cin != c4:
        return "no downsample, but the identity does not match the output"
    return None


def reason(mod, x, enabled, training, dtype):
    """The terms every path has: the kernels `enabled`, the module's mode, a GPU map of `dtype` (an fp32 one outside
    autocast), the structure, and fp32 BatchNorm parameters for the training kernels."""
    if not enabled:
        return "fused kernels disabled (scnattn.conv.ENABLED is False)"
    if mod.training != training:
        return "module is in %s mode" % ("training" if mod.training else "eval")
    if dtype == torch.float32 and torch.is_autocast_enabled():
        return "autocast is enabled"
    if not x.is_cuda:
        return "input is not a GPU tensor"
    if x.dtype != dtype:
        return "input is not a %s map" % str(dtype)[6:]
    r = structural_reason(mod, x)
    if r is None and training and any(bn.weight.dtype != torch.float32 for bn in bns(mod)[:3]):
        return "a BatchNorm parameter is not fp32"
    return r


def grads(need, dx, dw, dgb):
    """What a block's backward returns for (mod, x, w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd): d x, then per
    convolution i its weight gradient dw[i] and its BatchNorm's d gamma, d beta = dgb[i][1], dgb[i][0]; None if unneeded."""
    out = [None, dx]
    for w, gb in zip(dw, dgb):
        out += [w, None, None] if gb is None else [w, gb[1], gb[0]]
    return tuple(o if n else None for o, n in zip(out, need))
