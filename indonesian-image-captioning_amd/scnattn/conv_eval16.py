"""Eval-mode Bottleneck of the ResNet-152 trunk on bf16 maps: what `encoder.eval()` runs under
`torch.autocast("cuda", dtype=torch.bfloat16)` -- validation and caption generation after a `--dtype bf16` training run.

The block of scnattn/conv_eval.py on the bf16 GEMM (csrc/cgemm16.hip, EPI 3): every BatchNorm is the fixed per-channel map
z*scale + shift folded into the epilogue of the convolution that produces z, three launches, four with a downsample:

    a1  = relu(bn1(conv1(x)))                       scnattn_conv1x1_fwd_bn_eval16
    a2  = relu(bn2(conv2(a1)))     (3x3, stride s)   scnattn_conv3x3_fwd_bn_eval16
    idn = bnd(convd(x))  | x       (rows gathered at stride s)
    out = relu(bn3(conv3(a2)) + idn)

Maps are bf16 channels-last; accumulation, scale / shift and the epilogue are fp32 and each map is rounded once.  The 1x1
weights are the bf16 copies `_w16` that `refresh_weights` (scnattn/conv16.py) remakes from the fp32 masters at every trunk
forward under bf16 autocast (scnattn/stem.py run_trunk); a conv2 without one (an NCHW weight: the reference's default
EncoderCaption()) gets a transient bf16 [Cout][3][3][Cin] copy per call.  scale / shift are formed by the kernel from the
module's own parameters and running buffers at every call: nothing is cached across calls, and the running statistics and
`num_batches_tracked` are never touched.

Forward only: when autograd would need a gradient (the reference's inference.py runs the encoder in eval mode with grad
enabled) `eval16_reason` says so and the block keeps the module path."""
import ctypes as C

import torch

from . import block as B
from . import conv as _conv
from ._lib import BnEval16, ConvExtra
from .conv_eval import _vec

BF = torch.bfloat16


def eval16_reason(mod, x):
    """None when the fused bf16 eval block applies to `mod` (a scnattn.resnet.Bottleneck) on input `x`, else why not."""
    r = B.reason(mod, x, _conv.ENABLED, False, BF)
    if r:
        return r
    if any(t.dtype != torch.float32 or t.device != x.device
           for bn in B.bns(mod) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return "a BatchNorm parameter / statistic is not fp32 on the input's device"
    cvs = B.convs(mod)
    if any(cv.weight.device != x.device for cv in cvs):
        return "a convolution weight is not on the input's device"
    if cvs[1].in_channels % 32:
        return "conv2 takes %d channels, not a multiple of 32" % cvs[1].in_channels
    if not all(hasattr(cv, "_w16") for cv in cvs[:1] + cvs[2:]):
        return "a 1x1 convolution has no bf16 weight copy"
    if torch.is_grad_enabled() and (x.requires_grad or any(t is not None and t.requires_grad for t in B.params(mod))):
        return "a gradient is needed: the bf16 eval block is forward-only"
    return None


def _bn_eval(bn, relu, res=None, ldres=0):
    keep = (_vec(bn.weight), _vec(bn.bias), _vec(bn.running_mean), _vec(bn.running_var))
    b = BnEval16(gamma=keep[0].data_ptr(), beta=keep[1].data_ptr(), mean=keep[2].data_ptr(), var=keep[3].data_ptr(),
                 eps=float(bn.eps), res=None if res is None else res.data_ptr(), ldres=ldres, relu=1 if relu else 0)
    return b, keep


def bottleneck_eval16(mod, x):
    """Eval-mode forward of `mod` on the fused bf16 kernels, on the caller's stream (caller checked
    `eval16_reason(mod, x) is None`); returns the (N, C4, Ho, Wo) bf16 channels-last output."""
    dev = x.device
    h, st, ws = _conv._launch(dev)[:3]
    x = B.channels_last(x)
    N, Cin, Hi, Wi, p, C4, s, Ho, Wo, Rin, Rout = B.geometry(mod, x)
    c1, c2, c3 = B.convs(mod)[:3]
    x2 = _conv._as2d(x)
    bf = dict(device=dev, dtype=BF)
    f1, f3 = h.scnattn_conv1x1_fwd_bn_eval16, h.scnattn_conv3x3_fwd_bn_eval16
    with torch.no_grad():
        w2 = getattr(c2, "_w16", None)
        if w2 is None:      # never cached: an optimizer may rewrite the master in place through raw pointers
            w2 = c2.weight.detach().permute(0, 2, 3, 1).to(BF).contiguous()
        a1 = torch.empty((Rin, p), **bf)
        bn, keep1 = _bn_eval(mod.bn1, True)
        _conv._chk(f1(st, Rin, Cin, p, x2.data_ptr(), c1._w16.data_ptr(), a1.data_ptr(), C.byref(bn), None, ws.data_ptr(),
                      ws.numel()), "scnattn_conv1x1_fwd_bn_eval16")
        a2 = torch.empty((Rout, p), **bf)
        bn, keep2 = _bn_eval(mod.bn2, True)
        _conv._chk(f3(st, N, Hi, Wi, p, p, s, a1.data_ptr(), w2.data_ptr(), a2.data_ptr(), C.byref(bn), None, ws.data_ptr(),
                      ws.numel()), "scnattn_conv3x3_fwd_bn_eval16")
        if mod.downsample is not None:
            idn = torch.empty((Rout, C4), **bf)
            bn, keepd = _bn_eval(mod.downsample[1], False)
            ex = ConvExtra(stride=s, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo)
            _conv._chk(f1(st, Rout, Cin, C4, x2.data_ptr(), mod.downsample[0]._w16.data_ptr(), idn.data_ptr(), C.byref(bn),
                          C.byref(ex), ws.data_ptr(), ws.numel()), "scnattn_conv1x1_fwd_bn_eval16")
        else:
            idn = x2
        out = torch.empty((Rout, C4), **bf)
        bn, keep3 = _bn_eval(mod.bn3, True, idn, C4)
        _conv._chk(f1(st, Rout, p, C4, a2.data_ptr(), c3._w16.data_ptr(), out.data_ptr(), C.byref(bn), None, ws.data_ptr(),
                      ws.numel()), "scnattn_conv1x1_fwd_bn_eval16")
    return _conv._as4d(out, N, Ho, Wo)
