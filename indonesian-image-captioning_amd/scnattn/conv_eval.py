"""Eval-mode Bottleneck of the ResNet-152 trunk on the hand-written kernels (fp32, channels-last maps).

With running statistics a BatchNorm is the fixed per-channel map z*scale + shift (scale = gamma / sqrt(var + eps),
shift = beta - mean * scale), so it folds into the epilogue of the convolution that produces z (csrc/cgemm.hip, EPI 3):
the pre-BatchNorm maps z1, z2, z3 are never written, and a block is three launches, four with a downsample:

    a1  = relu(bn1(conv1(x)))                       scnattn_conv1x1_fwd_bn_eval
    a2  = relu(bn2(conv2(a1)))     (3x3, stride s)   scnattn_conv3x3_fwd_bn_eval
    idn = bnd(convd(x))  | x       (rows gathered at stride s)
    out = relu(bn3(conv3(a2)) + idn)

scale / shift are formed by the kernel from the module's own weight, bias and running buffers at every call, so a
training step that moves the running statistics in place (through raw pointers, which does not bump `_version`) is
seen by the next eval call; nothing is cached.  Running statistics and `num_batches_tracked` are never touched.

Autograd: the reference's inference.py runs the encoder in eval mode WITH grad enabled (layer2-4 require grad), so the
fused forward is one autograd node that saves only its input and, in backward, recomputes the block through the
unchanged module-path ops (`Bottleneck.module_forward`) and returns their gradients -- backward keeps today's kernels.

`Bottleneck.forward` (scnattn/resnet.py) takes this path when `eval_reason` returns None; every other case (bf16
autocast -- bf16 maps then take scnattn/conv_eval16.py --, widths that are not multiples of 16, CPU tensors, `conv.ENABLED = False`) keeps the module path."""
import ctypes as C

import torch

from . import block as B
from . import conv as _conv
from ._lib import BnEval, ConvExtra


def eval_reason(mod, x):
    """None when the fused eval block applies to `mod` (a scnattn.resnet.Bottleneck) on input `x`, else why not."""
    r = B.reason(mod, x, _conv.ENABLED, False, torch.float32)
    if r is None and any(t.dtype != torch.float32 or t.device != x.device for t in [cv.weight for cv in B.convs(mod)] +
                         [t for bn in B.bns(mod) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]):
        return "a parameter / statistic is not fp32 on the input's device"
    return r


def _vec(t):
    """A [C] fp32 vector the kernel can read 16 bytes at a time (parameters and buffers already are: no copy)."""
    if not t.is_contiguous() or t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _w2d(w, rows, cols):
    w = w.reshape(rows, cols)
    return w if w.is_contiguous() and w.data_ptr() % 16 == 0 else w.contiguous().clone()


def _bn_eval(bn, relu, res=None, ldres=0):
    keep = (_vec(bn.weight), _vec(bn.bias), _vec(bn.running_mean), _vec(bn.running_var))
    b = BnEval(gamma=keep[0].data_ptr(), beta=keep[1].data_ptr(), mean=keep[2].data_ptr(), var=keep[3].data_ptr(),
               eps=float(bn.eps), res=None if res is None else res.data_ptr(), ldres=ldres, relu=1 if relu else 0)
    return b, keep


def _forward(mod, x):
    """The fused eval block on the caller's stream; returns the (N, C4, Ho, Wo) channels-last output."""
    dev = x.device
    h, st, ws = _conv._launch(dev)[:3]
    x = B.channels_last(x)
    N, Cin, Hi, Wi, p, C4, s, Ho, Wo, Rin, Rout = B.geometry(mod, x)
    w1, w3 = mod.conv1.weight, mod.conv3.weight
    x2 = _conv._as2d(x)
    f32 = dict(device=dev, dtype=torch.float32)
    with torch.no_grad():
        # conv2's weight as [Cout][3][3][Cin]: a transient channels-last copy when the module is not channels-last (never
        # cached -- an optimizer may rewrite the weights in place through raw pointers)
        w2 = mod.conv2.weight.detach().contiguous(memory_format=torch.channels_last)
        a1 = torch.empty((Rin, p), **f32)
        bn, keep1 = _bn_eval(mod.bn1, True)
        _conv._chk(h.scnattn_conv1x1_fwd_bn_eval(st, Rin, Cin, p, x2.data_ptr(), _w2d(w1.detach(), p, Cin).data_ptr(),
                                                 a1.data_ptr(), C.byref(bn), None, ws.data_ptr(), ws.numel()),
                   "scnattn_conv1x1_fwd_bn_eval")
        a2 = torch.empty((Rout, p), **f32)
        bn, keep2 = _bn_eval(mod.bn2, True)
        _conv._chk(h.scnattn_conv3x3_fwd_bn_eval(st, N, Hi, Wi, p, p, s, a1.data_ptr(), w2.data_ptr(), a2.data_ptr(),
                                                 C.byref(bn), None, ws.data_ptr(), ws.numel()),
                   "scnattn_conv3x3_fwd_bn_eval")
        if mod.downsample is not None:
            idn = torch.empty((Rout, C4), **f32)
            bn, keepd = _bn_eval(mod.downsample[1], False)
            ex = ConvExtra(stride=s, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo)
            _conv._chk(h.scnattn_conv1x1_fwd_bn_eval(st, Rout, Cin, C4, x2.data_ptr(),
                                                     _w2d(mod.downsample[0].weight.detach(), C4, Cin).data_ptr(),
                                                     idn.data_ptr(), C.byref(bn), C.byref(ex), ws.data_ptr(), ws.numel()),
                       "scnattn_conv1x1_fwd_bn_eval")
        else:
            idn = x2
        out = torch.empty((Rout, C4), **f32)
        bn, keep3 = _bn_eval(mod.bn3, True, idn, C4)
        _conv._chk(h.scnattn_conv1x1_fwd_bn_eval(st, Rout, p, C4, a2.data_ptr(), _w2d(w3.detach(), C4, p).data_ptr(),
                                                 out.data_ptr(), C.byref(bn), None, ws.data_ptr(), ws.numel()),
                   "scnattn_conv1x1_fwd_bn_eval")
    return _conv._as4d(out, N, Ho, Wo)


class _EvalBottleneckFn(torch.autograd.Function):
    """Fused eval forward; backward recomputes the block through the module-path ops and returns their gradients."""

    @staticmethod
    def forward(ctx, mod, x, *params):
        ctx.mod = mod
        ctx.save_for_backward(x, *params)
        return _forward(mod, x)

    @staticmethod
    def backward(ctx, dout):
        x, *params = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]          # (x, *params)
        with torch.enable_grad():
            xr = x.detach().requires_grad_(need[0])
            y = ctx.mod.module_forward(xr)
            leaves = [t for t, n in zip([xr] + list(params), need) if n]
            got = iter(torch.autograd.grad(y, leaves, dout, allow_unused=True)) if leaves else iter(())
        return (None,) + tuple(next(got) if n else None for n in need)


def bottleneck_eval(mod, x):
    """Eval-mode forward of `mod` on the fused kernels (caller checked `eval_reason(mod, x) is None`)."""
    params = B.params(mod)
    if torch.is_grad_enabled() and (x.requires_grad or any(t is not None and t.requires_grad for t in params)):
        return _EvalBottleneckFn.apply(mod, x, *params)
    return _forward(mod, x)
