"""Image augmentation inside the device input pipeline: random resized crop, horizontal flip and colour
jitter applied by the launch that gathers a batch from the uint8 rows (csrc/augment.hip through the C ABI).  The reference
has no augmentation at all -- it feeds `Normalize` only (trains/attention_scn.py:121-126) -- so the semantics are this
project's own; include/scnattn.h states them.  Three things to know before switching it on:
  * the contrast step pulls towards the mean grey of the SOURCE image, not of the crop (one static table, one pass);
  * a mirrored image can contradict "kiri" / "kanan" (left / right) in its caption, which is why `flip` is a parameter;
  * the output keeps the source size: the crop is magnified back, never shrunk, so no antialias filter is involved.
There is no CPU fallback: the records are drawn and applied on the GPU."""
import ctypes as C

import numpy as np
import torch

from ._lib import AUGMENT_NPARAM, AugmentConfig, call, ptr, require_cuda, stream_of


def _pair(name, v):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("Augment: %s must be a (low, high) pair (got %r)" % (name, v)) from None
    return lo, hi


class Augment:
    """The distribution one sample's view is drawn from.  scale: crop area as a fraction of the image; ratio: change of the
    aspect, log-uniform; flip: probability of the mirror; brightness / contrast / saturation: strengths s, each factor
    uniform in [1 - s, 1 + s].  The view of a sample is a function of (seed, epoch, sample id) alone
    (`scnattn_augment_draw`), whatever the batch size, the rank or the loader mode."""

    def __init__(self, scale=(0.6, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=0.5, brightness=0.2, contrast=0.2,
                 saturation=0.2, seed=0):
        self.scale, self.ratio = _pair("scale", scale), _pair("ratio", ratio)
        self.flip, self.brightness, self.contrast, self.saturation = float(flip), float(brightness), float(contrast), float(saturation)
        self.seed = int(seed)
        if not 0.0 < self.scale[0] <= self.scale[1] <= 1.0:
            raise ValueError("Augment: scale needs 0 < low <= high <= 1 (got %r)" % (self.scale,))
        if not 0.0 < self.ratio[0] <= self.ratio[1] < float("inf"):
            raise ValueError("Augment: ratio needs 0 < low <= high (got %r)" % (self.ratio,))
        if not 0.0 <= self.flip <= 1.0:
            raise ValueError("Augment: flip is a probability in [0, 1] (got %r)" % self.flip)
        for name in ("brightness", "contrast", "saturation"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError("Augment: %s is a strength in [0, 1] (got %r)" % (name, getattr(self, name)))

    @property
    def is_identity(self):
        """every draw is the identity record: the loader then uses the plain kernel"""
        return (self.scale == (1.0, 1.0) and self.ratio == (1.0, 1.0) and self.flip == 0.0 and self.brightness == 0.0
                and self.contrast == 0.0 and self.saturation == 0.0)

    def config(self):
        """the fp32 values the device draws from (scnattn_augment_config)"""
        return AugmentConfig(self.scale[0], self.scale[1], self.ratio[0], self.ratio[1], self.flip, self.brightness,
                             self.contrast, self.saturation)

    def draw(self, sid, epoch, H, W):
        """sid: int64 [n] sample ids on the GPU -> params float32 [n, 8] = (x0, y0, w, h, flip, bright, contr, sat)"""
        if sid.dtype != torch.int64 or sid.dim() != 1 or not sid.is_contiguous():
            raise RuntimeError("Augment.draw: sid must be a contiguous int64 vector")
        require_cuda(sid)
        params = torch.empty((sid.numel(), AUGMENT_NPARAM), device=sid.device, dtype=torch.float32)
        cfg = self.config()
        call("scnattn_augment_draw", stream_of(sid), sid.numel(), ptr(sid), int(epoch), self.seed & 0xFFFFFFFFFFFFFFFF,
             C.byref(cfg), int(H), int(W), ptr(params))
        return params

    def __repr__(self):
        return ("Augment(scale=%r, ratio=%r, flip=%r, brightness=%r, contrast=%r, saturation=%r, seed=%r)"
                % (self.scale, self.ratio, self.flip, self.brightness, self.contrast, self.saturation, self.seed))


def identity_params(n, H, W, device):
    """the record that changes nothing, n times: (0, 0, W, H, 0, 1, 1, 1)"""
    return torch.tensor([0.0, 0.0, W, H, 0.0, 1.0, 1.0, 1.0], dtype=torch.float32, device=device).repeat(n, 1)


def _check_src(what, src):
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_contiguous():
        raise RuntimeError("%s: src must be a contiguous uint8 [N, 3, H, W] tensor" % what)
    if src.shape[1] != 3:
        raise RuntimeError("%s: images must have C = 3 planes (got %d)" % (what, src.shape[1]))


def mean_grey(src, return_sums=False):
    """src: uint8 [N, 3, H, W] on the GPU -> grey float32 [N], the mean of 0.299 R + 0.587 G + 0.114 B over the image on the
    0..1 scale (exact integer sums, one fp64 evaluation rounded to fp32); with return_sums also the int64 [N, 3] byte sums."""
    _check_src("mean_grey", src)
    require_cuda(src)
    N, _, H, W = src.shape
    grey = torch.empty(N, device=src.device, dtype=torch.float32)
    sums = torch.empty((N, 3), device=src.device, dtype=torch.int64) if return_sums else None
    call("scnattn_u8_mean_grey", stream_of(src), ptr(src), N, H * W, ptr(sums), ptr(grey))
    return (grey, sums) if return_sums else grey


def _triple(name, v, fill):
    v = np.full(3, fill, dtype=np.float32) if v is None else np.asarray(v, dtype=np.float32)
    if v.shape != (3,):
        raise ValueError("gather_augment: %s must hold 3 values" % name)
    return (C.c_float * 3)(*v.tolist())


def gather_augment(src, idx, params, mean, std, grey=None, dtype=torch.float32, channels_last=False, out=None):
    """src: uint8 [N, 3, H, W] on the GPU; idx: int64 [n] rows to take (None: rows 0..n-1); params: float32 [n, 8], from
    `Augment.draw` or hand-made; mean, std: 3 values each (None: 0 and 1, i.e. only the `/ 255`); grey: `mean_grey(src)`, or
    None to skip the contrast step.  Returns the augmented, normalised batch [n, 3, H, W] in `dtype` (float32 / bfloat16);
    `channels_last` selects the memory format, as for `gather_normalize`."""
    _check_src("gather_augment", src)
    N, _, H, W = src.shape
    if params.dtype != torch.float32 or params.dim() != 2 or params.shape[1] != AUGMENT_NPARAM or not params.is_contiguous():
        raise RuntimeError("gather_augment: params must be a contiguous float32 [n, %d] tensor" % AUGMENT_NPARAM)
    n = params.shape[0]
    if idx is not None:
        if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
            raise RuntimeError("gather_augment: idx must be a contiguous int64 vector")
        if idx.numel() != n:
            raise RuntimeError("gather_augment: %d rows but %d parameter records" % (idx.numel(), n))
    elif n > N:
        raise RuntimeError("gather_augment: more parameter records than source rows")
    if grey is not None and (grey.dtype != torch.float32 or tuple(grey.shape) != (N,) or not grey.is_contiguous()):
        raise RuntimeError("gather_augment: grey must be float32 [N], one value per source image")
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("gather_augment: dtype must be float32 or bfloat16")
    m, s = _triple("mean", mean, 0.0), _triple("std", std, 1.0)
    if any(x == 0.0 for x in s):
        raise ValueError("std evaluated to zero after conversion to torch.float32, leading to division by zero.")
    require_cuda(src, idx, params, grey, out)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    if out is None:
        out = torch.empty((n, 3, H, W), device=src.device, dtype=dtype, memory_format=fmt)
    elif (out.dtype != dtype or tuple(out.shape) != (n, 3, H, W) or out.device != src.device
          or not out.is_contiguous(memory_format=fmt)):
        raise RuntimeError("gather_augment: out does not match the batch")
    call("scnattn_u8_gather_augment", stream_of(src), ptr(src), N, ptr(idx), n, H, W, ptr(params), ptr(grey), m, s, ptr(out),
         int(dtype == torch.bfloat16), int(bool(channels_last)))
    return out
