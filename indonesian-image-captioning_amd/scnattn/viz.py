"""Attention overlays on the device: the per-word pictures of the reference's utils/vizualize.py:11-51.

Reference, per image on the host: `Image.resize([336, 336], LANCZOS)`, then per word
`skimage.transform.pyramid_expand(alpha, upscale=24, sigma=8)` (`skimage.transform.resize(alpha, [336, 336])` with
`smooth=False`) and a matplotlib `imshow(alpha, alpha=0.8)` over the photograph (`alpha=0` for the first word).

Here: one LANCZOS resize launch for the batch (`data.resize_u8(..., filter="lanczos")`, Pillow's bytes) and two launches
of csrc/overlay.hip for all maps of all images.  The smoothing is DEFINED as
`scipy.ndimage.zoom(a, upscale, order=1, mode='mirror', grid_mode=True)` followed by
`scipy.ndimage.gaussian_filter(., sigma, mode='reflect', truncate=4.0)` -- what skimage >= 0.19 is believed to compute
for `pyramid_expand(order=1, mode='reflect')`, unconfirmed.  Both steps are linear and separable, so the
result is `M_v . a . M_h^T` with one operator per axis, built here in numpy (the package does not import scipy).
matplotlib's rendering (figure, text, the Greys_r table, screen resampling) is not reproduced: the output is one uint8
RGB array per word, `(1 - beta) * photograph + beta * 255 * (S - min S) / (max S - min S)` rounded half up.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import data
from ._lib import OVERLAY_MAX_MAP, OVERLAY_MAX_OUT, call, lib, ptr, require_cuda, stream_of


def _zoom_operator(n, out):
    """[out, n]: linear interpolation at the input coordinate (o + 0.5) * n / out - 0.5 of output o (grid_mode), indices
    outside the axis mirrored about the edge samples (d c b | a b c d | c b a)."""
    Z = np.zeros((out, n), np.float64)
    period = 2 * n - 2
    for o in range(out):
        c = (o + 0.5) * (np.float64(n) / np.float64(out)) - 0.5
        f = math.floor(c)
        t = c - f
        for idx, wgt in ((f, 1.0 - t), (f + 1, t)):
            p = 0 if n == 1 else idx % period
            if p >= n:
                p = period - p
            Z[o, p] += wgt
    return Z


def _gauss_operator(n, sigma, truncate):
    """[n, n]: correlation with the normalised Gaussian of radius int(truncate * sigma + 0.5), the axis extended by
    reflection about its edges (d c b a | a b c d | d c b a), as often as the kernel needs."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (np.float64(sigma) * np.float64(sigma)) * x ** 2)
    g = g / g.sum()
    G = np.zeros((n, n), np.float64)
    for y in range(n):
        for k in range(-radius, radius + 1):
            p = (y + k) % (2 * n)
            if p >= n:
                p = 2 * n - 1 - p
            G[y, p] += g[k + radius]
    return G


@functools.lru_cache(maxsize=64)
def expand_operator(n, upscale, sigma, truncate=4.0):
    """The fp64 operator [ceil(upscale * n), n] of one axis: zoom (order 1, mirror, grid mode), then, unless sigma is
    None (the reference's `smooth=False`), the Gaussian (reflect, `truncate`).  Entries >= 0, rows sum to 1.  Cached per
    argument tuple; the array is read-only."""
    n = int(n)
    if n < 1 or not upscale > 0 or (sigma is not None and not sigma > 0):
        raise ValueError("expand_operator: n >= 1, upscale > 0 and sigma > 0 (or None) are required")
    out = int(math.ceil(upscale * n))
    M = _zoom_operator(n, out)
    if sigma is not None:
        M = _gauss_operator(out, sigma, truncate) @ M
    M.setflags(write=False)
    return M


_DEV_OPS = {}


def _operator_on(device, n, upscale, sigma):
    """`expand_operator` rounded once to fp32, on the device; uploaded once per (device, arguments)."""
    key = (str(device), n, upscale, sigma)
    if key not in _DEV_OPS:
        _DEV_OPS[key] = torch.from_numpy(expand_operator(n, upscale, sigma).astype(np.float32)).to(device)
    return _DEV_OPS[key]


def _maps(alphas, device=None):
    a = alphas if isinstance(alphas, torch.Tensor) else torch.as_tensor(np.asarray(alphas, dtype=np.float32))
    if a.dim() != 3 or a.shape[0] < 1:
        raise ValueError("scnattn.viz: attention maps must be [n >= 1, h, w] (got %r)" % (tuple(a.shape),))
    if device is not None:
        a = a.to(device)
    require_cuda(a)
    return a.float().contiguous()


def _expand(a, upscale, sigma, want_maps, want_range):
    n, h, w = a.shape
    if not (1 <= h <= OVERLAY_MAX_MAP and 1 <= w <= OVERLAY_MAX_MAP):
        raise ValueError("scnattn.viz: map sides must be in [1, %d]" % OVERLAY_MAX_MAP)
    Mv, Mh = _operator_on(a.device, h, upscale, sigma), _operator_on(a.device, w, upscale, sigma)
    OH, OW = Mv.shape[0], Mh.shape[0]
    if not (OH <= OVERLAY_MAX_OUT and OW <= OVERLAY_MAX_OUT):
        raise ValueError("scnattn.viz: expanded sides must be at most %d (got %d x %d)" % (OVERLAY_MAX_OUT, OH, OW))
    S = torch.empty((n, OH, OW), device=a.device, dtype=torch.float32) if want_maps else None
    lohi = torch.empty((n, 2), device=a.device, dtype=torch.float32) if want_range else None
    partial = torch.empty((n, lib().scnattn_attn_strips(OH), 2), device=a.device, dtype=torch.float32)
    call("scnattn_attn_expand", stream_of(a), ptr(a), n, h, w, ptr(Mv), ptr(Mh), OH, OW, ptr(S), ptr(lohi), ptr(partial))
    return Mv, Mh, S, lohi, partial


def pyramid_expand(alphas, upscale=24, sigma=8, return_range=False):
    """alphas: device tensor [n, h, w].  Returns the smoothed maps, fp32 [n, ceil(h * upscale), ceil(w * upscale)];
    sigma None: the zoom alone.  return_range: also the device tensor [n, 2] of each map's {min, max}."""
    _, _, S, lohi, _ = _expand(_maps(alphas), upscale, sigma, True, return_range)
    return (S, lohi) if return_range else S


def overlay_maps(photos, alphas, img_index, beta, upscale=24, sigma=8, recompute=False):
    """photos: uint8 [N, 3, OH, OW] on the device (`data.resize_u8`); alphas: device tensor [n, h, w] with OH, OW =
    upscale * (h, w); img_index: n host integers, the photograph of each map; beta: n host floats, the weight of each
    map over its photograph.  Returns uint8 [n, OH, OW, 3].  Two launches: the smoothed maps with their min / max, then the
    blend, which reads the fp32 maps back (4 * OH * OW bytes of scratch per map).  recompute=True: the first launch
    stores no maps and the blend recomputes them with the same code -- the same bytes out and no scratch, measured 0.34
    against 0.27 ms for 384 maps (profiles/overlay_bench.txt), so it is not the default."""
    a = _maps(alphas)
    require_cuda(photos)
    if photos.dtype != torch.uint8 or photos.dim() != 4 or photos.shape[1] != 3 or not photos.is_contiguous():
        raise RuntimeError("overlay_maps: photos must be a contiguous uint8 [N, 3, OH, OW] tensor")
    n, h, w = a.shape
    want = (int(math.ceil(upscale * h)), int(math.ceil(upscale * w)))
    if tuple(photos.shape[2:]) != want:
        raise ValueError("overlay_maps: the photographs are %d x %d, the expanded %d x %d maps %d x %d"
                         % (photos.shape[2], photos.shape[3], h, w, want[0], want[1]))
    idx = np.ascontiguousarray(img_index, dtype=np.int32).reshape(-1)
    b = np.ascontiguousarray(beta, dtype=np.float32).reshape(-1)
    if idx.size != n or b.size != n:
        raise ValueError("overlay_maps: img_index and beta need one entry per map")
    if idx.min() < 0 or idx.max() >= photos.shape[0]:
        raise ValueError("overlay_maps: an img_index is outside 0..%d" % (photos.shape[0] - 1))
    Mv, Mh, S, _, partial = _expand(a, upscale, sigma, not recompute, False)
    side = torch.from_numpy(np.concatenate([idx.view(np.float32), b])).to(a.device, non_blocking=True)   # one copy
    out = torch.empty((n,) + want + (3,), device=a.device, dtype=torch.uint8)
    call("scnattn_attn_overlay", stream_of(a), ptr(a), n, h, w, ptr(Mv), ptr(Mh), want[0], want[1], ptr(S), ptr(partial),
         ptr(photos), photos.shape[0], idx.ctypes.data_as(C.c_void_p), ptr(side), C.c_void_p(side.data_ptr() + 4 * n),
         ptr(out))
    return out


def attention_overlays(images, alphas, size=(336, 336), upscale=24, sigma=8, weight=0.8, smooth=True, device=None):
    """images: decoded uint8 arrays, as for `data.resize_u8`; alphas: per image one [T_i, h, w] tensor, array or nested
    list, as `sample_batch` returns them.  Returns per image one uint8 device tensor [T_i, OH, OW, 3]: the photograph
    resized with Pillow's LANCZOS, under each smoothed (smooth=False: only zoomed) map at `weight`; map 0 of an image,
    the `<start>` row of ones, at weight 0 (utils/vizualize.py:45-48).  size must be upscale x the map size.  One resize
    launch for the batch, two overlay launches for all maps."""
    images, alphas = list(images), list(alphas)
    if len(images) != len(alphas) or not images:
        raise ValueError("attention_overlays: one set of maps per image is required")
    if device is None:
        on = [a.device for a in alphas if isinstance(a, torch.Tensor) and a.is_cuda]
        device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    maps = [_maps(a, device) for a in alphas]
    h, w = maps[0].shape[1:]
    if any(tuple(m.shape[1:]) != (h, w) for m in maps):
        raise ValueError("attention_overlays: all maps of a batch must have one size")
    size = (int(size[0]), int(size[1]))
    if size != (int(math.ceil(upscale * h)), int(math.ceil(upscale * w))):
        raise ValueError("attention_overlays: size %r is not upscale = %r times the %d x %d maps" % (size, upscale, h, w))
    counts = [m.shape[0] for m in maps]
    photos = data.resize_u8(images, size, device=device, filter="lanczos")
    idx = np.repeat(np.arange(len(images), dtype=np.int32), counts)
    beta = np.concatenate([[0.0] + [float(weight)] * (c - 1) for c in counts]).astype(np.float32)
    out = overlay_maps(photos, torch.cat(maps), idx, beta, upscale, sigma if smooth else None)
    return list(out.split(counts))
