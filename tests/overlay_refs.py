"""TEST REFERENCE ONLY (never imported by the package): the host computations the attention overlays replace.

  * Pillow's 8-bit LANCZOS resize restated per output index (`precompute_coeffs` with `lanczos_filter`, support 3, then
    `normalize_coeffs_8bpc` and the two 8-bit passes), written apart from the vectorised `scnattn.data.resize_taps`;
    pinned by tests/golden/lanczos_pillow.npz (outputs of Pillow 12.2.0, tools/gen_lanczos_golden.py).
  * The smoothing as the scipy composition in fp64: `zoom(order=1, mode='mirror', grid_mode=True)`, then
    `gaussian_filter(sigma, mode='reflect', truncate=4.0)`.
  * The overlay value in fp64."""
import math

import numpy as np

import resize_refs as RR

PRECISION_BITS = 22
# source (H, W) -> target (OH, OW): the shapes of the golden file and of the GPU test
SMALL_SHAPES = [((7, 5), (3, 4)), ((5, 9), (16, 16)), ((16, 16), (16, 7)), ((33, 47), (16, 16)), ((1, 1), (4, 4)),
                ((3, 1000), (8, 8)), ((257, 255), (256, 256))]
GOLDEN_SHAPES = [s for s in SMALL_SHAPES if s[0] != (257, 255)] + [((3, 200), (8, 8))]
EXTRA_PAIRS = [(375, 336), (500, 336), (3, 1000), (1000, 3)]
# (n, upscale, sigma) of the operator tests; (h, w, upscale, sigma, maps) of the device tests
OPERATOR_CASES = [(14, 24, 8), (14, 24, None), (3, 4, 1.5), (5, 2, 0.7), (1, 3, 2.0), (2, 7, 30.0)]
MAP_CASES = [(14, 14, 24, 8, 2), (3, 5, 4, 1.5, 3), (1, 1, 3, 2.0, 2), (2, 2, 7, 30.0, 2), (14, 14, 24, None, 2)]


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def taps(in_size, out_size):
    """(xmin[out], n[out], coeff[out, ksize]) of Pillow's LANCZOS, one output index at a time."""
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmins, ns, coeffs = [], [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            w = lanczos((x + xmin - center + 0.5) * ss)
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        xmins.append(xmin)
        ns.append(xmax)
        coeffs.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
    return np.asarray(xmins, np.int32), np.asarray(ns, np.int32), np.asarray(coeffs, np.int32).reshape(out_size, ksize)


def apply_pass(img, table, axis):
    """One 8-bit pass of an (H, W, C) uint8 array along `axis` with the table (xmin, n, coeff)."""
    xmin, n, coeff = table
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + src.shape[1:], np.int64)
    for i in range(len(xmin)):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(int(n[i])):
            acc += int(coeff[i, k]) * src[int(xmin[i]) + k]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def resize(img, size, table=taps):
    """img: uint8 (H, W) or (H, W, 3); size: (OH, OW).  What `np.asarray(Image.fromarray(img).resize((OW, OH), LANCZOS))`
    returns; `table(in, out)` supplies the coefficients (default: the loop form above)."""
    OH, OW = size
    a = img[:, :, None] if img.ndim == 2 else img
    if a.shape[1] != OW:
        a = apply_pass(a, table(a.shape[1], OW), 1)
    if a.shape[0] != OH:
        a = apply_pass(a, table(a.shape[0], OH), 0)
    return a[:, :, 0] if img.ndim == 2 else a


def rows(img, size):
    """uint8 (3, OH, OW): grey replicated to three planes, resized, transposed -- the layout `resize_u8` returns"""
    if img.ndim == 2:
        img = np.concatenate([img[:, :, None]] * 3, axis=2)
    return np.ascontiguousarray(resize(img, size).transpose(2, 0, 1))


def images(src, grey):
    return [RR.random_image(src, 5 + src[0] + 3 * src[1], grey), RR.checker_image(src, grey)]


def expand(a, upscale, sigma):
    """The definition: fp64 scipy composition of one map (h, w) -> (h * upscale, w * upscale)."""
    import scipy.ndimage as ndi
    s = ndi.zoom(np.asarray(a, np.float64), upscale, order=1, mode="mirror", grid_mode=True)
    if sigma is not None:
        s = ndi.gaussian_filter(s, sigma, mode="reflect", truncate=4.0)
    return s


def operator(n, upscale, sigma):
    """[n * upscale, n]: the composition applied to the identity's columns"""
    return np.stack([expand(col, upscale, sigma) for col in np.eye(n)], axis=1)


def overlay(S, photo, beta):
    """fp64 overlay value v64 [OH, OW, 3] of one map: S fp64 [OH, OW], photo uint8 [3, OH, OW]."""
    lo, hi = S.min(), S.max()
    norm = np.clip((S - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.zeros_like(S)
    return (1.0 - beta) * photo.transpose(1, 2, 0).astype(np.float64) + beta * 255.0 * norm[:, :, None]


def maps(h, w, count, seed):
    """float32 [count + 2, h, w]: `count` softmax maps of scaled normal draws, one map with a single 1, one all-equal map"""
    rng = np.random.RandomState(seed)
    z = rng.randn(count, h * w) * 2.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    soft = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    one = np.zeros((1, h * w), np.float32)
    one[0, rng.randint(h * w)] = 1.0
    flat = np.full((1, h * w), np.float32(1.0 / (h * w)), np.float32)
    return np.concatenate([soft, one, flat]).reshape(count + 2, h, w)
