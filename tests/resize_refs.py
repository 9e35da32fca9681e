"""TEST REFERENCE ONLY (never imported by the package): Pillow's 8-bit bilinear resize restated in numpy, the way
`PIL.Image.resize((OW, OH), resample=BILINEAR)` -- which is what the reference's `scipy.misc.imresize(img, (OH, OW))`
calls (inference.py:37, utils/dataset.py:372) -- computes it for an "L" or "RGB" image:

  * `precompute_coeffs`: per output index the bounds [xmin, xmin + n) and the normalised triangle weights, in double;
  * `normalize_coeffs_8bpc`: weights -> integers with 22 fraction bits;
  * `ImagingResampleHorizontal_8bpc`, then `ImagingResampleVertical_8bpc`: clip8((2^21 + sum coeff * byte) >> 22),
    the horizontal result rounded to uint8 before the vertical pass reads it; a pass whose axis keeps its size is
    skipped.

The table function is a plain per-output loop, written apart from the vectorised `scnattn.data.resize_taps` it checks.
Pinned by tests/golden/resize_pillow.npz (outputs of Pillow 12.2.0, tools/gen_resize_golden.py)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# source (H, W) -> target (OH, OW), grey?  The shapes of the issue; the last two are the workload's.
SMALL_SHAPES = [((7, 5), (3, 4)), ((5, 9), (16, 16)), ((16, 16), (16, 7)), ((13, 16), (5, 16)), ((16, 16), (16, 16)),
                ((33, 47), (16, 16)), ((1, 1), (4, 4)), ((3, 1000), (8, 8)), ((257, 255), (256, 256))]
WORKLOAD_SHAPES = [((375, 500), (256, 256), False), ((480, 640), (256, 256), True)]
AXIS_PAIRS = sorted({(s[a], t[a]) for s, t in SMALL_SHAPES for a in (0, 1)} |
                    {(s[a], t[a]) for s, t, _ in WORKLOAD_SHAPES for a in (0, 1)})


def taps(in_size, out_size):
    """(xmin[out], n[out], coeff[out, ksize]) as Python ints, one output index at a time."""
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
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
            a = (x + xmin - center + 0.5) * ss
            if a < 0.0:
                a = -a
            w = 1.0 - a if a < 1.0 else 0.0
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        xmins.append(xmin)
        ns.append(xmax)
        coeffs.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
    return np.asarray(xmins, np.int32), np.asarray(ns, np.int32), np.asarray(coeffs, np.int32).reshape(out_size, ksize)


def _pass(img, out_size, axis):
    """One 8-bit pass along `axis` of an (H, W, C) uint8 array."""
    xmin, n, coeff = taps(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for i in range(out_size):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(int(n[i])):
            acc += int(coeff[i, k]) * src[int(xmin[i]) + k]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def resize(img, size):
    """img: uint8 (H, W) or (H, W, 3); size: (OH, OW).  Returns what `np.asarray(Image.fromarray(img).resize((OW, OH), 2))`
    returns, same rank as the input."""
    OH, OW = size
    a = img[:, :, None] if img.ndim == 2 else img
    if a.shape[1] != OW:
        a = _pass(a, OW, 1)
    if a.shape[0] != OH:
        a = _pass(a, OH, 0)
    return a[:, :, 0] if img.ndim == 2 else a


def rows(img, size):
    """uint8 (3, OH, OW): the reference's stored row -- grey replicated to three planes, resized, transposed
    (inference.py:34-38)."""
    if img.ndim == 2:
        img = np.concatenate([img[:, :, None]] * 3, axis=2)
    return np.ascontiguousarray(resize(img, size).transpose(2, 0, 1))


def random_image(shape, seed, grey=False):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=shape if grey else shape + (3,)).astype(np.uint8)


def checker_image(shape, grey=False):
    """0 / 255 checkerboard (phase shifted per channel): every rounding and the clamp carry weight."""
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    if grey:
        return (((yy + xx) & 1) * 255).astype(np.uint8)
    return np.stack([(((yy + xx + c) & 1) * 255) for c in range(3)], axis=2).astype(np.uint8)
