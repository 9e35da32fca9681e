"""fp64 references of the stem kernels of csrc/stem.hip (include/scnattn.h: scnattn_stem_tiles, scnattn_stem_conv7,
scnattn_stem_bn_relu_maxpool), the case tables of tests/test_gpu_stem_kernels.py, their seeded inputs, the judges, and a Python
mirror of the host side: stem_tiles, ldp, and the tile walk of the persistent stem_conv7_kernel (which 8 x 16 output tiles
workgroup b visits, which pixels of a ragged tile are valid).

  * z: fp64 conv2d(stride 2, padding 3) -- the definition -- with the sum bound (147 + 8) u S, S = conv2d(|x|, |w|): the zero
    padding contributes nothing, the pad tap multiplies a zero weight;
  * statistics [2][64][ldp]: slot b against the fp64 sums of (z_stored - shift), its square, over the valid pixels of the
    tiles workgroup b walked, (n + 8) u sum|terms| with n those pixels (bn_refs.judge_slots);
  * pooling: each candidate is one fma(z, scale, shift), the output the max over the in-image window and 0: bound
    u max_window(|z scale| + |shift|) (bf16 output: b + 2^-8 (|ref| + b)); a window whose candidates are all negative gives +0.0
    bit for bit.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

import bn_refs as B

U, U8, F64, cdiv = B.U, B.U8, B.F64, B.cdiv
TH, TW, WG_MAX = 8, 16, 768           # S_TH, S_TW, the persistent grid

K_Z = "=(147+8)*2^-24*conv2d(|x|,|w|)"
K_POOL = "=2^-24*max_window(|z*scale|+|shift|) (bf16: + 2^-8)"


# ==== the mirror =========================================================================================================
def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def tile_grid(N, H, W):
    Ho, Wo = out_hw(H, W)
    return cdiv(Ho, TH), cdiv(Wo, TW)


def stem_tiles(N, H, W):
    ty, tx = tile_grid(N, H, W)
    return min(N * ty * tx, WG_MAX)


def ldp(N, H, W):
    return (stem_tiles(N, H, W) + 3) & ~3


@lru_cache(maxsize=None)
def tile_walk(N, H, W):
    """-> one list per workgroup b of the tiles it visits, in order: (n, oh0, ow0, valid rows, valid columns)"""
    Ho, Wo = out_hw(H, W)
    ty, tx = tile_grid(N, H, W)
    grid = stem_tiles(N, H, W)
    walk = [[] for _ in range(grid)]
    for tile in range(N * ty * tx):
        n, rem = divmod(tile, tx * ty)
        tyi, txi = divmod(rem, tx)
        oh0, ow0 = tyi * TH, txi * TW
        walk[tile % grid].append((n, oh0, ow0, min(TH, Ho - oh0), min(TW, Wo - ow0)))
    return walk


@lru_cache(maxsize=None)
def pixel_slots(N, H, W):
    """the workgroup of every output pixel, [N * Ho * Wo] (row order of z).  Shared: never written to."""
    Ho, Wo = out_hw(H, W)
    slot = torch.full((N, Ho, Wo), -1, dtype=torch.long)
    for b, tiles in enumerate(tile_walk(N, H, W)):
        for (n, oh0, ow0, vh, vw) in tiles:
            assert bool((slot[n, oh0:oh0 + vh, ow0:ow0 + vw] == -1).all())
            slot[n, oh0:oh0 + vh, ow0:ow0 + vw] = b
    assert bool((slot >= 0).all())
    return slot.reshape(-1)


def walk_facts(N, H, W):
    walk = tile_walk(N, H, W)
    Ho, Wo = out_hw(H, W)
    tiles = [t for w in walk for t in w]
    return {"N": N, "H": H, "W": W, "Ho": Ho, "Wo": Wo, "tiles": len(tiles), "wgs": len(walk),
            "two": sum(len(w) == 2 for w in walk), "three": sum(len(w) == 3 for w in walk),
            "onerow": int(any(t[3] == 1 for t in tiles)), "onecol": int(any(t[4] == 1 for t in tiles)),
            "ragged": int(any(t[3] < TH or t[4] < TW for t in tiles)), "full": int(any(t[3] == TH and t[4] == TW for t in tiles))}


# ==== cases ==============================================================================================================
# xfmt: nchw | cl (channels-last) | crop (an NCHW view with sh > W inside a larger image, NaN in the gaps);  wfmt: nchw | cl
# stat: 0 stat_partial NULL, 1 given with stat_shift NULL, 2 both given
ConvCase = namedtuple("ConvCase", "N H W xfmt wfmt stat tags")
PoolCase = namedtuple("PoolCase", "N Hz Wz C obf tags")

CONV_CASES = [
    ConvCase(1, 1, 1, "nchw", "nchw", 2, "tiles1 Ho1 Wo1"),
    ConvCase(1, 33, 17, "cl", "cl", 1, "Ho17 Wo9 onerow tiles3"),
    ConvCase(3, 50, 70, "crop", "nchw", 2, "Ho25 Wo35 onerow ragged tiles36"),
    ConvCase(2, 17, 33, "nchw", "cl", 2, "Ho9 Wo17 onerow onecol"),
    ConvCase(2, 32, 64, "cl", "nchw", 0, "full tiles8"),
    ConvCase(2, 32, 64, "crop", "cl", 2, "full tiles8"),
    ConvCase(770, 5, 5, "nchw", "nchw", 2, "tiles770 wgs768 two2"),
    ConvCase(1600, 5, 5, "cl", "nchw", 1, "tiles1600 wgs768 three64"),
    ConvCase(770, 5, 5, "crop", "cl", 0, "tiles770 wgs768 two2"),
]
POOL_CASES = [PoolCase(N, Hz, Wz, C, obf, "")
              for i, (N, Hz, Wz) in enumerate([(1, 1, 1), (2, 2, 2), (1, 3, 3), (3, 4, 5), (2, 17, 9)])
              for (C, obf) in [((4, 8, 64)[i % 3], 0), ((8, 64, 4)[i % 3], 1)]] + [PoolCase(2, 17, 9, 4, 0, ""), PoolCase(3, 4, 5, 64, 1, "")]


def case_id(c):
    return "-".join(str(v) for v in c[:-1])


def x_layout(c):
    """element strides (sn, sc, sh, sw) of the (N, 3, H, W) window"""
    N, H, W = c.N, c.H, c.W
    if c.xfmt == "nchw":
        return (3 * H * W, H * W, W, 1)
    if c.xfmt == "cl":
        return (H * W * 3, 1, W * 3, 3)
    Hb, Wb = H + 2, W + 5
    return (3 * Hb * Wb, Hb * Wb, Wb, 1)


def w_layout(c):
    return (147, 49, 7, 1) if c.wfmt == "nchw" else (147, 1, 21, 3)


def _gen(*key):
    return torch.Generator().manual_seed(60000 + zlib.crc32(repr(key).encode()) % 100000)


@lru_cache(maxsize=None)
def conv_inputs(N, H, W):
    g = _gen("conv", N, H, W)
    return {"x": torch.randn(N, 3, H, W, generator=g), "w": torch.randn(64, 3, 7, 7, generator=g) * 147 ** -0.5,
            "shift": 1.5 + 0.1 * torch.randn(64, generator=g)}          # well away from 0: a pixel counted as -shift shows


@lru_cache(maxsize=None)
def pool_inputs(c):
    g = _gen("pool", c.N, c.Hz, c.Wz, c.C)
    C = c.C
    scale = (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.arange(C) % 2).float())      # both signs
    shift = 0.3 * torch.randn(C, generator=g)
    shift[C - 1] = -20.0                                               # every window of this channel is all negative
    return {"z": torch.randn(c.N * c.Hz * c.Wz, C, generator=g), "ss": torch.stack([scale, shift], 1).contiguous()}


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@lru_cache(maxsize=None)
def conv_ref(N, H, W):
    """-> (z [N*Ho*Wo][64], S) in fp64"""
    I = conv_inputs(N, H, W)
    x, w = I["x"].double(), I["w"].double()
    return _rows(F.conv2d(x, w, stride=2, padding=3)), _rows(F.conv2d(x.abs(), w.abs(), stride=2, padding=3))


def pool_windows(v, Hz, Wz, fill, start=-1):
    """v [N, Hz, Wz, C] -> max over the 3 x 3 / stride 2 window starting at 2 * o + start, out-of-image taps = fill;
    written as nine shifted slices"""
    Ho, Wo = out_hw(Hz, Wz)
    pad = torch.full((v.shape[0], 2 * Ho + 3, 2 * Wo + 3, v.shape[3]), fill, dtype=v.dtype)
    pad[:, 1:1 + Hz, 1:1 + Wz] = v
    out = None
    for dh in range(3):
        for dw in range(3):
            t = pad[:, 1 + start + dh:1 + start + dh + 2 * Ho:2, 1 + start + dw:1 + start + dw + 2 * Wo:2]
            out = t if out is None else torch.maximum(out, t)
    return out.reshape(-1, v.shape[3])


def pool_ref(c, I, dt=F64, start=-1, clamp=True):
    """-> (out [N*Ho*Wo][C], the window max of the candidates before the clamp at 0, the window max of |z scale| + |shift|)"""
    z, sc, sh = I["z"].to(dt).reshape(c.N, c.Hz, c.Wz, c.C), I["ss"][:, 0].to(dt), I["ss"][:, 1].to(dt)
    cand = z * sc + sh
    top = pool_windows(cand, c.Hz, c.Wz, float("-inf"), start)
    mag = pool_windows((z * sc).abs() + sh.abs(), c.Hz, c.Wz, 0.0, start)
    return (top.clamp_min(0.0) if clamp else top), top, mag


# ==== judges =============================================================================================================
def judge_conv(c, I, out, kernel, ok):
    """out: z [N*Ho*Wo][64], partial [2][64][workgroups] or None"""
    want, S = conv_ref(c.N, c.H, c.W)
    ok(kernel, "z", out["z"], want, (147 + 8) * U * S, K_Z)
    if c.stat:
        d = out["z"].double() - (I["shift"].double() if c.stat == 2 else 0.0)
        B.judge_slots(kernel, ok, out["partial"].permute(0, 2, 1), d, d * d, pixel_slots(c.N, c.H, c.W), stem_tiles(c.N, c.H, c.W))


def judge_pool(c, I, out, kernel, ok):
    want, top, mag = pool_ref(c, I)
    b = U * mag
    ok(kernel, "out", out, want, b + U8 * (want.abs() + b) if c.obf else b, K_POOL)
    neg = top < -b
    assert bool(neg.any()), "%s: no all-negative window in the case" % kernel
    assert bool((out.float().contiguous().view(torch.int32)[neg] == 0).all()), "%s: an all-negative window is not +0.0" % kernel
