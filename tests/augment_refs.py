"""fp64 references, cases and judges of the augmentation kernels (csrc/augment.hip: scnattn_u8_mean_grey,
scnattn_augment_draw, scnattn_u8_gather_augment), shared by tests/test_augment_refs.py (CPU: the references against torch's
own fp64 ops, the judges against torch's CPU fp32 evaluation and against planted defects) and tests/test_gpu_augment.py (the
kernels and the loader).  The references are index arithmetic, not the torch ops they are held to.  Philox comes from
tests/rollout_refs.py.

What is computed (this project's own semantics: neither the reference nor torchvision has them; include/scnattn.h):
  mean grey   SR, SG, SB = integer byte sums of the planes; grey = (0.299 SR + 0.587 SG + 0.114 SB) / (255 HW)
  draw        u_k = (word_k >> 8) 2^-24 of Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (q, sid & 0xffffffff,
              sid >> 32, epoch); q = 0: u0 area, u1 aspect, u2 x offset, u3 y offset; q = 1: u4 flip, u5 brightness, u6
              contrast, u7 saturation.
              a = scale_lo + u0 (scale_hi - scale_lo);  r = exp(log ratio_lo + u1 (log ratio_hi - log ratio_lo))
              w = min(W, W sqrt(a r));  h = min(H, H sqrt(a / r));  x0 = u2 (W - w);  y0 = u3 (H - h);  flip = u4 < flip_p
              bright / contr / sat = 1 + (2 u - 1) strength.          record = (x0, y0, w, h, flip, bright, contr, sat)
  pixel (oy, ox) of output row i, source image `row`:
              ox' = flip ? W - 1 - ox : ox
              sx = clamp(x0 + (ox' + 0.5) (w / W) - 0.5, 0, W - 1), sy likewise;  ix = floor(sx), fx = sx - ix,
              ix1 = min(ix + 1, W - 1) (the same for y)
              v_c = (top + fy (bot - top)) / 255, top = b00 + fx (b01 - b00), bot = b10 + fx (b11 - b10)
              v_c = clamp(bright v_c, 0, 1)
              m = min(1, bright grey[row]);  v_c = clamp(contr v_c + (1 - contr) m, 0, 1)          (skipped without grey)
              g = 0.299 v_R + 0.587 v_G + 0.114 v_B;  v_c = clamp(sat v_c + (1 - sat) g, 0, 1)
              out = (v_c - mean_c) / std_c;  an index outside [0, N): NaN

Bounds (u = 2^-24).
  drawn parameters  the uniforms are exact (24-bit integers times 2^-24), so flip is exact.  For an fp32 evaluation of the
              formulas: a carries 3 roundings (the difference, the product, the sum), relative 3 u scale_hi / a <= 3 u /
              scale_lo; r is behind logf and expf and is covered by the yardstick; the square root halves a relative error,
              the products with r and with W add 2 roundings and the root 1: w, h within (4 + 2 / scale_lo) u |ref| --
              counted as (8 + 2 / scale_lo) u |ref|; x0 = u2 (W - w) inherits w's error and adds the difference and the
              product: e_w + 2 u W; a colour factor is one product and one sum: 2 u (1 + strength).  On top, per column,
              4 x the worst error of torch's CPU fp32 evaluation of the same formulas on the case (exp / log / sqrt), as
              judge_probs of tests/taghead_refs.py does for expf.
  pixels      against fp64 AT THE STORED fp32 parameters (and grey, mean, std).
              Coordinates: sx is w / W, a product, a sum and a difference, each a value of at most W + 1:
              delta = 4 u (max(H, W) + 1), or 0 where the case makes every one of them exact (`exact_coords`, which the
              judge verifies by evaluating the coordinates in fp32).  The blend is continuous and piecewise linear in
              (sy, sx) with slope at most D / 255, D the largest absolute difference of adjacent source bytes around the tap
              (a 5 x 5 neighbourhood of the tap's cell, so the cell next door counts when delta crosses a boundary), and the
              clamps are 1-Lipschitz: a coordinate error moves v by at most delta (Dx + Dy) / 255.  No element is left out near
              cell boundaries or clamp kinks.
              Value chain: bytes and their differences are exact; top and bot carry 2 roundings each (weights 1 - fy and fy:
              2 together), the vertical blend 3 more, the division 1: e = 6 u on a value of at most 1.
              brightness   e <- |bright| e + u |bright v|
              contrast     e_m = u |bright grey|;  e <- |contr| e + |1 - contr| e_m + u (|contr v| + 2 |(1 - contr) m| + |lin|)
              saturation   e_g = sum_c w_c e_c + 5 u g (three rounded constants and products, two sums);
                           e <- |sat| e + |1 - sat| e_g + u (|sat v| + 2 |(1 - sat) g| + |lin|)
              normalise    e <- (e + u |v - mean|) / |std| + u |out|
              and 1 % on the total for the second-order terms (a rounding of a value that is itself off by e).  A fused
              multiply-add only removes roundings.
  bf16        b + 2^-8 (|ref| + b): one round to nearest even on top of the fp32 value, as elsewhere in the project.
  mean grey   the sums exactly; grey within 1 fp32 ulp of the fp64 value (one rounding of an fp64 result that may itself be a
              few fp64 ulps off)."""
import numpy as np
import torch

import rollout_refs as RR
from kernel_harness import U, _bound_ok, _note

F64 = torch.float64
F32 = torch.float32
BF = torch.bfloat16
WG = (0.299, 0.587, 0.114)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (N, H, W, n): every pixel on a border; not square, W no multiple of 16; repeated rows and one out of range; the real row size
SHAPES = ((7, 4, 4, 3), (7, 8, 24, 4), (7, 32, 32, 5), (7, 256, 256, 2))
CFG_DEFAULT = (0.6, 1.0, 3.0 / 4.0, 4.0 / 3.0, 0.5, 0.2, 0.2, 0.2)
CFG_EXTREME = (0.05, 1.0, 0.25, 4.0, 1.0, 1.0, 1.0, 1.0)
CFG_NARROW = (0.3, 0.3, 2.0, 2.0, 0.0, 0.0, 0.5, 0.0)
CONFIGS = {"default": CFG_DEFAULT, "extreme": CFG_EXTREME, "narrow": CFG_NARROW}


def f32(x):
    """the fp32 value of a Python number, as a Python float"""
    return float(np.float32(x))


# ---- cases --------------------------------------------------------------------------------------------------------------
def gen_source(kind, N, H, W, seed=0):
    """uint8 [N, 3, H, W]: "random" bytes (the largest adjacent differences) or "ramp", a smooth ramp with +-2 of noise"""
    rng = np.random.RandomState(seed * 7919 + N * 131 + H * 17 + W + (0 if kind == "random" else 1))
    if kind == "random":
        a = rng.randint(0, 256, size=(N, 3, H, W))
        a[0, :, 0, :2] = [[0, 255]] * 3
    else:
        y, x = np.mgrid[0:H, 0:W]
        base = (x * 200.0 / max(W - 1, 1) + y * 50.0 / max(H - 1, 1))[None, None]
        a = base * (0.5 + 0.5 * rng.rand(N, 3, 1, 1)) + rng.randint(-2, 3, size=(N, 3, H, W))
    return torch.from_numpy(np.clip(a, 0, 255).astype(np.uint8))


def gen_idx(N, n):
    """rows to take: the last, repeats, and for n >= 5 one index outside [0, N)"""
    rows = [N - 1, 0, 0, 2, N, 1, -1][:n]
    return torch.tensor(rows, dtype=torch.int64)


def table(n, H, W, x0=0.0, y0=0.0, w=None, h=None, flip=0.0, bright=1.0, contr=1.0, sat=1.0):
    """n copies of one record, float32 [n, 8]"""
    rec = [x0, y0, W if w is None else w, H if h is None else h, flip, bright, contr, sat]
    return torch.tensor(rec, dtype=F32).repeat(n, 1)


def tables(n, H, W):
    """name -> (params [n, 8], exact_coords) of the hand-made tables of the GPU module"""
    t = {
        "identity": (table(n, H, W), True),
        "flip": (table(n, H, W, flip=1.0), True),
        "half": (table(n, H, W, x0=W // 4, y0=H // 4, w=W / 2, h=H / 2), True),              # dyadic: sx exact
        "flush": (table(n, H, W, x0=W - W / 2, y0=H - H / 2, w=W / 2, h=H / 2, flip=1.0), True),   # right and bottom edges
        "smallest": (table(n, H, W, x0=0.37 * W, y0=0.41 * H, w=W * (0.05 * 0.25) ** 0.5, h=H * (0.05 / 0.25) ** 0.5), False),   # CFG_EXTREME at u0 = u1 = 0
        "colour": (table(n, H, W, x0=0.11 * W, y0=0.07 * H, w=0.77 * W, h=0.83 * H, bright=1.4, contr=0.6, sat=1.7), False),
        "dark": (table(n, H, W, x0=0.2 * W, w=0.7 * W, flip=1.0, bright=0.7, contr=1.8, sat=0.3), False),
    }
    mixed = torch.cat([t[k][0][:1] for k in ("colour", "half", "dark", "flip", "smallest", "identity", "flush")])[:n]
    t["mixed"] = (mixed.contiguous(), False)
    return t


# ---- mean grey ----------------------------------------------------------------------------------------------------------
def mean_grey_ref(src):
    """src uint8 [N, 3, H, W] -> (sums int64 [N, 3], grey fp64 [N])"""
    N, _, H, W = src.shape
    flat = src.reshape(N, 3, H * W).to(torch.int64)
    if H * W <= 1024:                    # index arithmetic where it is affordable; integer sums have one value anyway
        sums = torch.zeros(N, 3, dtype=torch.int64)
        for q in range(H * W):
            sums += flat[:, :, q]
    else:
        sums = flat.sum(dim=2)
    s = sums.to(F64)
    return sums, (WG[0] * s[:, 0] + WG[1] * s[:, 1] + WG[2] * s[:, 2]) / (255.0 * H * W)


def judge_grey(kernel, sums, grey, src):
    want_s, want_g = mean_grey_ref(src)
    if sums is not None:
        assert torch.equal(sums.cpu().to(torch.int64), want_s), "%s: byte sums differ" % kernel
    ulp = torch.tensor(np.spacing(want_g.numpy().astype(np.float32)).astype(np.float64))
    _bound_ok(kernel, "grey", grey, want_g, ulp, kind="=1 fp32 ulp of the fp64 value")


def cpu32_grey(src):
    s = src.reshape(src.shape[0], 3, -1).to(torch.int64).sum(dim=2).to(F64)
    return ((WG[0] * s[:, 0] + WG[1] * s[:, 1] + WG[2] * s[:, 2]) / (255.0 * src.shape[2] * src.shape[3])).to(F32)


# ---- the draw -----------------------------------------------------------------------------------------------------------
def uniforms(seed, epoch, sid):
    """sid: int64 sequence -> fp64 [n, 8], exact"""
    sid = np.asarray(sid, dtype=np.int64).astype(np.uint64)
    lo, hi = sid & np.uint64(0xFFFFFFFF), sid >> np.uint64(32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = []
    for q in (0, 1):
        words += RR.philox4x32_10((np.full(sid.shape, q), lo, hi, np.full(sid.shape, epoch)), key)
    bits = np.stack(words, axis=1)
    return torch.from_numpy((bits >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)


def cfg32(cfg):
    """the fp32 values of a configuration (what the device is given), as Python floats"""
    return tuple(f32(x) for x in cfg)


def draw_eval(cfg, u, H, W, dtype):
    """the formulas in `dtype` on the fp32 configuration values"""
    c = [torch.tensor(x, dtype=dtype) for x in cfg32(cfg)]
    u = u.to(dtype)
    a = c[0] + u[:, 0] * (c[1] - c[0])
    r = torch.exp(torch.log(c[2]) + u[:, 1] * (torch.log(c[3]) - torch.log(c[2])))
    Wt, Ht = torch.tensor(float(W), dtype=dtype), torch.tensor(float(H), dtype=dtype)
    w = torch.minimum(Wt, Wt * torch.sqrt(a * r))
    h = torch.minimum(Ht, Ht * torch.sqrt(a / r))
    flip = (u[:, 4].to(F32) < torch.tensor(cfg32(cfg)[4], dtype=F32)).to(dtype)
    col = [u[:, 2] * (Wt - w), u[:, 3] * (Ht - h), w, h, flip]
    col += [1.0 + (2.0 * u[:, 5 + k] - 1.0) * c[5 + k] for k in range(3)]
    return torch.stack(col, dim=1)


def draw_ref(cfg, seed, epoch, sid, H, W):
    return draw_eval(cfg, uniforms(seed, epoch, sid), H, W, F64)


def cpu32_draw(cfg, seed, epoch, sid, H, W):
    return draw_eval(cfg, uniforms(seed, epoch, sid), H, W, F32)


def judge_params(kernel, got, cfg, seed, epoch, sid, H, W):
    want = draw_ref(cfg, seed, epoch, sid, H, W)
    yard = (cpu32_draw(cfg, seed, epoch, sid, H, W).to(F64) - want).abs().max(dim=0)[0]
    c = cfg32(cfg)
    k = (8.0 + 2.0 / c[0]) * U
    ew, eh = k * want[:, 2].abs(), k * want[:, 3].abs()
    counted = torch.stack([ew + 2 * U * W, eh + 2 * U * H, ew, eh, torch.zeros_like(ew)] +
                          [torch.full_like(ew, 2 * U * (1.0 + c[5 + j])) for j in range(3)], dim=1)
    bound = counted + 4.0 * yard.unsqueeze(0)
    bound[:, 4] = 0.0
    got = got.cpu()
    assert torch.equal(got[:, 4].to(F64), want[:, 4]), "%s: flip differs" % kernel
    _bound_ok(kernel, "params", got, want, bound, kind="=counted roundings + 4 x CPU-fp32 worst error per column")
    _note(kernel, "flip", 0.0, "=exact")
    g = got.to(F64)                      # what every drawn record satisfies
    assert bool((g[:, 2] <= W).all() and (g[:, 3] <= H).all() and (g[:, 2] > 0).all() and (g[:, 3] > 0).all())
    assert bool((g[:, 0] >= 0).all() and (g[:, 1] >= 0).all())


# ---- pixels -------------------------------------------------------------------------------------------------------------
def axis_taps(off, crop, size, dtype, flip=False, defect=None):
    """i0, i1 (int64 [size]) and f ([size], dtype) of every output position of one axis"""
    o = torch.arange(size, dtype=dtype)
    if flip:
        o = (size - o if defect == "mirror" else size - 1 - o)
    off, crop = torch.tensor(off, dtype=dtype), torch.tensor(crop, dtype=dtype)
    k = crop / torch.tensor(float(size), dtype=dtype)
    s = off + (o if defect == "half" else o + 0.5) * k - (0.0 if defect == "half" else 0.5)
    if defect == "edge":                 # indices clamped instead of the coordinate, and the neighbour not at all
        s = s.clamp(min=0.0)
        fl = s.floor()
        i0 = fl.long().clamp(max=size - 1)
        return i0, i0 + 1, s - fl
    s = s.clamp(0.0, float(size - 1))
    i0 = s.floor().long()
    return i0, (i0 + 1).clamp(max=size - 1), s - i0.to(dtype)


def _local_max(d):
    """d [3, H, W] -> max over the 5 x 5 neighbourhood of every position"""
    return torch.nn.functional.max_pool2d(d.unsqueeze(0), 5, stride=1, padding=2).squeeze(0)


def image_eval(img, rec, grey, mean, std, dtype, defect=None, delta=0.0):
    """one output image [3, H, W] in `dtype` from the source image img (uint8 [3, H, W]) and the record rec (8 Python floats
    holding fp32 values); grey: the source image's fp32 mean grey as a Python float, or None.  With dtype fp64 also the
    bound, for coordinates that are off by at most delta.  defect: one of the planted defects of tests/test_augment_refs.py."""
    _, H, W = img.shape
    x0, y0, w, h, flip, bright, contr, sat = (float(v) for v in rec)
    b = img.to(dtype)
    iy, iy1, fy = axis_taps(y0, h, H, dtype, defect=defect if defect == "half" else None)
    ix, ix1, fx = axis_taps(x0, w, W, dtype, flip=flip != 0.0, defect=defect)
    flat = torch.cat([b.reshape(3, H * W), b.new_zeros(3, 1)], dim=1)          # one element past the end for "edge"
    at = lambda r, c: flat[:, (r[:, None] * W + c[None, :]).reshape(-1)].reshape(3, H, W)      # noqa: E731
    b00, b01, b10, b11 = at(iy, ix), at(iy, ix1), at(iy1, ix), at(iy1, ix1)
    fxr, fyr = fx[None, None, :], fy[None, :, None]
    top, bot = b00 + fxr * (b01 - b00), b10 + fxr * (b11 - b10)
    v = (top + fyr * (bot - top)) / 255.0
    ev = None
    if dtype == F64:
        dx = torch.zeros_like(b)
        dx[:, :, :-1] = (b[:, :, 1:] - b[:, :, :-1]).abs()
        dy = torch.zeros_like(b)
        dy[:, :-1, :] = (b[:, 1:, :] - b[:, :-1, :]).abs()
        pick = lambda d: _local_max(d)[:, iy][:, :, ix]                                        # noqa: E731
        ev = 6 * U + delta * (pick(dx) + pick(dy)) / 255.0
    bt, ct, st = (torch.tensor(t, dtype=dtype) for t in (bright, contr, sat))
    one = torch.tensor(1.0, dtype=dtype)
    raw = bt * v
    if ev is not None:
        ev = bt.abs() * ev + U * raw.abs()
    v = raw if defect == "noclamp" else raw.clamp(0.0, 1.0)
    if grey is not None:
        gt = torch.tensor(grey, dtype=dtype)
        m = gt.clamp(max=1.0) if defect == "mraw" else torch.minimum(one, bt * gt)
        lin = ct * v + (one - ct) * m
        if ev is not None:
            ev = ct.abs() * ev + (one - ct).abs() * U * (bt * gt).abs() + \
                U * ((ct * v).abs() + 2 * ((one - ct) * m).abs() + lin.abs())
        v = lin.clamp(0.0, 1.0)
    wg = [torch.tensor(t, dtype=dtype) for t in (WG[::-1] if defect == "bgr" else WG)]
    g = wg[0] * v[0] + wg[1] * v[1] + wg[2] * v[2]
    lin = st * v + (one - st) * g.unsqueeze(0)
    if ev is not None:
        eg = wg[0] * ev[0] + wg[1] * ev[1] + wg[2] * ev[2] + 5 * U * g.abs()
        ev = st.abs() * ev + (one - st).abs() * eg.unsqueeze(0) + \
            U * ((st * v).abs() + 2 * ((one - st) * g.unsqueeze(0)).abs() + lin.abs())
    v = lin.clamp(0.0, 1.0)
    mt = torch.tensor([f32(t) for t in mean], dtype=dtype).view(3, 1, 1)
    sd = torch.tensor([f32(t) for t in std], dtype=dtype).view(3, 1, 1)
    out = (v - mt) / sd
    if ev is None:
        return out
    return out, 1.01 * ((ev + U * (v - mt).abs()) / sd.abs() + U * out.abs())


def batch_ref(src, idx, params, grey, mean=MEAN, std=STD, exact_coords=False):
    """fp64 reference [n, 3, H, W] (NaN rows where idx is out of range) and its per-element bound.  params: float32 [n, 8]
    (the stored records), grey: float32 [N] or None."""
    N, _, H, W = src.shape
    n = params.shape[0]
    out = torch.full((n, 3, H, W), float("nan"), dtype=F64)
    bound = torch.zeros(n, 3, H, W, dtype=F64)
    delta = 0.0 if exact_coords else 4 * U * (max(H, W) + 1)
    for i in range(n):
        row = i if idx is None else int(idx[i])
        if not 0 <= row < N:
            continue
        rec = params[i].tolist()
        if exact_coords:                 # the claim, verified: the fp32 coordinates equal the fp64 ones
            for off, crop, size, fl in ((rec[0], rec[2], W, rec[4] != 0.0), (rec[1], rec[3], H, False)):
                a, c = axis_taps(off, crop, size, F32, fl), axis_taps(off, crop, size, F64, fl)
                assert torch.equal(a[0], c[0]) and torch.equal(a[2].to(F64), c[2]), "coordinates are not exact in fp32"
        out[i], bound[i] = image_eval(src[row], rec, None if grey is None else float(grey[row]), mean, std, F64, delta=delta)
    return out, bound


def cpu32_batch(src, idx, params, grey, mean=MEAN, std=STD, defect=None, channels_last=False):
    """torch's CPU fp32 evaluation of the same formulas, [n, 3, H, W] float32; with `defect` one planted mistake.
    "nchw": a channels-last buffer filled in NCHW order."""
    N, _, H, W = src.shape
    n = params.shape[0]
    out = torch.full((n, 3, H, W), float("nan"), dtype=F32)
    for i in range(n):
        row = i if idx is None else int(idx[i])
        if 0 <= row < N:
            out[i] = image_eval(src[row], params[i].tolist(), None if grey is None else float(grey[row]), mean, std, F32,
                                defect=None if defect == "nchw" else defect)
    if defect == "nchw":
        out = out.contiguous().view(n, H, W, 3).permute(0, 3, 1, 2)
    return out


def judge_pixels(kernel, got, src, idx, params, grey, mean=MEAN, std=STD, exact_coords=False, bf16=False, ref=None):
    """got: [n, 3, H, W] (logical shape, any memory format), float32 or bfloat16 values.  ref: a (out, bound) pair of
    batch_ref for the same arguments, computed once and shared."""
    want, b = ref if ref is not None else batch_ref(src, idx, params, grey, mean, std, exact_coords)
    got = got.detach().cpu().to(F64)
    bad = want.isnan()
    assert bool((got.isnan() == bad).all()), "%s: the NaN rows are not the rows of the indices out of range" % kernel
    if bf16:
        b = b + 2.0 ** -8 * (want.abs() + b)
    keep = ~bad
    _bound_ok(kernel, "bf16" if bf16 else "fp32", got[keep], want[keep], b[keep],
              kind="=counted roundings + delta x adjacent byte difference x gains / std" + (", bf16: b + 2^-8 (|ref| + b)" if bf16 else ""))


def identity_value(src, rows, mean=MEAN, std=STD):
    """the three-rounding fp32 value of ((b / 255) - mean) / std for rows of src: float32 [n, 3, H, W]"""
    v = src[rows].to(F32) / torch.tensor(255.0, dtype=F32)
    m = torch.tensor([f32(t) for t in mean], dtype=F32).view(1, 3, 1, 1)
    s = torch.tensor([f32(t) for t in std], dtype=F32).view(1, 3, 1, 1)
    return (v - m) / s
