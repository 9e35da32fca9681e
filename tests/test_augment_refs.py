"""CPU tests of tests/augment_refs.py: the sampling reference against torch.nn.functional.grid_sample in fp64, the uniforms
against the paper's Philox, every judge against torch's CPU fp32 evaluation of the same formulas (which must pass) and
against planted defects (which must not).  No GPU is needed; tests/test_gpu_augment.py holds the kernels to the same judges."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_refs as R
import rollout_refs as RR

F64, F32 = torch.float64, torch.float32
SMALL = [s for s in R.SHAPES if s[1] <= 32]


# ---- the uniforms ----------------------------------------------------------------------------------------------------------
def test_uniforms_are_the_papers_philox_words():
    """counter (q, sid low, sid high, epoch), key (seed low, seed high); u = (word >> 8) 2^-24, exact in fp32"""
    seed, epoch, sid = 0x299f31d0a4093822, 0x03707344, 0x13198a2e85a308d3      # the paper's third vector, q aside
    u = R.uniforms(seed, epoch, [sid, 5])
    for q in (0, 1):
        w = RR.philox4x32_10((q, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
        for k in range(4):
            assert float(u[0, 4 * q + k]) == float(int(w[k]) >> 8) * 2.0 ** -24
    # the known answer itself: counter word 0 is q, so take the vector whose first word is 0
    z = R.uniforms(0, 0, [0])
    want = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert [float(x) for x in z[0, :4]] == [float(x >> 8) * 2.0 ** -24 for x in want]
    assert bool((u.to(F32).to(F64) == u).all()) and bool((u >= 0).all()) and bool((u < 1).all())
    assert not torch.equal(R.uniforms(seed, epoch + 1, [5]), u[1:]) and not torch.equal(R.uniforms(seed + 1, epoch, [5]), u[1:])
    assert torch.equal(R.uniforms(seed, epoch, [5]), u[1:])


# ---- the sampling reference vs grid_sample ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("name", ["identity", "flip", "half", "flush", "smallest", "colour"])
def test_sampling_reference_is_grid_sample_with_border_padding(shape, name):
    """with the colour factors at 1 and no normalisation the reference is the bilinear sample alone: grid_sample in fp64,
    align_corners=False, padding_mode="border", on the grid the record describes"""
    N, H, W, n = shape
    src = R.gen_source("random", N, H, W)
    rec = R.tables(1, H, W)[name][0][0].tolist()
    rec[5:] = [1.0, 1.0, 1.0]
    got, _ = R.image_eval(src[1], rec, None, (0, 0, 0), (1, 1, 1), F64)
    x0, y0, w, h, flip = rec[:5]
    ox = torch.arange(W, dtype=F64)
    if flip:
        ox = W - 1 - ox
    sx = x0 + (ox + 0.5) * (w / W) - 0.5
    sy = y0 + (torch.arange(H, dtype=F64) + 0.5) * (h / H) - 0.5
    gx, gy = (2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1           # unnormalise of align_corners=False: ((g + 1) size - 1) / 2
    grid = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=2).unsqueeze(0)
    want = F.grid_sample(src[1:2].to(F64), grid, mode="bilinear", padding_mode="border", align_corners=False)[0] / 255.0
    assert float((got - want).abs().max()) <= 1e-12


# ---- the judges: torch's CPU fp32 evaluation passes, planted defects do not --------------------------------------------------
def _case(shape, kind, name):
    N, H, W, n = shape
    src = R.gen_source(kind, N, H, W)
    idx = R.gen_idx(N, n)
    params, exact = R.tables(n, H, W)[name]
    grey = R.cpu32_grey(src)
    return src, idx, params, grey, exact


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("name", ["identity", "flip", "half", "flush", "smallest", "colour", "dark", "mixed"])
def test_pixel_judge_accepts_cpu_fp32(shape, kind, name):
    src, idx, params, grey, exact = _case(shape, kind, name)
    for g in (grey, None):
        got = R.cpu32_batch(src, idx, params, g)
        R.judge_pixels("cpu32", got, src, idx, params, g, exact_coords=exact)
        R.judge_pixels("cpu32", got.to(R.BF), src, idx, params, g, exact_coords=exact, bf16=True)


DEFECTS = {          # defect -> a table on which it must show
    "half": "colour", "mirror": "flip", "edge": "flush", "bgr": "dark", "noclamp": "colour", "mraw": "dark", "nchw": "identity",
}


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_pixel_judge_rejects_planted_defects(shape, kind, defect):
    """half: the half-pixel offset missing; mirror: W - ox instead of W - 1 - ox; edge: indices clamped instead of the
    coordinate and ix + 1 not clamped at the right edge (it reads the next row); bgr: grey weights in BGR order; noclamp: no
    clamp after brightness; mraw: the contrast mean not brightened; nchw: a channels-last buffer filled in NCHW order"""
    src, idx, params, grey, exact = _case(shape, kind, DEFECTS[defect])
    if defect == "noclamp":              # bright pixels must exceed 1 for the clamp to matter
        src = src.clone()
        src[:, :, ::2, :] = 250
    R.judge_pixels("cpu32", R.cpu32_batch(src, idx, params, grey), src, idx, params, grey, exact_coords=exact)
    bad = R.cpu32_batch(src, idx, params, grey, defect=defect)
    for bf16 in (False, True):
        with pytest.raises(AssertionError):
            R.judge_pixels("defect", bad.to(R.BF) if bf16 else bad, src, idx, params, grey, exact_coords=exact, bf16=bf16)


def test_pixel_judge_rejects_a_wrong_nan_row_and_a_dyadic_claim_that_is_false():
    src, idx, params, grey, exact = _case(R.SHAPES[2], "random", "half")
    got = R.cpu32_batch(src, idx, params, grey)
    assert bool(got[4].isnan().all())                     # the index N
    bad = got.clone()
    bad[4] = 0.0
    with pytest.raises(AssertionError):
        R.judge_pixels("defect", bad, src, idx, params, grey, exact_coords=True)
    colour = R.tables(5, 32, 32)["colour"][0]
    with pytest.raises(AssertionError):                   # 0.77 W / W is not exact: the judge checks the claim
        R.batch_ref(src, idx, colour, grey, exact_coords=True)


def test_exact_tables_leave_only_counted_roundings():
    """identity: the fp32 evaluation IS the three-rounding value; flip: its mirror; with exact coordinates the bound has no
    coordinate term, so it stays within a few u of |ref| whatever the image"""
    N, H, W, n = R.SHAPES[1]
    src, idx = R.gen_source("random", N, H, W), R.gen_idx(N, n)
    t = R.tables(n, H, W)
    ident = R.cpu32_batch(src, idx, t["identity"][0], None)
    assert torch.equal(ident, R.identity_value(src, idx))
    assert torch.equal(R.cpu32_batch(src, idx, t["flip"][0], None), ident.flip(3))
    want, bound = R.batch_ref(src, idx, t["half"][0], None, exact_coords=True)
    assert float((bound / (want.abs() + 1.0)).max()) < 64 * R.U
    _, loose = R.batch_ref(src, idx, t["half"][0], None, exact_coords=False)
    assert float((loose / bound).max()) > 2.0


def test_colour_special_cases_of_the_reference():
    N, H, W, n = R.SHAPES[1]
    src, idx = R.gen_source("ramp", N, H, W), R.gen_idx(N, n)
    grey = R.cpu32_grey(src)
    zero, unit = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    crop = dict(x0=3.0, y0=1.0, w=17.5, h=5.25)
    out, _ = R.batch_ref(src, idx, R.table(n, H, W, bright=0.0, **crop), grey)
    m = torch.tensor([R.f32(v) for v in R.MEAN], dtype=F64).view(1, 3, 1, 1)
    s = torch.tensor([R.f32(v) for v in R.STD], dtype=F64).view(1, 3, 1, 1)
    assert torch.equal(out, ((0.0 - m) / s).expand_as(out))
    out, _ = R.batch_ref(src, idx, R.table(n, H, W, sat=0.0, bright=1.2, contr=0.7, **crop), grey, zero, unit)
    assert torch.equal(out[:, 0], out[:, 1]) and torch.equal(out[:, 1], out[:, 2])
    out, _ = R.batch_ref(src, idx, R.table(n, H, W, contr=0.0, bright=1.3, **crop), grey, zero, unit)
    want = torch.minimum(torch.tensor(1.0, dtype=F64), R.f32(1.3) * grey[idx].to(F64)).view(n, 1, 1, 1)
    assert torch.equal(out, want.expand_as(out))


# ---- the drawn parameters ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(R.CONFIGS))
@pytest.mark.parametrize("hw", [(4, 4), (8, 24), (256, 256)])
def test_param_judge_accepts_cpu_fp32_and_rejects_defects(cfg, hw):
    H, W = hw
    c = R.CONFIGS[cfg]
    sid = [0, 1, 2, 77, (1 << 40) + 3, -1] + list(range(1000, 1100))
    got = R.cpu32_draw(c, 12345, 3, sid, H, W)
    R.judge_params("cpu32", got, c, 12345, 3, sid, H, W)
    want = R.draw_ref(c, 12345, 3, sid, H, W)
    assert bool((want[:, 0] + want[:, 2] <= W * (1 + 1e-15)).all()) and bool((want[:, 1] + want[:, 3] <= H * (1 + 1e-15)).all())
    a = want[:, 2] * want[:, 3] / (H * W)                 # the area fraction where neither side was cut
    free = (want[:, 2] < W) & (want[:, 3] < H)
    assert bool((a[free] >= c[0] * (1 - 1e-6)).all()) and bool((a[free] <= c[1] * (1 + 1e-6)).all())
    for col, delta in ((0, 1e-4 * W), (3, 1e-4 * H), (6, 1e-5)):
        if float(want[:, col].abs().max()) == 0.0 or (col == 6 and c[6] == 0.0):
            continue
        bad = got.clone()
        bad[:, col] += delta
        with pytest.raises(AssertionError):
            R.judge_params("defect", bad, c, 12345, 3, sid, H, W)
    swapped = R.draw_eval(c, R.uniforms(12345, 3, sid)[:, [1, 0, 2, 3, 4, 5, 6, 7]], H, W, F32)      # area and aspect swapped
    if cfg != "narrow":
        with pytest.raises(AssertionError):
            R.judge_params("defect", swapped, c, 12345, 3, sid, H, W)
    if 0.0 < c[4] < 1.0:
        bad = got.clone()
        bad[:, 4] = 1.0 - bad[:, 4]
        with pytest.raises(AssertionError):
            R.judge_params("defect", bad, c, 12345, 3, sid, H, W)
        assert 0 < int(got[:, 4].sum()) < len(sid)


# ---- mean grey ---------------------------------------------------------------------------------------------------------------
def test_grey_judge_accepts_cpu_and_rejects_defects():
    src = R.gen_source("ramp", 7, 8, 24)
    sums, grey = R.mean_grey_ref(src)
    assert torch.equal(sums, src.to(torch.int64).sum(dim=(2, 3)))
    lum = (0.299 * src[:, 0].to(F64) + 0.587 * src[:, 1].to(F64) + 0.114 * src[:, 2].to(F64)).mean(dim=(1, 2)) / 255.0
    assert float((grey - lum).abs().max()) < 1e-13
    R.judge_grey("cpu32", sums, R.cpu32_grey(src), src)
    bgr = ((0.114 * sums[:, 0] + 0.587 * sums[:, 1] + 0.299 * sums[:, 2]).to(F64) / (255.0 * 8 * 24)).to(F32)
    with pytest.raises(AssertionError):
        R.judge_grey("defect", sums, bgr, src)
    with pytest.raises(AssertionError):
        R.judge_grey("defect", sums + 1, R.cpu32_grey(src), src)
    off = torch.from_numpy(np.nextafter(np.nextafter(R.cpu32_grey(src).numpy(), np.float32(2)), np.float32(2)))
    with pytest.raises(AssertionError):
        R.judge_grey("defect", sums, off, src)
