"""GPU tests of the attention overlays: the LANCZOS resize (csrc/resize.hip through `filter="lanczos"`) against the loop
restatement of Pillow's (tests/overlay_refs.py), the smoothed maps and the overlays of csrc/overlay.hip (through
scnattn.viz) against the fp64 scipy composition, the public path up to `Captioner(...)(images, overlays=True)`, and the
refusals, which happen before anything is launched.

Bounds.  S: |S - S64| <= (2 (k_h + k_v) + 4) 2^-24 max|a|, k the largest non-zero count per row of the case's two
operators: each operator entry rounded once to fp32, one rounding per product and per sum in the two convex stages.
Overlay: with delta = 255 beta 3 tol_S / (hi - lo) + 2^-16, an element whose fp64 value v64 has |frac(v64) - 0.5| > delta
must equal floor(v64 + 0.5), the others may differ by 1; the guard band holds at most 2 % of a case's elements and
max|a| / (hi - lo) < 4, both asserted from the reference before the device result is looked at.

The case (2, 2, 7, 30.0) cannot meet that precondition with any map: its operator's entries are 0.49999 and 0.50001, so
hi - lo <= 2.5e-5 max|a| and the ratio is above 4e4 for every 2 x 2 map (measured 40134 .. 65292 on the maps here), the
guard band 100 %.  The case stays in: its elements are held to "differ by at most 1", and -- like every case -- to
`test_overlay_is_the_documented_fp32_formula`, which is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_refs as BR
import overlay_refs as OR
import resize_refs as RR
from oracle import data_ref as DR
from scnattn import data as SD

pytestmark = pytest.mark.gpu

BETAS = (0.0, 0.8, 1.0)
NO_CAP = {(2, 2, 7, 30.0)}          # see the module docstring
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- LANCZOS resize ------------------------------------------------------------------------------------------------
def _case(src, dst, grey=False):
    key = (src, dst, grey)
    if key not in _REF:
        imgs = OR.images(src, grey)
        _REF[key] = (imgs, np.stack([OR.rows(im, dst) for im in imgs]))
    return _REF[key]


@pytest.mark.parametrize("grey", [False, True])
@pytest.mark.parametrize("src,dst", OR.SMALL_SHAPES)
def test_lanczos_small_shapes(dev, src, dst, grey):
    imgs, want = _case(src, dst, grey)
    got = SD.resize_u8(imgs, dst, device=dev, filter="lanczos")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(imgs), 3) + dst and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_lanczos_workload_shape(dev):
    imgs, want = _case((375, 500), (336, 336))
    assert torch.equal(SD.resize_u8(imgs, (336, 336), device=dev, filter="lanczos").cpu(), torch.from_numpy(want))


def _mixed():
    parts = [_case((7, 5), (16, 16)), _case((3, 1000), (16, 16)), _case((33, 47), (16, 16), True), _case((16, 16), (16, 16)),
             _case((5, 9), (16, 16))]
    return [p[0][0] for p in parts], np.stack([p[1][0] for p in parts])


def test_lanczos_mixed_batch_one_launch(dev):
    imgs, want = _mixed()
    packed = SD.pack_images(imgs, (16, 16), filter="lanczos")
    assert packed.filter == "lanczos" and [(d.H, d.W, d.C) for d in packed.desc][2] == (33, 47, 1)
    got = SD.resize_u8(packed, device=dev).cpu()
    assert torch.equal(got, torch.from_numpy(want))
    for k, im in enumerate(imgs):
        assert torch.equal(SD.resize_u8([im], (16, 16), device=dev, filter="lanczos")[0].cpu(), got[k])


@pytest.mark.parametrize("size", [(16, 16), (16, 7), (336, 336)])
def test_lanczos_normalize_equals_gather_normalize_of_the_rows(dev, size):
    imgs = [RR.random_image((33, 47), 1), RR.checker_image((16, 16)), RR.random_image((5, 9), 2, grey=True),
            RR.random_image((3, 1000), 3)]
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    u8 = SD.resize_u8(imgs, size, device=dev, filter="lanczos")
    assert torch.equal(u8[0].cpu(), torch.from_numpy(OR.rows(imgs[0], size)))
    for dtype in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            got = SD.resize_normalize(imgs, lut, size, dtype=dtype, channels_last=cl, filter="lanczos")
            want = SD.gather_normalize(u8, None, lut, dtype=dtype, channels_last=cl)
            assert got.stride() == want.stride() and torch.equal(got, want)
    assert torch.equal(SD.resize_normalize(imgs, lut, size, filter="lanczos")[0].cpu(), DR.image_item(OR.rows(imgs[0], size)))


# ---- smoothed maps -------------------------------------------------------------------------------------------------
def _maps_case(case):
    """maps fp32 [n, h, w], S64 [n, OH, OW], tol_S per map [n], photographs uint8 [2, 3, OH, OW], img_index [n]"""
    if case not in _REF:
        h, w, upscale, sigma, count = case
        a = OR.maps(h, w, count, seed=0)
        S64 = np.stack([OR.expand(m, upscale, sigma) for m in a])
        k = sum(int((OR.operator(n, upscale, sigma) != 0).sum(axis=1).max()) for n in (h, w))
        tol = (2 * k + 4) * 2.0 ** -24 * np.abs(a.astype(np.float64)).max(axis=(1, 2))
        rng = np.random.RandomState(50)
        photos = rng.randint(0, 256, (2, 3) + S64.shape[1:]).astype(np.uint8)
        _REF[case] = (a, S64, tol, photos, np.arange(len(a), dtype=np.int32) % 2)
    return _REF[case]


@pytest.mark.parametrize("case", OR.MAP_CASES)
def test_pyramid_expand_against_fp64(dev, case):
    from scnattn import viz
    h, w, upscale, sigma, _ = case
    a, S64, tol, _, _ = _maps_case(case)
    S, lohi = viz.pyramid_expand(torch.from_numpy(a).to(dev), upscale, sigma, return_range=True)
    assert S.dtype == torch.float32 and tuple(S.shape) == (len(a), h * upscale, w * upscale) and S.is_contiguous()
    S, lohi = S.cpu().numpy(), lohi.cpu().numpy()
    err = np.abs(S.astype(np.float64) - S64).max(axis=(1, 2))
    print("case %r: max |S - S64| / tol_S per map %s" % (case, np.round(err / tol, 4)))
    assert (err <= tol).all()
    assert np.array_equal(lohi[:, 0], S.min(axis=(1, 2))) and np.array_equal(lohi[:, 1], S.max(axis=(1, 2)))
    assert np.array_equal(viz.pyramid_expand(torch.from_numpy(a).to(dev), upscale, sigma).cpu().numpy(), S)
    if h == w == 1:
        assert (S == a).all()                  # a 1 x 1 map stays constant
    assert (S[-1] == a[-1, 0, 0]).all()        # so does the all-equal map


# ---- overlays ------------------------------------------------------------------------------------------------------
def _overlay(dev, case, beta):
    from scnattn import viz
    h, w, upscale, sigma, _ = case
    a, _, _, photos, idx = _maps_case(case)
    return viz.overlay_maps(torch.from_numpy(photos).to(dev), torch.from_numpy(a).to(dev), idx,
                            np.full(len(a), beta, np.float32), upscale, sigma)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", OR.MAP_CASES)
def test_overlay_against_fp64(dev, case, beta):
    a, S64, tol, photos, idx = _maps_case(case)
    b = float(np.float32(beta))
    flat = [bool(m.min() == m.max()) for m in a]
    # everything the verdict rests on comes from the reference, before the device runs
    v64, delta = [], []
    for m in range(len(a)):
        v64.append(OR.overlay(S64[m], photos[idx[m]], b))
        span = S64[m].max() - S64[m].min()
        delta.append(np.inf if flat[m] else 255.0 * b * 3.0 * tol[m] / span + 2.0 ** -16)
    v64 = np.stack(v64)
    frac = np.abs(v64 - np.floor(v64) - 0.5)
    guard = np.stack([frac[m] <= delta[m] for m in range(len(a))])
    ramps = [m for m in range(len(a)) if not flat[m]]
    if beta > 0 and ramps and case[:4] not in NO_CAP:
        ratio = max(np.abs(a[m]).max() / (S64[m].max() - S64[m].min()) for m in ramps)
        share = guard[ramps].mean()
        print("case %r beta %.1f: max|a| / (hi - lo) <= %.2f, guard band %.3f %%" % (case, beta, ratio, 100 * share))
        assert ratio < 4 and share <= 0.02
    got = _overlay(dev, case, beta)
    assert got.dtype == torch.uint8 and tuple(got.shape) == v64.shape and got.is_contiguous()
    got = got.cpu().numpy().astype(np.int64)
    want = np.floor(v64 + 0.5).astype(np.int64)
    for m in range(len(a)):
        photo = photos[idx[m]].transpose(1, 2, 0)
        if beta == 0:
            assert np.array_equal(got[m], photo)                                       # the photograph itself
        elif flat[m]:
            assert np.array_equal(got[m], np.floor((1.0 - b) * photo + 0.5))           # round((1 - beta) img), exactly
        else:
            assert np.array_equal(got[m][~guard[m]], want[m][~guard[m]])
            assert np.abs(got[m] - want[m]).max() <= 1


@pytest.mark.parametrize("case", OR.MAP_CASES)
def test_overlay_is_the_documented_fp32_formula(dev, case):
    """byte for byte: the fp32 formula of include/scnattn.h on the maps and ranges `pyramid_expand` returns -- which also
    shows that the overlay launch recomputes S with the same bits"""
    from scnattn import viz
    h, w, upscale, sigma, _ = case
    a, _, _, photos, idx = _maps_case(case)
    S, lohi = viz.pyramid_expand(torch.from_numpy(a).to(dev), upscale, sigma, return_range=True)
    S, lohi = S.cpu().numpy(), lohi.cpu().numpy()
    f = np.float32
    for beta in BETAS:
        got = _overlay(dev, case, beta)
        again = viz.overlay_maps(torch.from_numpy(photos).to(dev), torch.from_numpy(a).to(dev), idx,
                                 np.full(len(a), beta, np.float32), upscale, sigma, recompute=True)
        assert torch.equal(got, again)                 # the maps recomputed instead of read back: the same bytes
        got = got.cpu().numpy()
        b = f(beta)
        keep, b255 = f(1) - b, b * f(255)
        for m in range(len(a)):
            lo, hi = lohi[m]
            nrm = np.clip((S[m] - lo) / (hi - lo), f(0), f(1)) if hi > lo else np.zeros_like(S[m])
            v = keep * photos[idx[m]].transpose(1, 2, 0).astype(f) + (b255 * nrm)[:, :, None]
            assert v.dtype == f
            assert np.array_equal(got[m], np.clip((v + f(0.5)).astype(np.int32), 0, 255))


# ---- public path ---------------------------------------------------------------------------------------------------
def test_attention_overlays_equal_the_per_piece_calls(dev):
    from scnattn import viz
    imgs = [RR.random_image((33, 47), 31), RR.random_image((64, 40), 32, grey=True)]
    maps = OR.maps(14, 14, 2, seed=3)
    alphas = [np.ones((1, 14, 14), np.float32), torch.from_numpy(maps[:3]).to(dev)]
    got = viz.attention_overlays(imgs, alphas)
    assert [tuple(g.shape) for g in got] == [(1, 336, 336, 3), (3, 336, 336, 3)] and all(g.dtype == torch.uint8 for g in got)
    photos = SD.resize_u8(imgs, (336, 336), device=dev, filter="lanczos")
    assert torch.equal(got[0][0], photos[0].permute(1, 2, 0))                      # map 0: the photograph (beta 0)
    assert torch.equal(got[1][0], photos[1].permute(1, 2, 0))
    piece = viz.overlay_maps(photos[1:], torch.from_numpy(maps[1:3]).to(dev), [0, 0], [0.8, 0.8])
    assert torch.equal(got[1][1:], piece)
    zoom = viz.attention_overlays(imgs, alphas, smooth=False)
    assert torch.equal(zoom[1][1:], viz.overlay_maps(photos[1:], torch.from_numpy(maps[1:3]).to(dev), [0, 0], [0.8, 0.8],
                                                     sigma=None))
    assert not torch.equal(zoom[1][1], got[1][1])


@pytest.mark.parametrize("kind", ["attention_scn", "pure_attention", "pure_scn"])
def test_captioner_overlays(dev, kind):
    import test_gpu_captioner as TC
    from scnattn import viz
    from scnattn.inference import Captioner
    wm = BR.word_map(TC.V)
    enc, tag, dec = TC._modules(kind, dev)
    images = TC._images()
    cap = Captioner(enc, dec, wm, tagger=tag, beam_size=3)
    plain = cap(images)
    assert all(set(r) == {"tokens", "words", "alphas", "tags"} for r in plain)
    records = cap(images, overlays=True)
    assert [r["tokens"] for r in records] == [r["tokens"] for r in plain]
    if kind == "pure_scn":
        assert all(r["overlays"] is None and r["alphas"] is None for r in records)
        return
    hh = len(records[0]["alphas"][0])
    want = viz.attention_overlays(images, [r["alphas"] for r in records], size=(336, 336), upscale=336 // hh)
    for rec, w in zip(records, want):
        assert rec["overlays"].dtype == torch.uint8 and rec["overlays"].is_cuda
        assert tuple(rec["overlays"].shape) == (len(rec["alphas"]), 336, 336, 3)
        assert torch.equal(rec["overlays"], w)


# ---- refusals: decided on the host, before any launch (the pointers handed over are host memory) ---------------------
def _taps_call(h, table, n_in=5, OW=8, dst=True):
    from scnattn import _lib as L
    src, lut, out = (C.c_uint8 * 4096)(), (C.c_float * 768)(), (C.c_uint8 * 4096)()
    taps = (C.c_int32 * len(table))(*[int(v) for v in table])
    desc = (L.ImageDesc * 1)(L.ImageDesc(0, 8, n_in, 3, 0, -1, 0))          # 8 x 5 -> 8 x 8: a horizontal pass only
    return h.scnattn_u8_resize_taps(None, src, 4096, desc, desc, 1, taps, taps, len(table), 8, OW, lut,
                                    out if dst else None, 0, 0)


def test_refusals_before_any_launch():
    from scnattn import _lib as L
    h = L.lib()
    xmin, n, coeff = SD.resize_taps(5, 8, filter="lanczos")
    good = np.concatenate([[coeff.shape[1]], xmin, n, coeff.ravel()]).astype(np.int64)

    def bad(pos, value):
        t = good.copy()
        t[pos] = value
        return t

    first_coeff = 1 + 16
    for table, kw, word in [
            (bad(1 + 8 + 3, coeff.shape[1] + 1), {}, b"tap count n"),                  # n > ksize
            (bad(1 + 8 + 3, 0), {}, b"tap count n"),
            (bad(first_coeff, 1 << 23), {}, b"24-bit"),                                # a coefficient >= 2^23
            (bad(first_coeff, -(1 << 23)), {}, b"24-bit"),
            (np.concatenate([good[:first_coeff], np.where(np.arange(coeff.size) % 7 < 3, (1 << 23) - 1, 0)]), {}, b"32 bits"),
            (bad(1, -1), {}, b"leave the source axis"),
            (bad(1 + 7, 4), {}, b"leave the source axis"),                             # xmin + n > in
            (bad(0, coeff.shape[1] + 1), {}, b"runs past the tap buffer"),             # a longer row than the buffer holds
            (bad(0, 0), {}, b"row length"),
            (good, {"dst": False}, b"null pointer")]:                                  # a null output
        assert _taps_call(h, table, **kw) == -1, word
        assert word in h.scnattn_last_error(), (word, h.scnattn_last_error())

    fl, i32 = (C.c_float * 4096)(), (C.c_int32 * 4)
    u8 = (C.c_uint8 * 4096)()

    def overlay(idx=(0, 1), out=u8, n_img=2, hw=(2, 2), size=(4, 4)):
        return h.scnattn_attn_overlay(None, fl, 2, hw[0], hw[1], fl, fl, size[0], size[1], None, fl, u8, n_img, i32(*idx),
                                      i32(*idx), fl, out)

    for kw, word in [({"idx": (0, 2)}, b"img_index"), ({"idx": (-1, 0)}, b"img_index"), ({"out": None}, b"null pointer"),
                     ({"hw": (0, 2)}, b"map size"), ({"hw": (2, L.OVERLAY_MAX_MAP + 1)}, b"map size"),
                     ({"size": (4, L.OVERLAY_MAX_OUT + 1)}, b"output size"), ({"hw": (2, 32), "size": (4, 1024)}, b"LDS"),
                     ({"n_img": 0}, b"photograph")]:
        assert overlay(**kw) == -1, word
        assert word in h.scnattn_last_error(), (word, h.scnattn_last_error())
    assert h.scnattn_attn_expand(None, fl, 2, 2, 2, fl, fl, 4, 4, fl, fl, None) == -1 and b"null pointer" in h.scnattn_last_error()
    assert h.scnattn_attn_strips(0) == -1 and h.scnattn_attn_strips(336) == 21



def test_public_refusals(dev):
    from scnattn import viz
    imgs = [RR.random_image((7, 5), 1)]
    with pytest.raises(ValueError, match="times the"):                                  # 336 is not 23 x 14
        viz.attention_overlays(imgs, [np.ones((2, 14, 14), np.float32)], upscale=23)
    with pytest.raises(ValueError, match="times the"):
        viz.attention_overlays(imgs, [np.ones((2, 14, 14), np.float32)], size=(336, 312))
    photos = torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="img_index"):
        viz.overlay_maps(photos, torch.ones((2, 2, 2), device="cuda"), [0, 1], [0.8, 0.8], upscale=2, sigma=None)
