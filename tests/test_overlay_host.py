"""CPU-only tests of the attention overlays' host side: the LANCZOS coefficient tables of `scnattn.data.resize_taps`
against the per-output loop of tests/overlay_refs.py, the numpy resize on those tables against recorded Pillow outputs
and against Pillow itself where it is installed, the bounds the C entry point validates, the unchanged bilinear default,
and `scnattn.viz.expand_operator` against the scipy composition that defines it."""
import os
import re

import numpy as np
import pytest

import overlay_refs as OR
import resize_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(i, o) for i in range(1, 41) for o in range(1, 41)] + OR.EXTRA_PAIRS
NEW = ("scnattn_u8_resize_taps", "scnattn_attn_strips", "scnattn_attn_expand", "scnattn_attn_overlay")


def _package_table(i, o):
    from scnattn import data as SD
    return SD.resize_taps(i, o, filter="lanczos")


def test_lanczos_taps_equal_the_loop_form_and_respect_the_validated_bounds():
    worst = 0
    for i, o in PAIRS:
        want, got = OR.taps(i, o), _package_table(i, o)
        for a, b in zip(want, got):
            assert b.dtype == np.int32 and b.shape == a.shape and np.array_equal(a, b), (i, o)
        xmin, n, coeff = got
        ksize = coeff.shape[1]
        assert ((1 <= n) & (n <= ksize)).all() and (xmin >= 0).all() and (xmin.astype(np.int64) + n <= i).all(), (i, o)
        mag = np.abs(coeff.astype(np.int64))
        assert mag.max() < (1 << 23), (i, o)
        assert (mag.sum(axis=1) * 255 + (1 << 21)).max() < (1 << 31), (i, o)
        assert not coeff[np.arange(ksize)[None, :] >= n[:, None]].any(), (i, o)       # nothing behind a row's n taps
        worst = max(worst, int(mag.sum(axis=1).max()))
    assert worst > (1 << 22)               # Lanczos has negative lobes: the sum of magnitudes exceeds the weight 1.0


def test_lanczos_taps_are_cached_and_refuse_bad_arguments():
    from scnattn import data as SD
    assert SD.resize_taps(33, 16, filter="lanczos")[2] is SD.resize_taps(33, 16, "lanczos")[2]
    assert (SD.resize_taps(33, 16, filter="lanczos")[2] < 0).any()
    with pytest.raises(ValueError):
        SD.resize_taps(33, 16, filter="bicubic")
    with pytest.raises(ValueError):
        SD.resize_taps(0, 16, filter="lanczos")
    with pytest.raises(ValueError):
        SD.pack_images([RR.random_image((5, 4), 0)], (8, 8), filter="nearest")


def test_bilinear_default_is_unchanged():
    from scnattn import data as SD
    for pair in RR.AXIS_PAIRS + [(4000, 256), (256, 4000)]:
        plain, named = SD.resize_taps(*pair), SD.resize_taps(*pair, filter="bilinear")
        for a, b, w in zip(plain, named, RR.taps(*pair)):
            assert a is b and np.array_equal(a, w)          # one cache entry; the table of the loop restatement
    imgs = [RR.random_image((7, 5), 1), RR.random_image((16, 16), 2, grey=True)]
    p, q = SD.pack_images(imgs, (16, 16)), SD.pack_images(imgs, (16, 16), filter="bilinear")
    assert p.filter == q.filter == "bilinear" and np.array_equal(p.taps, q.taps) and p.src_off == q.src_off
    assert bytes(p.desc) == bytes(q.desc)


def test_pack_images_lanczos_layout_carries_the_row_length():
    from scnattn import data as SD
    imgs = [RR.random_image((7, 5), 1), RR.random_image((16, 16), 2, grey=True), RR.random_image((33, 16), 3)]
    p = SD.pack_images(imgs, (16, 16), filter="lanczos")
    d0, d1, d2 = p.desc
    assert p.filter == "lanczos" and (d1.tab_h, d1.tab_v) == (-1, -1) and d2.tab_h == -1
    for off, pair in ((d0.tab_h, (5, 16)), (d0.tab_v, (7, 16)), (d2.tab_v, (33, 16))):
        xmin, n, coeff = SD.resize_taps(*pair, filter="lanczos")
        assert p.taps[off] == coeff.shape[1]
        body = p.taps[off + 1:off + 1 + 32 + coeff.size]
        assert np.array_equal(body, np.concatenate([xmin, n, coeff.ravel()]))
    assert SD.resize_taps(5, 16, filter="lanczos")[2].shape[1] == 7 and SD.resize_taps(33, 16, filter="lanczos")[2].shape[1] == 15
    assert p.taps_len == sum(1 + sum(a.size for a in SD.resize_taps(*pr, filter="lanczos")) for pr in ((5, 16), (7, 16), (33, 16)))


def test_numpy_resize_on_package_tables_equals_recorded_pillow_outputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lanczos_pillow.npz"))
    n = len([k for k in z.files if k.startswith("in_")])
    assert n == 4 * len(OR.GOLDEN_SHAPES) and str(z["pillow_version"]) == "12.2.0"
    shapes = set()
    for k in range(n):
        img, want = z["in_%02d" % k], z["out_%02d" % k]
        for table in (_package_table, OR.taps):
            got = OR.resize(img, want.shape[:2], table)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (k, img.shape, want.shape)
        shapes.add((img.shape[:2], want.shape[:2]))
    assert shapes == set(OR.GOLDEN_SHAPES)


@pytest.mark.parametrize("src,dst", OR.SMALL_SHAPES + [((375, 500), (336, 336)), ((100, 80), (336, 336))])
def test_numpy_resize_on_package_tables_equals_pillow(src, dst):
    Image = pytest.importorskip("PIL.Image")
    for grey in (False, True):
        for img in OR.images(src, grey):
            want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), resample=Image.LANCZOS))
            assert np.array_equal(OR.resize(img, dst, _package_table), want)


@pytest.mark.parametrize("n,upscale,sigma", OR.OPERATOR_CASES)
def test_expand_operator_equals_the_scipy_composition(n, upscale, sigma):
    from scnattn import viz
    M = viz.expand_operator(n, upscale, sigma)
    want = OR.operator(n, upscale, sigma)
    assert M.dtype == np.float64 and M.shape == want.shape == (n * upscale, n)
    assert np.abs(M - want).max() <= 1e-13
    assert np.abs(M.sum(axis=1) - 1.0).max() <= 1e-12
    assert (M >= 0).all()
    assert viz.expand_operator(n, upscale, sigma) is M and not M.flags.writeable        # cached per argument tuple


def test_expand_operator_applies_as_two_products():
    """the linear-operator argument: M_v . a . M_h^T is the composition applied to the map, h != w included"""
    from scnattn import viz
    rng = np.random.RandomState(0)
    for h, w, upscale, sigma in [(14, 14, 24, 8), (3, 5, 4, 1.5), (2, 2, 7, 30.0), (14, 14, 24, None)]:
        a = rng.rand(h, w)
        got = viz.expand_operator(h, upscale, sigma) @ a @ viz.expand_operator(w, upscale, sigma).T
        assert np.abs(got - OR.expand(a, upscale, sigma)).max() <= 1e-13
    assert (viz.expand_operator(14, 24, 8) != 0).sum(axis=1).max() <= 5


def test_package_does_not_import_scipy_and_header_declares_the_new_exports():
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = %r; import scnattn.viz, scnattn.inference; "
            "assert 'scipy' not in sys.modules and 'PIL' not in sys.modules" % [os.path.join(ROOT, "indonesian-image-captioning_amd")])
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(L.lib(), name), name
    assert int(re.search(r"#define SCNATTN_OVERLAY_MAX_MAP (\d+)", header).group(1)) == L.OVERLAY_MAX_MAP
    assert int(re.search(r"#define SCNATTN_OVERLAY_MAX_OUT (\d+)", header).group(1)) == L.OVERLAY_MAX_OUT
