"""CPU-only tests of the image resize's host side: the numpy restatement of Pillow's 8-bit bilinear resize
(tests/resize_refs.py) against recorded Pillow outputs and against Pillow itself where it is installed, the package's
coefficient tables against the restatement's, `pack_images`' refusals and layout, the header's declarations, and the C
entry point's refusals, which happen before anything touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resize_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scnattn_u8_resize_bilinear", "scnattn_resize_table_ints")
CASES = [(s, t, g) for s, t in RR.SMALL_SHAPES for g in (False, True)] + RR.WORKLOAD_SHAPES


def test_restatement_equals_recorded_pillow_outputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow.npz"))
    n = len([k for k in z.files if k.startswith("in_")])
    assert n >= 32 and str(z["pillow_version"]) == "12.2.0"
    shapes = set()
    for k in range(n):
        img, want = z["in_%02d" % k], z["out_%02d" % k]
        got = RR.resize(img, want.shape[:2])
        assert got.dtype == np.uint8 and np.array_equal(got, want), (k, img.shape, want.shape)
        shapes.add((img.shape[:2], want.shape[:2]))
    assert shapes == {(s, t) for s, t in RR.SMALL_SHAPES if s != (257, 255)}


@pytest.mark.parametrize("src,dst,grey", CASES)
def test_restatement_equals_pillow(src, dst, grey):
    Image = pytest.importorskip("PIL.Image")
    for img in (RR.random_image(src, 7, grey), RR.checker_image(src, grey)):
        want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), resample=2))
        assert np.array_equal(RR.resize(img, dst), want)


@pytest.mark.parametrize("pair", RR.AXIS_PAIRS + [(4000, 256), (256, 4000)])
def test_resize_taps_equals_restatement(pair):
    from scnattn import data as SD
    want, got = RR.taps(*pair), SD.resize_taps(*pair)
    for w, g in zip(want, got):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)
    assert SD.resize_taps(*pair)[2] is got[2]          # cached per (in, out)
    from scnattn import _lib as L
    assert L.lib().scnattn_resize_table_ints(*pair) == (0 if pair[0] == pair[1] else sum(g.size for g in got))


def test_resize_taps_refuses_bad_sizes():
    from scnattn import data as SD
    from scnattn import _lib as L
    for pair in [(0, 4), (4, 0), (L.RESIZE_MAX_DIM + 1, 4)]:
        with pytest.raises(ValueError):
            SD.resize_taps(*pair)
        assert L.lib().scnattn_resize_table_ints(*pair) == -1


def test_pack_images_rejects_float_four_channel_and_empty():
    from scnattn import data as SD
    ok = RR.random_image((5, 4), 0)
    for bad in ([ok.astype(np.float32)], [ok, np.zeros((5, 4, 4), np.uint8)], [], [np.zeros((0, 4, 3), np.uint8)],
                [ok, np.zeros((5,), np.uint8)], [ok.tolist()]):
        with pytest.raises(ValueError):
            SD.pack_images(bad, (8, 8))
    with pytest.raises(ValueError):
        SD.pack_images([ok], (0, 8))


def test_pack_images_layout():
    from scnattn import data as SD
    imgs = [RR.random_image((7, 5), 1), RR.random_image((16, 16), 2, grey=True), RR.random_image((7, 16), 3)]
    p = SD.pack_images(imgs, (16, 16))
    assert p.n == 3 and p.size == (16, 16) and p.buffer.dtype.is_floating_point is False
    raw = p.buffer.numpy()
    d0, d1, d2 = p.desc
    assert (d0.H, d0.W, d0.C) == (7, 5, 3) and (d1.H, d1.W, d1.C) == (16, 16, 1) and (d2.H, d2.W, d2.C) == (7, 16, 3)
    assert (d1.tab_h, d1.tab_v) == (-1, -1) and d2.tab_h == -1 and d2.tab_v == d0.tab_v     # one table per (in, out)
    for d, im in zip(p.desc, imgs):
        assert d.offset % 16 == 0
        assert np.array_equal(raw[p.src_off + d.offset:p.src_off + d.offset + im.size], im.reshape(-1))
    xmin, n, coeff = SD.resize_taps(5, 16)
    assert np.array_equal(p.taps[d0.tab_h:d0.tab_h + 32 + coeff.size], np.concatenate([xmin, n, coeff.ravel()]))
    assert p.taps_len == sum(a.size for a in SD.resize_taps(5, 16)) + sum(a.size for a in SD.resize_taps(7, 16))
    assert p.src_bytes == raw.size - p.src_off and p.src_off % 16 == 0


def test_resize_refuses_cpu_device():
    from scnattn import data as SD
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SD.resize_u8([RR.random_image((5, 4), 0)], (8, 8), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SD.resize_normalize([RR.random_image((5, 4), 0)], torch.from_numpy(SD.normalize_lut()), (8, 8))


def test_header_declares_every_new_export():
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    h = L.lib()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(h, name), name
    assert int(re.search(r"#define SCNATTN_RESIZE_MAX_DIM (\d+)", header).group(1)) == L.RESIZE_MAX_DIM
    assert "} scnattn_image_desc;" in header and C.sizeof(L.ImageDesc) == 32


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """Every refusal is decided on the host copy of the descriptors, before any HIP call: the pointers handed over here
    are host memory that a launch would fault on."""
    from scnattn import _lib as L
    h = L.lib()
    src = (C.c_uint8 * 4096)()
    taps = (C.c_int32 * 4096)()
    lut = (C.c_float * 768)()
    dst = (C.c_uint8 * 16)()
    n_h, n_v = h.scnattn_resize_table_ints(5, 8), h.scnattn_resize_table_ints(7, 8)
    assert n_h == 8 * 5 and n_v == 8 * 5

    def run(descs, OH=8, OW=8, src_bytes=4096, taps_len=4096, kind=0, cl=0, src_p=src, desc_p=True, dst_p=dst, n=None):
        arr = (L.ImageDesc * len(descs))(*descs)
        return h.scnattn_u8_resize_bilinear(None, src_p, src_bytes, arr if desc_p else None, arr, len(descs) if n is None else n,
                                            taps, taps_len, OH, OW, lut, dst_p, kind, cl)

    good = L.ImageDesc(0, 7, 5, 3, 0, n_h, 0)
    for descs, kw, word in [
            ([L.ImageDesc(4096 - 104, 7, 5, 3, 0, n_h, 0)], {}, b"past the packed buffer"),      # 105 bytes from 3992
            ([good, L.ImageDesc(-16, 7, 5, 3, 0, n_h, 0)], {}, b"past the packed buffer"),
            ([good], {"src_bytes": 104}, b"past the packed buffer"),
            ([L.ImageDesc(0, 7, 5, 2, 0, n_h, 0)], {}, b"1 or 3 channels"),
            ([L.ImageDesc(0, 7, 5, 4, 0, n_h, 0)], {}, b"1 or 3 channels"),
            ([L.ImageDesc(0, 0, 5, 3, 0, n_h, 0)], {}, b"image size"),
            ([L.ImageDesc(0, 7, 0, 3, 0, n_h, 0)], {}, b"image size"),
            ([L.ImageDesc(0, 7, L.RESIZE_MAX_DIM + 1, 1, 0, n_h, 0)], {"src_bytes": 1 << 20}, b"image size"),
            ([good], {"OH": 0}, b"target size"),
            ([good], {"OW": L.RESIZE_MAX_DIM + 1}, b"target size"),
            ([good], {"taps_len": n_h + n_v - 1}, b"vertical tap table"),
            ([L.ImageDesc(0, 7, 5, 3, -1, n_h, 0)], {}, b"horizontal tap table"),
            ([good], {"src_p": None}, b"null pointer"),
            ([good], {"desc_p": False}, b"null pointer"),
            ([good], {"dst_p": None}, b"null pointer"),
            ([good], {"kind": 3}, b"dst_kind"),
            ([good], {"kind": 0, "cl": 1}, b"planar"),
            ([good], {"n": -1}, b"images")]:
        assert run(descs, **kw) == -1, word
        assert word in h.scnattn_last_error(), (word, h.scnattn_last_error())
    assert run([], n=0) == 0                      # an empty batch launches nothing
