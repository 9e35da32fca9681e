"""GPU tests of the image resize (csrc/resize.hip through scnattn.data.resize_u8 / resize_normalize) against the numpy
restatement of Pillow's 8-bit bilinear resize (tests/resize_refs.py) and the CPU restatement of the reference's
`/ 255.` + Normalize (oracle/data_ref.py).  Integer work plus a value table: every comparison is `torch.equal`."""
import numpy as np
import pytest
import torch

import resize_refs as RR
from oracle import data_ref as DR
from scnattn import data as SD

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _images(src, grey):
    return [RR.random_image(src, 11 + src[0] + 3 * src[1], grey), RR.checker_image(src, grey)]


def _case(src, dst, grey=False):
    """(images, uint8 rows [n, 3, OH, OW] of the restatement), computed once per process"""
    key = (src, dst, grey)
    if key not in _REF:
        imgs = _images(src, grey)
        _REF[key] = (imgs, np.stack([RR.rows(im, dst) for im in imgs]))
    return _REF[key]


def _normalized(rows, dtype):
    return torch.stack([DR.image_item(r) for r in rows]).to(dtype)


@pytest.mark.parametrize("grey", [False, True])
@pytest.mark.parametrize("src,dst", RR.SMALL_SHAPES)
def test_resize_u8_small_shapes(dev, src, dst, grey):
    imgs, want = _case(src, dst, grey)
    got = SD.resize_u8(imgs, dst, device=dev)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(imgs), 3) + dst and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("src,dst,grey", RR.WORKLOAD_SHAPES)
def test_resize_u8_workload_shapes(dev, src, dst, grey):
    imgs, want = _case(src, dst, grey)
    assert torch.equal(SD.resize_u8(imgs, dst, device=dev).cpu(), torch.from_numpy(want))


def _mixed():
    """the 7x5 RGB, the 3x1000 RGB, the 480x640 grey and the 375x500 RGB image, in that order"""
    parts = [_case((7, 5), (256, 256)), _case((3, 1000), (256, 256)), _case((480, 640), (256, 256), True),
             _case((375, 500), (256, 256))]
    return [p[0][0] for p in parts], np.stack([p[1][0] for p in parts])


def test_mixed_batch_one_launch(dev):
    imgs, want = _mixed()
    packed = SD.pack_images(imgs, (256, 256))
    assert [(d.H, d.W, d.C) for d in packed.desc] == [(7, 5, 3), (3, 1000, 3), (480, 640, 1), (375, 500, 3)]
    got = SD.resize_u8(packed, device=dev).cpu()
    assert torch.equal(got, torch.from_numpy(want))
    assert torch.equal(got[2, 0], got[2, 1]) and torch.equal(got[2, 0], got[2, 2])        # grey: one plane, three times


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_resize_normalize_256(dev, dtype, channels_last):
    imgs, rows = _mixed()
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    got = SD.resize_normalize(imgs, lut, (256, 256), dtype=dtype, channels_last=channels_last)
    assert got.dtype == dtype and tuple(got.shape) == (4, 3, 256, 256)
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert torch.equal(got.cpu(), _normalized(rows, dtype))


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_resize_normalize_16x7_leaves_the_vector_store_path(dev, dtype, channels_last):
    srcs = [((16, 16), False), ((33, 47), False), ((5, 9), True), ((7, 5), False)]
    imgs, rows = [], []
    for src, grey in srcs:
        i, r = _case(src, (16, 7), grey)
        imgs += i
        rows += list(r)
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    got = SD.resize_normalize(imgs, lut, (16, 7), dtype=dtype, channels_last=channels_last)
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert torch.equal(got.cpu(), _normalized(rows, dtype))
    u8 = SD.resize_u8(imgs, (16, 7), device=dev)
    assert torch.equal(u8.cpu(), torch.from_numpy(np.stack(rows)))


@pytest.mark.parametrize("size", [(256, 256), (16, 16), (16, 7), (24, 80)])
def test_resize_normalize_equals_its_two_halves(dev, size):
    imgs = [RR.random_image((33, 47), 1), RR.checker_image((16, 16)), RR.random_image((5, 9), 2, grey=True),
            RR.random_image((3, 1000), 3), RR.checker_image((257, 255))]
    for mean, std in ((DR.MEAN, DR.STD), (None, None)):
        lut = torch.from_numpy(SD.identity_lut(3) if mean is None else SD.normalize_lut(mean, std)).to(dev)
        u8 = SD.resize_u8(imgs, size, device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            for cl in (False, True):
                got = SD.resize_normalize(imgs, lut, size, dtype=dtype, channels_last=cl)
                want = SD.gather_normalize(u8, None, lut, dtype=dtype, channels_last=cl)
                assert got.stride() == want.stride() and torch.equal(got, want)


def test_batch_size_independence(dev):
    last = RR.random_image((33, 47), 5)
    others = [RR.random_image((7, 5), 6), RR.checker_image((257, 255)), RR.random_image((16, 16), 7, grey=True),
              RR.random_image((3, 1000), 8)]
    for size in ((16, 16), (256, 256)):
        alone = SD.resize_u8([last], size, device=dev)
        batch = SD.resize_u8(others + [last], size, device=dev)
        assert torch.equal(alone[0], batch[4])
        assert torch.equal(alone[0].cpu(), torch.from_numpy(RR.rows(last, size)))
