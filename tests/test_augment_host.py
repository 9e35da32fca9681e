"""Host logic of the augmentation (no GPU): `Augment`'s validation, the argument refusals of scnattn_u8_mean_grey,
scnattn_augment_draw and scnattn_u8_gather_augment (each decided before any HIP call, so the pointers handed over here are
host addresses a launch would fault on), the Python wrappers' refusals, and the C ABI's declarations."""
import ctypes as C
import os
import re

import pytest
import torch

from scnattn import _lib as L
from scnattn import augment as A
from scnattn import data as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced
SYMS = ("scnattn_u8_mean_grey", "scnattn_augment_draw", "scnattn_u8_gather_augment")


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error(), h.scnattn_last_error()


def test_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    h = L.lib()
    for sym in SYMS:
        assert "int %s(void* stream" % sym in header and sym in L.EXPORTS and getattr(h, sym) is not None
    assert "#define SCNATTN_VERSION 109 " in header and h.scnattn_version() == 109       # new symbols only
    assert "} scnattn_augment_config;" in header and C.sizeof(L.AugmentConfig) == 32
    fields = re.search(r"typedef struct scnattn_augment_config \{(.*?)\}", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in L.AugmentConfig._fields_]
    assert int(re.search(r"#define SCNATTN_AUGMENT_NPARAM (\d+)", header).group(1)) == L.AUGMENT_NPARAM == 8


@pytest.mark.parametrize("kw,text", [
    (dict(scale=(0.0, 1.0)), "scale needs 0 < low <= high <= 1"),
    (dict(scale=(0.8, 0.5)), "scale needs 0 < low <= high <= 1"),
    (dict(scale=(0.5, 1.5)), "scale needs 0 < low <= high <= 1"),
    (dict(scale=0.5), "scale must be a (low, high) pair"),
    (dict(ratio=(0.0, 1.0)), "ratio needs 0 < low <= high"),
    (dict(ratio=(2.0, 1.0)), "ratio needs 0 < low <= high"),
    (dict(ratio=(1.0, 2.0, 3.0)), "ratio must be a (low, high) pair"),
    (dict(flip=1.5), "flip is a probability in [0, 1]"),
    (dict(flip=-0.1), "flip is a probability in [0, 1]"),
    (dict(brightness=1.2), "brightness is a strength in [0, 1]"),
    (dict(contrast=-0.2), "contrast is a strength in [0, 1]"),
    (dict(saturation=float("nan")), "saturation is a strength in [0, 1]"),
])
def test_augment_validation_messages(kw, text):
    with pytest.raises(ValueError) as e:
        A.Augment(**kw)
    assert text in str(e.value)


def test_augment_defaults_identity_and_config():
    a = A.Augment()
    assert (a.scale, a.ratio, a.flip, a.brightness, a.contrast, a.saturation, a.seed) == \
        ((0.6, 1.0), (0.75, 4.0 / 3.0), 0.5, 0.2, 0.2, 0.2, 0)
    assert not a.is_identity
    ident = A.Augment(scale=(1, 1), ratio=(1, 1), flip=0, brightness=0, contrast=0, saturation=0, seed=9)
    assert ident.is_identity
    for kw in (dict(scale=(0.9, 1.0)), dict(ratio=(1.0, 1.1)), dict(flip=0.1), dict(brightness=0.1), dict(contrast=0.1),
               dict(saturation=0.1)):
        base = dict(scale=(1, 1), ratio=(1, 1), flip=0, brightness=0, contrast=0, saturation=0)
        base.update(kw)
        assert not A.Augment(**base).is_identity
    c = a.config()
    assert [getattr(c, n) for n, _ in L.AugmentConfig._fields_] == \
        [float(torch.tensor(v, dtype=torch.float32)) for v in (0.6, 1.0, 0.75, 4.0 / 3.0, 0.5, 0.2, 0.2, 0.2)]
    assert "Augment(scale=(0.6, 1.0)" in repr(a)


def test_wrappers_refuse_bad_tensors_before_any_call():
    src = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    params = torch.zeros(2, 8)
    for f in (lambda: A.mean_grey(src), lambda: A.gather_augment(src, None, params, None, None),
              lambda: A.Augment().draw(torch.zeros(2, dtype=torch.int64), 0, 4, 4)):
        with pytest.raises(RuntimeError) as e:
            f()
        assert "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("make,text", [
    (lambda: A.mean_grey(torch.zeros(2, 1, 4, 4, dtype=torch.uint8)), "C = 3"),
    (lambda: A.mean_grey(torch.zeros(2, 3, 4, 4)), "contiguous uint8"),
    (lambda: A.gather_augment(torch.zeros(2, 4, 4, 4, dtype=torch.uint8), None, torch.zeros(2, 8), None, None), "C = 3"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(2, 7), None, None), "float32 [n, 8]"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(2, 8, dtype=torch.float64), None, None),
     "float32 [n, 8]"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(16), None, None), "float32 [n, 8]"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(3, 8), None, None), "more parameter records"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 8), None,
                              None), "3 rows but 2 parameter records"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8), None,
                              None), "int64 vector"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(2, 8), None, None, grey=torch.zeros(3)),
     "grey must be float32 [N]"),
    (lambda: A.gather_augment(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), None, torch.zeros(2, 8), None, None, dtype=torch.float16),
     "dtype must be float32 or bfloat16"),
    (lambda: A.Augment().draw(torch.zeros(2, dtype=torch.int32), 0, 4, 4), "int64 vector"),
])
def test_wrappers_refuse_wrong_shapes_and_types(make, text):
    with pytest.raises(RuntimeError) as e:
        make()
    assert text in str(e.value)


def test_wrappers_refuse_bad_mean_std():
    src, params = torch.zeros(2, 3, 4, 4, dtype=torch.uint8), torch.zeros(2, 8)
    with pytest.raises(ValueError):
        A.gather_augment(src, None, params, (0.5, 0.5), (0.2, 0.2, 0.2))
    with pytest.raises(ValueError):
        A.gather_augment(src, None, params, (0.5, 0.5, 0.5), (0.2, 0.0, 0.2))


def test_device_loader_refuses_a_cpu_device_first():
    with pytest.raises(RuntimeError):
        SD.DeviceBatchLoader("/nonexistent", "x", "VAL", 4, "cpu", augment=A.Augment())


def test_mean_grey_argument_checks():
    h = L.lib()
    f = h.scnattn_u8_mean_grey
    _refused(h, f(None, None, 2, 16, None, _P), b"null pointer")
    _refused(h, f(None, _P, 2, 16, None, None), b"null pointer")
    _refused(h, f(None, _P, 2, 0, None, _P), b"bad shape")
    _refused(h, f(None, _P, -1, 16, None, _P), b"bad shape")
    _refused(h, f(None, _P, 2, (1 << 28) + 1, None, _P), b"bad shape")
    assert f(None, None, 0, 16, None, None) == 0            # nothing to do


def test_augment_draw_argument_checks():
    h = L.lib()
    f = h.scnattn_augment_draw

    def call(n=4, sid=_P, epoch=0, cfg=(0.6, 1.0, 0.75, 4.0 / 3.0, 0.5, 0.2, 0.2, 0.2), H=8, W=8, params=_P):
        return f(None, n, sid, epoch, 7, None if cfg is None else C.byref(L.AugmentConfig(*cfg)), H, W, params)

    _refused(h, call(sid=None), b"null pointer")
    _refused(h, call(params=None), b"null pointer")
    _refused(h, call(cfg=None), b"null pointer")
    _refused(h, call(n=-1), b"bad shape")
    _refused(h, call(H=0), b"bad shape")
    _refused(h, call(W=16385), b"bad shape")
    _refused(h, call(epoch=-1), b"bad shape")
    _refused(h, call(cfg=(0.0, 1.0, 0.75, 1.3, 0.5, 0.2, 0.2, 0.2)), b"scale_lo")
    _refused(h, call(cfg=(0.6, 1.1, 0.75, 1.3, 0.5, 0.2, 0.2, 0.2)), b"scale_lo")
    _refused(h, call(cfg=(0.6, 1.0, 1.5, 1.3, 0.5, 0.2, 0.2, 0.2)), b"ratio_lo")
    _refused(h, call(cfg=(0.6, 1.0, float("nan"), 1.3, 0.5, 0.2, 0.2, 0.2)), b"ratio_lo")
    _refused(h, call(cfg=(0.6, 1.0, 0.75, 1.3, 1.5, 0.2, 0.2, 0.2)), b"flip_p")
    _refused(h, call(cfg=(0.6, 1.0, 0.75, 1.3, 0.5, 0.2, 1.2, 0.2)), b"colour strengths")
    assert call(n=0, sid=None, params=None) == 0


def test_gather_augment_argument_checks():
    h = L.lib()
    f = h.scnattn_u8_gather_augment
    mean, std = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)

    def call(src=_P, N=4, idx=None, n=2, H=8, W=8, params=_P, grey=None, mean=mean, std=std, dst=_P, bf16=0, nhwc=0):
        return f(None, src, N, idx, n, H, W, params, grey, mean, std, dst, bf16, nhwc)

    _refused(h, call(src=None), b"null pointer")
    _refused(h, call(params=None), b"null pointer")
    _refused(h, call(dst=None), b"null pointer")
    _refused(h, call(mean=None), b"null pointer")
    _refused(h, call(std=None), b"null pointer")
    _refused(h, call(N=0), b"bad shape")
    _refused(h, call(n=-1), b"bad shape")
    _refused(h, call(H=0), b"bad shape")
    _refused(h, call(W=16385), b"bad shape")
    _refused(h, call(std=(C.c_float * 3)(0.2, 0.0, 0.2)), b"std must be non-zero")
    _refused(h, call(n=1 << 22, H=16384, W=16384), b"batch too large")
    assert call(n=0, params=None, dst=None) == 0
