"""CPU-only tests of the eval-mode trunk path (scnattn/conv_eval.py, include/scnattn.h scnattn_*_bn_eval): the two
entry points are exported and reject bad arguments with -1 and a message before anything touches the GPU, and
`eval_reason` names why a block stays on the module path."""
import ctypes as C

import pytest
import torch


def _h():
    from scnattn import _lib
    return _lib, _lib.lib()


# any non-null, 16-byte aligned address: the argument checks must reject the call before it is dereferenced
_P = 1 << 20


def _bn(L, **kw):
    d = dict(gamma=_P, beta=_P, mean=_P, var=_P, eps=1e-5, res=None, ldres=0, relu=1)
    d.update(kw)
    return L.BnEval(**d)


def test_bn_eval_entry_points_are_exported():
    L, h = _h()
    for name in ("scnattn_conv1x1_fwd_bn_eval", "scnattn_conv3x3_fwd_bn_eval"):
        assert hasattr(h, name)
        assert name in L.EXPORTS


def test_conv1x1_fwd_bn_eval_argument_checks():
    L, h = _h()
    f = h.scnattn_conv1x1_fwd_bn_eval
    bn = _bn(L)
    assert f(None, 64, 64, 64, _P, _P, _P, None, None, None, 0) == -1
    assert b"bn is NULL" in h.scnattn_last_error()
    assert f(None, 64, 64, 64, _P, _P, _P, C.byref(_bn(L, var=None)), None, None, 0) == -1
    assert b"null BatchNorm" in h.scnattn_last_error()
    for kw in (dict(epi=1), dict(epi=3), dict(pro=1)):
        ex = L.ConvExtra(**kw)
        assert f(None, 64, 64, 64, _P, _P, _P, C.byref(bn), C.byref(ex), None, 0) == -1
        assert b"geometry only" in h.scnattn_last_error()
    assert f(None, 64, 40, 64, _P, _P, _P, C.byref(bn), None, None, 0) == -1
    assert b"multiples of 16" in h.scnattn_last_error()
    assert f(None, 64, 64, 72, _P, _P, _P, C.byref(bn), None, None, 0) == -1
    assert b"multiples of 16" in h.scnattn_last_error()
    assert f(None, 64, 64, 64, _P, _P, _P, C.byref(_bn(L, res=_P + 4, ldres=64)), None, None, 0) == -1
    assert b"res must be" in h.scnattn_last_error()
    assert f(None, 64, 64, 64, _P, _P, _P, C.byref(_bn(L, res=_P, ldres=66)), None, None, 0) == -1
    assert b"res must be" in h.scnattn_last_error()
    assert f(None, 64, 64, 64, _P, _P, _P, C.byref(_bn(L, mean=_P + 8)), None, None, 0) == -1
    assert b"aligned" in h.scnattn_last_error()
    # a null operand is caught by the GEMM's own checks, still before any launch
    assert f(None, 64, 64, 64, None, _P, _P, C.byref(bn), None, None, 0) == -1
    assert b"null operand" in h.scnattn_last_error()


def test_conv3x3_fwd_bn_eval_argument_checks():
    L, h = _h()
    f = h.scnattn_conv3x3_fwd_bn_eval
    bn = _bn(L)
    assert f(None, 2, 8, 8, 64, 64, 1, _P, _P, _P, None, None, None, 0) == -1
    assert b"bn is NULL" in h.scnattn_last_error()
    ex = L.ConvExtra(epi=2)
    assert f(None, 2, 8, 8, 64, 64, 1, _P, _P, _P, C.byref(bn), C.byref(ex), None, 0) == -1
    assert b"geometry only" in h.scnattn_last_error()
    assert f(None, 2, 8, 8, 24, 64, 1, _P, _P, _P, C.byref(bn), None, None, 0) == -1
    assert b"multiples of 16" in h.scnattn_last_error()
    assert f(None, 2, 8, 8, 64, 64, 3, _P, _P, _P, C.byref(bn), None, None, 0) == -1
    assert b"geometry" in h.scnattn_last_error()


def _block(inplanes=256, planes=64, stride=1):
    from torch import nn
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                             FusedBatchNorm2d(planes * 4))
    return Bottleneck(inplanes, planes, stride, down)


def test_eval_reason_cpu_training_autocast(monkeypatch):
    from scnattn import conv_eval as CE
    from scnattn import conv as SC
    m = _block().eval()
    x = torch.randn(1, 256, 4, 4)
    assert "GPU" in CE.eval_reason(m, x)
    m.train()
    assert "training" in CE.eval_reason(m, x)
    m.eval()
    # CUDA autocast cannot be switched on without a GPU: stand in for it
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert "autocast" in CE.eval_reason(m, x)
    monkeypatch.undo()
    saved = SC.ENABLED
    SC.ENABLED = False
    try:
        assert "disabled" in CE.eval_reason(m, x)
    finally:
        SC.ENABLED = saved
    # the module path still serves CPU eval tensors (structure tests), unchanged
    with torch.no_grad():
        y = m(x)
        assert torch.equal(y, m.module_forward(x))
    assert y.shape == (1, 256, 4, 4)
