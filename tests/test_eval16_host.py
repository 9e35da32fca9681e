"""CPU-only tests of the bf16 eval-mode trunk path (scnattn/conv_eval16.py, include/scnattn.h scnattn_*_bn_eval16): the two
entry points are exported and refuse bad arguments with -1 and a message before anything touches the GPU, `eval16_reason`
names why a block stays on the module path, and `conv_eval.eval_reason` still answers "autocast" under autocast."""
import ctypes as C

import torch


def _h():
    from scnattn import _lib
    return _lib, _lib.lib()


# any non-null, 16-byte aligned address: the argument checks must reject the call before it is dereferenced
_P = 1 << 20


def _bn(L, **kw):
    d = dict(gamma=_P, beta=_P, mean=_P, var=_P, eps=1e-5, res=None, ldres=0, relu=1)
    d.update(kw)
    return L.BnEval16(**d)


def _refused(h, rc, text):
    assert rc == -1
    msg = h.scnattn_last_error()
    assert text in msg, msg


def test_bn_eval16_entry_points_are_exported():
    L, h = _h()
    for name in ("scnattn_conv1x1_fwd_bn_eval16", "scnattn_conv3x3_fwd_bn_eval16"):
        assert hasattr(h, name)
        assert name in L.EXPORTS
    assert h.scnattn_version() == 109       # new symbols only: they did not bump the version


def test_conv1x1_fwd_bn_eval16_argument_checks():
    L, h = _h()
    f = h.scnattn_conv1x1_fwd_bn_eval16
    bn = _bn(L)

    def call(R=64, Cin=64, Cout=64, x=_P, w=_P, y=_P, bn=bn, ex=None):
        return f(None, R, Cin, Cout, x, w, y, None if bn is None else C.byref(bn), None if ex is None else C.byref(ex), None, 0)

    _refused(h, call(bn=None), b"bn is NULL")
    for kw in (dict(epi=1), dict(epi=3), dict(pro=1)):
        _refused(h, call(ex=L.ConvExtra(**kw)), b"geometry only")
    for name in ("gamma", "beta", "mean", "var"):
        _refused(h, call(bn=_bn(L, **{name: None})), b"non-null and 16-byte aligned")
        _refused(h, call(bn=_bn(L, **{name: _P + 8})), b"non-null and 16-byte aligned")
    _refused(h, call(Cin=36), b"multiples of 8")
    _refused(h, call(Cout=68), b"multiples of 8")
    _refused(h, call(R=0), b"R > 0")
    _refused(h, call(bn=_bn(L, res=_P + 8, ldres=64)), b"residual must be")          # not 16-byte aligned
    _refused(h, call(bn=_bn(L, res=_P, ldres=68)), b"residual must be")              # ldres % 8
    _refused(h, call(bn=_bn(L, res=_P, ldres=56)), b"residual must be")              # ldres < Cout
    _refused(h, call(R=1 << 22, bn=_bn(L, res=_P, ldres=1 << 9)), b"residual must be")   # 4 GB: beyond the descriptor range
    _refused(h, call(ex=L.ConvExtra(stride=2)), b"gather geometry")
    # a null or misaligned operand is caught by the GEMM's own checks, still before any launch
    _refused(h, call(x=None), b"null operand")
    _refused(h, call(w=_P + 4), b"16-byte rows")
    _refused(h, call(ex=L.ConvExtra(force_split=2)), b"forced split does not fit")   # no workspace


def test_conv3x3_fwd_bn_eval16_argument_checks():
    L, h = _h()
    f = h.scnattn_conv3x3_fwd_bn_eval16
    bn = _bn(L)

    def call(N=2, Hi=8, Wi=8, Cin=64, Cout=64, s=1, bn=bn, ex=None):
        return f(None, N, Hi, Wi, Cin, Cout, s, _P, _P, _P, None if bn is None else C.byref(bn),
                 None if ex is None else C.byref(ex), None, 0)

    _refused(h, call(bn=None), b"bn is NULL")
    _refused(h, call(ex=L.ConvExtra(epi=2)), b"geometry only")
    _refused(h, call(Cin=48), b"multiple of 32")
    _refused(h, call(Cout=68), b"multiple of 32, Cout of 8")
    _refused(h, call(s=3), b"geometry")
    _refused(h, call(N=0), b"geometry")
    _refused(h, call(bn=_bn(L, var=None)), b"non-null and 16-byte aligned")
    _refused(h, call(bn=_bn(L, res=_P, ldres=60)), b"residual must be")


def test_cgemm16_refuses_the_eval_epilogue_without_its_vectors():
    """scnattn_cgemm16 carries no running variance: epi = 3 through it is refused, not run with a null vector."""
    L, h = _h()
    ex = L.ConvExtra(epi=3, egamma=_P, ebeta=_P, emean=_P)
    rc = h.scnattn_cgemm16(None, 64, 64, 64, _P, 64, _P, 64, 0.0, _P, 64, 1, None, 0, C.byref(ex))
    _refused(h, rc, b"non-null and 16-byte aligned")
    rc = h.scnattn_cgemm16(None, 64, 64, 64, _P, 64, _P, 64, 0.0, _P, 64, 0, None, 0, C.byref(ex))      # fp32 output
    _refused(h, rc, b"needs a bf16 output")


def _block(inplanes=256, planes=64, stride=1):
    from torch import nn
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                             FusedBatchNorm2d(planes * 4))
    return Bottleneck(inplanes, planes, stride, down)


def test_eval16_reason_names_the_reason(monkeypatch):
    from scnattn import conv_eval16 as CE16
    from scnattn import conv as SC
    m = _block().eval()
    x = torch.randn(1, 256, 4, 4, dtype=torch.bfloat16)
    assert "GPU" in CE16.eval16_reason(m, x)
    m.train()
    assert "training" in CE16.eval16_reason(m, x)
    m.eval()
    monkeypatch.setattr(SC, "ENABLED", False)
    assert "disabled" in CE16.eval16_reason(m, x)
    monkeypatch.undo()
    # past the device check (no GPU here: stand in for it): an fp32 map, then the block's own terms
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert "bfloat16" in CE16.eval16_reason(m, x.float())
    assert "no bf16 weight copy" in CE16.eval16_reason(m, x)            # refresh_weights has not run
    for cv in (m.conv1, m.conv3):
        cv._w16 = None
    with torch.no_grad():
        assert CE16.eval16_reason(m, x) is None                          # conv2 without a copy is served (transient copy)
    assert "gradient" in CE16.eval16_reason(m, x)                        # grad enabled, parameters require it
    for p in m.parameters():
        p.requires_grad_(False)
    assert CE16.eval16_reason(m, x) is None
    assert "gradient" in CE16.eval16_reason(m, x.clone().requires_grad_(True))
    m.bn2.running_var = m.bn2.running_var.double()
    assert "not fp32" in CE16.eval16_reason(m, x)
    m.bn2.running_var = m.bn2.running_var.float()
    m48 = _block(192, 48).eval()
    for cv in (m48.conv1, m48.conv3):
        cv._w16 = None
    with torch.no_grad():
        assert "multiple of 32" in CE16.eval16_reason(m48, torch.randn(1, 192, 4, 4, dtype=torch.bfloat16))


def test_eval_reason_under_autocast_is_unchanged(monkeypatch):
    """An fp32 map under autocast keeps today's answer from conv_eval.eval_reason, and the bf16 block does not take it."""
    from scnattn import conv_eval as CE
    from scnattn import conv_eval16 as CE16
    m = _block().eval()
    x = torch.randn(1, 256, 4, 4)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert "autocast" in CE.eval_reason(m, x)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert "autocast" in CE.eval_reason(m, x)
    assert "bfloat16" in CE16.eval16_reason(m, x)
    monkeypatch.undo()
    with torch.no_grad():       # the module path still serves CPU tensors, unchanged
        assert torch.equal(m(x), m.module_forward(x))
