"""CPU tests of tests/taghead_refs.py and of the tagger head's host side.

1. The index-arithmetic fp64 references equal torch's own fp64 ops (adaptive_avg_pool2d, linear, sigmoid,
   binary_cross_entropy -- the functions the reference calls) and their autograd to 1e-12.
2. The judges exclude nothing a correct fp32 evaluation produces: torch's CPU fp32 evaluation of the same formulas passes
   every judge on every case of the GPU test (worst err / bound over all cases: pooled 0.089, dx 0.189 fp32 / 0.986 bf16,
   rows 0.026, loss 0.097, dz 0.327, probs 0.25 by construction -- printed by the test).
3. Each planted defect fails its judge.
4. Host logic: CPU tensors raise RuntimeError (no fallback), the four symbols are in the ctypes table and in the header, the
   library's version stays what it was (109), and the entry points refuse bad arguments with -1 before anything is launched."""
import os

import pytest
import torch

import taghead_refs as R
from kernel_harness import _STATS

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scnattn_tag_pool_fwd", "scnattn_tag_pool_bwd", "scnattn_bce_fwd", "scnattn_bce_bwd")


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), "%s: %.3e" % (what, err)


# ---- 1. references vs torch fp64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ks", (False, True))
def test_head_reference_equals_torch_fp64(with_ks):
    B, H, Wd, C, S = 3, 2, 3, 20, 37
    g = torch.Generator().manual_seed(5)
    x4 = torch.randn(B, C, H, Wd, generator=g, dtype=F64, requires_grad=True)
    W = (torch.randn(S, C, generator=g, dtype=F64) * 0.7).requires_grad_(True)
    b = torch.randn(S, generator=g, dtype=F64).requires_grad_(True)
    t = torch.rand(B, S, generator=g, dtype=F64)
    ks = ((torch.rand(B, C, generator=g) >= 0.15).double() / 0.85) if with_ks else None
    xd = torch.nn.functional.adaptive_avg_pool2d(x4, 1).flatten(1)
    xd = xd if ks is None else xd * ks
    p = torch.sigmoid(torch.nn.functional.linear(xd, W, b))
    loss = torch.nn.functional.binary_cross_entropy(p, t)
    loss.backward()
    r = R.head_ref(x4.detach().permute(0, 2, 3, 1).reshape(B, H * Wd, C), ks, W.detach(), b.detach(), t)
    _close(r["probs"], p.detach(), "probs")
    _close(r["loss"], loss.detach(), "loss")
    _close(r["dW"], W.grad, "dW")
    _close(r["db"], b.grad, "db")
    _close(r["dx"], x4.grad.permute(0, 2, 3, 1).reshape(B, H * Wd, C), "dx")
    assert r["agree"] == int(((p >= 0.5) == (t >= 0.5)).sum())


def test_bce_reference_equals_torch_fp64_at_the_clamps():
    """saturated and tiny probabilities: torch's binary_cross_entropy and its backward, and the sigmoid's, in fp64"""
    p = torch.tensor([[0.0, 1.0, 0.0, 1.0, 9.3e-14, 0.5, 0.3, 1.0 - 2.0 ** -30]], dtype=F64, requires_grad=True)
    t = torch.tensor([[0.0, 1.0, 1.0, 0.0, 1.0, 0.49, 0.3, 0.0]], dtype=F64)
    loss = torch.nn.functional.binary_cross_entropy(p, t)
    loss.backward()
    f = R.bce_fwd_ref(p.detach(), t)
    _close(f["loss"], loss.detach(), "loss")
    assert f["terms"][0, :4].tolist() == [0.0, 0.0, 100.0, 100.0]
    dz = p.grad * (p.detach() * (1.0 - p.detach()))                 # times the sigmoid's derivative
    _close(R.bce_bwd_ref(p.detach(), t, 1.0), dz, "dz")
    assert R.bce_bwd_ref(p.detach(), t, 1.0)[0, :4].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_torch_cpu_fp32_sigmoid_saturates_as_the_cases_assume():
    z = torch.tensor([120.0, -120.0, 0.0, -30.0])
    p = torch.sigmoid(z)
    assert p[:3].tolist() == [1.0, 0.0, 0.5] and 0.0 < float(p[3]) < 1e-12
    assert float(p[3] * (1 - p[3])) < 1e-12


# ---- 2. torch CPU fp32 passes every judge -----------------------------------------------------------------------------------
def _pool_cases():
    return [(s, bf, k) for s in R.POOL_SHAPES for bf in (False, True) for k in (False, True)]


def test_cpu_fp32_passes_every_judge():
    _STATS.clear()
    for (B, HW, C), bf16, with_ks in _pool_cases():
        x, ks, dp = R.gen_pool(B, HW, C, bf16, with_ks)
        R.judge_pool_fwd("cpu32 pool_fwd", R.cpu32_pool_fwd(x, ks), x, ks)
        R.judge_pool_bwd("cpu32 pool_bwd%s" % ("16" if bf16 else ""), R.cpu32_pool_bwd(dp, ks, HW, bf16), dp, ks, HW, bf16)
        if bf16:
            R.judge_pool_fwd("cpu32 pool_fwd r16", R.cpu32_pool_fwd(x, ks, True), x, ks, True)
            if HW > 1 and C > 4:      # ... and the fp32 bound does not let a rounded mean through, nor the rounded bound a truncated one
                with pytest.raises(AssertionError):
                    R.judge_pool_fwd("defect", R.cpu32_pool_fwd(x, ks, True), x, ks)
                y = R.cpu32_pool_fwd(x, None)
                with pytest.raises(AssertionError):
                    R.judge_pool_fwd("defect", (y.view(torch.int32) & -65536).view(torch.float32) * (1.0 if ks is None else ks), x, ks, True)
    for B, S in R.BCE_SHAPES:
        z, t, planted = R.gen_bce(B, S)
        p, rows, loss, agree = R.cpu32_bce_fwd(z, t)
        R.judge_probs("cpu32 bce_fwd", p, z, planted)
        R.judge_rows("cpu32 bce_fwd", rows, p, t)
        R.judge_loss("cpu32 bce_fwd", loss, rows, B, S)
        R.judge_agree("cpu32 bce_fwd", agree, p, t)
        for g in (1.0, 0.37):
            R.judge_bce_bwd("cpu32 bce_bwd", R.cpu32_bce_bwd(p, t, g), p, t, g, planted)
    for (kern, name), (ratio, _, _, n) in sorted(_STATS.items()):
        print("%-16s %-7s worst err/bound %.3f over %d cases" % (kern, name, ratio, n))
        assert ratio <= 1.0
    _STATS.clear()


def test_bce_terms_of_cpu_fp32_stay_below_the_cap():
    """logits in [-8, 8]: the fp32 probabilities stay within 2.8e-5 of the row maximum of fp64, far inside the 1e-4 cap, so
    the cap is never the binding bar for a correct kernel"""
    for B, S in R.BCE_SHAPES:
        z, _, _ = R.gen_bce(B, S)
        want = R.sigmoid_ref(z)
        err = (torch.sigmoid(z).to(F64) - want).abs().max(dim=1)[0] / want.abs().max(dim=1)[0]
        assert float(err.max()) <= 2.8e-5
        assert 4.0 * R.sigmoid_yard(z) <= 1e-4 * float(want.abs().max(dim=1)[0].min())


# ---- 3. planted defects -------------------------------------------------------------------------------------------------
def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn("defect", *a)
    _STATS.clear()


def test_planted_defects_fail():
    B, S = 3, 37
    z, t, planted = R.gen_bce(B, S)
    p, rows, loss, agree = R.cpu32_bce_fwd(z, t)
    R.judge_loss("ok", loss, rows, B, S)
    _fails(R.judge_loss, rows.sum() / B, rows, B, S)                                     # mean over B instead of B * S
    lp, lq = torch.log(p), torch.log1p(-p)
    late = -((t * lp).clamp_min(-100.0) + ((1.0 - t) * lq).clamp_min(-100.0)).sum(dim=1)
    assert bool(late.isnan().any())
    _fails(R.judge_rows, late, p, t)                                                     # clamp after the multiplication: NaN
    none = -(torch.where(t > 0, t * lp, torch.zeros_like(p)) + torch.where(t < 1, (1.0 - t) * lq, torch.zeros_like(p))).sum(dim=1)
    assert bool(none.isinf().any())
    _fails(R.judge_rows, none, p, t)                                                     # no clamp at all: inf
    assert float(p[0, planted["half_eq"]]) == 0.5
    _fails(R.judge_agree, ((p > 0.5) == (t >= 0.5)).float().sum(), p, t)                 # > for >= on p
    _fails(R.judge_agree, ((p > 0.5) == (t > 0.5)).float().sum(), p, t)                  # > for >= on both
    _fails(R.judge_agree, ((p >= 0.5) == (t > 0.5)).float().sum(), p, t)                 # > for >= on t
    _fails(R.judge_agree, agree + 1.0, p, t)                                             # count off by one
    _fails(R.judge_agree, agree - 1.0, p, t)
    n = float(p.numel())
    R.judge_bce_bwd("ok", R.cpu32_bce_bwd(p, t, 1.0), p, t, 1.0, planted)
    _fails(R.judge_bce_bwd, (p - t) / n, p, t, 1.0, planted)                             # the logits form's gradient
    only_sat = R.cpu32_bce_bwd(p, t, 1.0).clone()
    s = planted["sat1_t0"]
    only_sat[0, s] = (p[0, s] - t[0, s]) / n
    _fails(R.judge_bce_bwd, only_sat, p, t, 1.0, planted)                                # ... at one saturated element only

    for (Bp, HW, C), bf16 in (((3, 4, 20), False), ((2, 49, 264), True)):
        x, ks, dp = R.gen_pool(Bp, HW, C, bf16, True)
        good = R.cpu32_pool_fwd(x, ks)
        R.judge_pool_fwd("ok", good, x, ks)
        _fails(R.judge_pool_fwd, R.cpu32_pool_fwd(x, (ks > 0).float()), x, ks)           # 0/1 mask without its scale
        _fails(R.judge_pool_fwd, good * HW, x, ks)                                       # 1/HW missing
        _fails(R.judge_pool_fwd, good - x[:, HW - 1, :] / HW * ks, x, ks)                # the last pixel row dropped
        _fails(R.judge_pool_fwd, good - x[:, 0, :] / HW * ks, x, ks)                     # the first
        gb = R.cpu32_pool_bwd(dp, ks, HW, bf16)
        R.judge_pool_bwd("ok", gb, dp, ks, HW, bf16)
        _fails(R.judge_pool_bwd, gb * HW, dp, ks, HW, bf16)                              # 1/HW missing in the backward
        _fails(R.judge_pool_bwd, R.cpu32_pool_bwd(dp, (ks > 0).float(), HW, bf16), dp, ks, HW, bf16)
        one = gb.clone()
        one[0, HW - 1, C - 1] = 0.0 if float(one[0, 0, C - 1]) != 0.0 else 1.0
        _fails(R.judge_pool_bwd, one, dp, ks, HW, bf16)                                  # one pixel differs
    x, ks, dp = R.gen_pool(2, 49, 264, True, True)
    exact = R.cpu32_pool_bwd(dp, ks, 49, False)
    trunc = (exact.view(torch.int32) & -65536).view(torch.float32)                       # bf16 by truncation
    _fails(R.judge_pool_bwd, trunc, dp, ks, 49, True)


# ---- 4. host logic ----------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_declared_and_the_version_stays():
    from scnattn import _lib as L
    h = L.lib()
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    for name in NAMES:
        assert name in L._SIGS and name in L.EXPORTS and hasattr(h, name)
        assert "int %s(void* stream" % name in header
    assert h.scnattn_version() == 109       # new symbols only: they did not bump the version
    assert "#define SCNATTN_VERSION 109" in header


def test_cpu_tensors_raise():
    from scnattn import functional as SF
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    from trains.harness import TaggerTrainStep, validate_tagger
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.tag_head_loss(torch.randn(2, 8, 2, 2), None, torch.randn(3, 8), torch.randn(3), torch.rand(2, 3))
    m = EncoderTagger(semantic_size=5)
    m.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    imgs, tags = torch.randn(2, 3, 64, 64), torch.rand(2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.tag_loss(imgs, tags)
    ts = TaggerTrainStep(device="cpu", encoder=m, semantic_size=5)
    assert ts.cfg["encoder_lr"] == 1e-4 and ts.cfg["grad_clip"] == 5.0 and ts.cfg["dropout"] == 0.15 and ts.cfg["batch_size"] == 32
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["linear.weight", "linear.bias"]   # fine_tune_encoder=False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.step(imgs, tags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validate_tagger([(imgs, tags)], m)
    with pytest.raises(TypeError):
        TaggerTrainStep(device="cpu", encoder=m, learning_rate=1.0)


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error(), h.scnattn_last_error()


def test_entry_points_refuse_before_launching():
    from scnattn import _lib as L
    h = L.lib()

    def pf(B=2, HW=4, C=8, x=_P, ks=None, ldk=8, out=_P, ldo=8, s=(32, 8, 1)):
        return h.scnattn_tag_pool_fwd(None, B, HW, C, x, 0, s[0], s[1], s[2], ks, ldk, out, ldo)

    def pb(B=2, HW=4, C=8, dp=_P, ldd=8, ks=None, ldk=8, dx=_P, s=(32, 8, 1)):
        return h.scnattn_tag_pool_bwd(None, B, HW, C, dp, ldd, ks, ldk, dx, 1, s[0], s[1], s[2])

    def bf(B=2, S=8, z=_P, ldz=8, t=_P, ldt=8, p=_P, ldp=8, rows=_P, out=_P):
        return h.scnattn_bce_fwd(None, B, S, z, ldz, t, ldt, p, ldp, rows, out)

    def bb(B=2, S=8, p=_P, ldp=8, t=_P, ldt=8, g=_P, dz=_P, lddz=8):
        return h.scnattn_bce_bwd(None, B, S, p, ldp, t, ldt, g, dz, lddz)

    _refused(h, pf(x=None), b"null map or output")
    _refused(h, pf(out=None), b"null map or output")
    _refused(h, pf(B=0), b"bad shape")
    _refused(h, pf(HW=0), b"bad shape")
    _refused(h, pf(ldo=7), b"leading dimension")
    _refused(h, pf(ks=_P, ldk=7), b"leading dimension")
    _refused(h, pf(s=(32, -8, 1)), b"negative stride")
    _refused(h, h.scnattn_tag_pool_fwd(None, 2, 4, 8, _P, 3, 32, 8, 1, None, 8, _P, 8), b"bf16 must be")
    _refused(h, pb(dx=None), b"null gradient or map")
    _refused(h, pb(dp=None), b"null gradient or map")
    _refused(h, pb(HW=0), b"bad shape")
    _refused(h, pb(ldd=7), b"leading dimension")
    _refused(h, pb(s=(32, 0, 1)), b"distinct")
    _refused(h, bf(B=0), b"bad shape")
    _refused(h, bf(p=None), b"null argument")
    _refused(h, bf(rows=None), b"null argument")
    _refused(h, bf(ldt=7), b"leading dimension")
    _refused(h, bf(B=4097, S=4096, ldz=4096, ldt=4096, ldp=4096), b"2^24")
    _refused(h, bb(dz=None), b"null argument")           # the gradient is asked for, its output is null
    _refused(h, bb(g=None), b"null argument")
    _refused(h, bb(lddz=7), b"leading dimension")
    _refused(h, bb(B=4097, S=4096, ldp=4096, ldt=4096, lddz=4096), b"2^24")
