"""CPU tests of tests/tagloss_refs.py and of the host side of the tagger loss family (scnattn_tagloss_fwd / _bwd,
scnattn.functional.TagLoss).

1. The references: the hand-written derivative equals fp64 autograd of the forward reference; (w, 0, 0, 0) equals
   binary_cross_entropy_with_logits(pos_weight = w) in fp64; the identity setting equals the BCE reference of taghead_refs
   away from its -100 clamp.
2. The judges accept torch's CPU fp32 evaluation of the kernel's expressions on every case of the GPU test, and the guard band
   of the margin leaves out nothing on the (3, 1001) case (m = 0.05 and m = 0.2).
3. Each planted defect fails its judge: 1 - p by subtraction at z = 30, the weight on the negative part, the two gammas
   swapped, the margin applied to the positives, the gradient without its [p > m] mask.
4. Host logic: TagLoss refuses what the library refuses and cannot be changed; balanced / prior_bias on a hand-counted
   matrix; the symbols are bound and declared and the version stays; the entry points refuse before launching; CPU tensors
   raise."""
import os

import pytest
import torch

import taghead_refs as T
import tagloss_refs as R
from kernel_harness import _STATS

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scnattn_tagloss_fwd", "scnattn_tagloss_bwd")
_IDS = [R.setting_id(s) for s in R.SETTINGS]


def _close(a, b, what, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), "%s: %.3e" % (what, err)


def _smooth_case(weights, m):
    """z in [-8, 8] with +-30 and +-120 added, kept 1e-3 away from the margin's kink in p (autograd has no derivative there)
    and off z = 0, where autograd differentiates max(z, 0) and |z| by convention, not sp(z)"""
    g = torch.Generator().manual_seed(7)
    z = torch.rand(3, 41, generator=g, dtype=F64) * 16.0 - 8.0
    z[0, :6] = torch.tensor([30.0, -30.0, 120.0, -120.0, 1e-3, 20.0], dtype=F64)
    if m > 0:
        p = 1.0 / (1.0 + torch.exp(-z))
        z = torch.where((p - R.f32(m)).abs() < 1e-3, z + 0.5, z)
    t = (torch.rand(3, 41, generator=g) >= 0.5).to(F64)
    t = torch.where(torch.rand(3, 41, generator=g) < 0.2, torch.rand(3, 41, generator=g, dtype=F64), t)
    w = (torch.rand(41, generator=g, dtype=F64) * 20.0) if weights else None
    if weights:
        w[0], w[1] = 0.0, 99.0
    return z, t, w


# ---- 1. the references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", R.SETTINGS + ((0.0, 1.0, 0.2, True), (3.0, 16.0, 0.0, False)), ids=lambda s: R.setting_id(s))
def test_backward_reference_equals_fp64_autograd(setting):
    gp, gn, m, weights = setting
    z, t, w = _smooth_case(weights, m)
    zg = z.clone().requires_grad_(True)
    a, b = R.parts_ref(zg, t, w, gp, gn, m)
    loss = (a + b).sum() / z.numel()
    (0.37 * loss).backward()
    r = R.bwd_ref(z, t, w, gp, gn, m, 0.37)
    err = float((r["dz"] - zg.grad).abs().max())
    print("%s: autograd vs hand-written %.3e on gradients up to %.3e" % (R.setting_id(setting), err, float(zg.grad.abs().max())))
    _close(r["dz"], zg.grad, "dz")
    _close(R.fwd_ref(z, t, w, gp, gn, m)["loss"], loss.detach(), "loss")
    assert not bool(r["guard"].any())


def test_weighted_reference_equals_bce_with_logits_fp64():
    z, t, w = _smooth_case(True, 0.0)
    z[1, :2] = 0.0                                  # torch's own backward is analytic: z = 0 is checked here
    zg = z.clone().requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(zg, t, pos_weight=w)
    loss.backward()
    _close(R.fwd_ref(z, t, w, 0.0, 0.0, 0.0)["loss"], loss.detach(), "loss")
    _close(R.bwd_ref(z, t, w, 0.0, 0.0, 0.0, 1.0)["dz"], zg.grad, "dz")


def test_identity_equals_the_bce_reference_away_from_its_clamp():
    g = torch.Generator().manual_seed(8)
    z = torch.rand(3, 37, generator=g, dtype=F64) * 16.0 - 8.0
    t = torch.rand(3, 37, generator=g, dtype=F64)
    p = T.sigmoid_ref(z)
    want = T.bce_fwd_ref(p, t)
    got = R.fwd_ref(z, t, None, 0.0, 0.0, 0.0)
    _close(got["loss"], want["loss"], "loss", 1e-11)          # log1p(-p) of the BCE reference forms 1 - p: 3e-13 at z = 8
    _close(got["rows"], want["rows"], "rows", 1e-11)
    _close(R.bwd_ref(z, t, None, 0.0, 0.0, 0.0, 0.37)["dz"], T.bce_bwd_ref(p, t, 0.37), "dz", 1e-11)
    # ... and where BCELoss clamps, the logits form keeps the term and the gradient
    zs, ts = torch.tensor([[-120.0, 120.0]], dtype=F64), torch.tensor([[1.0, 0.0]], dtype=F64)
    assert R.fwd_ref(zs, ts, None, 0.0, 0.0, 0.0)["terms"].tolist() == [[120.0, 120.0]]
    assert R.bwd_ref(zs, ts, None, 0.0, 0.0, 0.0, 2.0)["dz"].tolist() == [[-1.0, 1.0]]
    assert T.bce_fwd_ref(T.sigmoid_ref(zs), ts)["terms"].tolist() == [[100.0, 100.0]]


# ---- 2. torch CPU fp32 passes every judge -----------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", R.SETTINGS, ids=_IDS)
def test_cpu_fp32_passes_every_judge(setting):
    gp, gn, m, weights = setting
    _STATS.clear()
    for B, S in R.SHAPES:
        z, t, w, planted = R.gen(B, S, weights)
        p, rows, loss, agree = R.cpu32_tagloss_fwd(z, t, w, gp, gn, m)
        R.judge_rows("cpu32 tagloss_fwd", rows, z, t, w, gp, gn, m, "%dx%d" % (B, S))
        R.judge_loss("cpu32 tagloss_fwd", loss, rows, B, S)
        T.judge_agree("cpu32 tagloss_fwd", agree, p, t)
        R.judge_dz("cpu32 tagloss_bwd", R.cpu32_tagloss_bwd(z, t, w, gp, gn, m, R.G), z, t, w, gp, gn, m, R.G, planted,
                   "%dx%d" % (B, S))
        if planted:
            s = planted["sat0_t1"]
            ws = 1.0 if w is None else float(w[s])
            assert float(R.fwd_ref(z, t, w, gp, gn, m)["terms"][0, s]) == ws * 120.0        # nothing is clamped at -100
    for (kern, name), (ratio, _, _, n) in sorted(_STATS.items()):
        assert ratio <= 1.0, (kern, name, ratio)
    _STATS.clear()
    R.MEASURED.clear()


@pytest.mark.parametrize("m", (0.05, 0.2))
def test_guard_band_leaves_out_nothing_on_3x1001(m):
    z, t, _, _ = R.gen(3, 1001, False)
    assert int(R.bwd_ref(z, t, None, 0.0, 4.0, m, 1.0)["guard"].sum()) == 0


def test_guard_band_is_bounded():
    """a case with more than 1 % of its elements at the margin is refused by the judge, not silently left unjudged"""
    z = torch.full((2, 50), float(torch.log(torch.tensor(0.05 / 0.95, dtype=F64))))
    t = torch.zeros(2, 50)
    with pytest.raises(AssertionError, match="guard band"):
        R.judge_dz("defect", torch.zeros(2, 50), z, t, None, 0.0, 0.0, 0.05, 1.0)
    _STATS.clear()
    R.MEASURED.clear()


# ---- 3. planted defects -------------------------------------------------------------------------------------------------
def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn("defect", *a)
    _STATS.clear()
    R.MEASURED.clear()


def _rows32(terms64):
    return terms64.float().sum(dim=1)


@pytest.mark.parametrize("shape", ((3, 37), (32, 1000)), ids=("3x37", "32x1000"))
def test_planted_defects_fail(shape):
    B, S = shape
    k = R.G / (B * S)
    # 1 - p by subtraction: at z = 30 the fp32 p is 1 and the positive's gradient is lost
    z, t, w, planted = R.gen(B, S, True)
    good = R.cpu32_tagloss_bwd(z, t, w, 0.0, 0.0, 0.0, R.G)
    R.judge_dz("ok", good, z, t, w, 0.0, 0.0, 0.0, R.G, planted)
    p32 = torch.sigmoid(z)
    sub = (torch.tensor(R.G) / float(B * S)) * (t * w * -(1.0 - p32) + (1.0 - t) * p32)
    assert float(sub[0, planted["big_t1"]]) == 0.0 and float(good[0, planted["big_t1"]]) != 0.0
    _fails(R.judge_dz, sub, z, t, w, 0.0, 0.0, 0.0, R.G, planted)
    only = good.clone()
    only[0, planted["big_t1"]] = 0.0
    _fails(R.judge_dz, only, z, t, w, 0.0, 0.0, 0.0, R.G, planted)                        # ... at that element alone
    # the weight applied to the negative part
    a, b = R.parts_ref(z, t, None, 0.0, 0.0, 0.0)
    _fails(R.judge_rows, _rows32(a + b * w.to(F64)), z, t, w, 0.0, 0.0, 0.0)
    da, db, _ = R.grad_parts_ref(z, t, None, 0.0, 0.0, 0.0)
    _fails(R.judge_dz, (k * (da + db * w.to(F64))).float(), z, t, w, 0.0, 0.0, 0.0, R.G)
    # the two gammas swapped
    z, t, _, planted = R.gen(B, S, False)
    p, rows, _, _ = R.cpu32_tagloss_fwd(z, t, None, 1.5, 0.5, 0.0)
    _fails(R.judge_rows, rows, z, t, None, 0.5, 1.5, 0.0)
    _fails(R.judge_dz, R.cpu32_tagloss_bwd(z, t, None, 1.5, 0.5, 0.0, R.G), z, t, None, 0.5, 1.5, 0.0, R.G)
    # the margin applied to the positives as well: -log(max(p - m, tiny)) for -log p
    m = R.f32(0.05)
    p64 = T.sigmoid_ref(z)
    a, b = R.parts_ref(z, t, None, 0.0, 4.0, 0.05)
    bad_pos = t.to(F64) * -torch.log((p64 - m).clamp_min(1e-30))
    _fails(R.judge_rows, _rows32(bad_pos + b), z, t, None, 0.0, 4.0, 0.05)
    da, db, _ = R.grad_parts_ref(z, t, None, 0.0, 4.0, 0.05)
    bad_dpos = torch.where(p64 > m, -t.to(F64) * p64 * (1.0 - p64) / (p64 - m).clamp_min(1e-30), torch.zeros_like(p64))
    _fails(R.judge_dz, (k * (bad_dpos + db)).float(), z, t, None, 0.0, 4.0, 0.05, R.G)
    # the gradient without its [p > m] mask: p q / (1 - 0) below the margin instead of 0
    da, db, _ = R.grad_parts_ref(z, t, None, 0.0, 0.0, 0.05)
    q64 = torch.exp(-R.sp(z.to(F64)))
    nomask = torch.where(p64 > m, db, (1.0 - t.to(F64)) * p64 * q64)
    assert bool(((p64 < m) & (t < 1)).any())
    _fails(R.judge_dz, (k * (da + nomask)).float(), z, t, None, 0.0, 0.0, 0.05, R.G)
    R.judge_dz("ok", R.cpu32_tagloss_bwd(z, t, None, 0.0, 0.0, 0.05, R.G), z, t, None, 0.0, 0.0, 0.05, R.G, planted)
    _STATS.clear()
    R.MEASURED.clear()


# ---- 4. host logic ----------------------------------------------------------------------------------------------------------
def test_tagloss_object():
    from scnattn.functional import TagLoss, prior_bias
    assert TagLoss().is_identity and TagLoss(None, 0, 0, 0).is_identity
    assert not TagLoss.asl().is_identity and not TagLoss.focal().is_identity and not TagLoss(torch.ones(3)).is_identity
    a = TagLoss.asl()
    assert (a.gamma_pos, a.gamma_neg, a.margin, a.pos_weight) == (0.0, 4.0, 0.05, None)
    f = TagLoss.focal(1.5, torch.tensor([1.0, 2.0]))
    assert (f.gamma_pos, f.gamma_neg, f.margin) == (1.5, 1.5, 0.0) and f.pos_weight.tolist() == [1.0, 2.0]
    with pytest.raises(AttributeError):
        a.margin = 0.1
    o = a.struct()
    assert (o.gamma_pos, o.gamma_neg) == (0.0, 4.0) and o.margin == R.f32(0.05)
    for bad in (dict(gamma_pos=-0.1), dict(gamma_neg=16.5), dict(gamma_pos=float("nan")), dict(gamma_neg=float("inf")),
                dict(margin=-0.01), dict(margin=1.0), dict(margin=float("nan")), dict(margin=0.05, gamma_neg=0.5),
                dict(pos_weight=torch.tensor([1.0, -1.0])), dict(pos_weight=torch.tensor([1.0, float("nan")])),
                dict(pos_weight=torch.ones(2, 2)), dict(pos_weight=torch.ones(3, dtype=F64)), dict(pos_weight=[1.0, 2.0])):
        with pytest.raises(ValueError):
            TagLoss(**bad)
    TagLoss(margin=0.05, gamma_neg=1.0), TagLoss(margin=0.05, gamma_neg=0.0), TagLoss(gamma_neg=0.5), TagLoss(gamma_pos=16.0)
    # 6 images, 4 tags with 0, 1, 3 and 6 positives (0.5 counts as positive, 0.49 does not)
    tg = torch.tensor([[0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0.5, 1], [0, 0, 0.49, 1], [0, 0, 0, 1], [0, 0, 0, 1]], dtype=torch.float32)
    b = TagLoss.balanced(tg)
    want = [min(max((6 / 1) ** 0.5, 1.0), 100.0), 5.0 ** 0.5, 1.0, 1.0]          # n = 0 counts as 1; (6-6)/6 -> clamped to 1
    assert b.pos_weight.dtype == torch.float32 and b.pos_weight.tolist() == pytest.approx(want, rel=1e-6)
    b2 = TagLoss.balanced(tg, power=1.0, cap=4.0, gamma_neg=2.0, gamma_pos=1.0)
    assert b2.pos_weight.tolist() == [4.0, 4.0, 1.0, 1.0] and (b2.gamma_pos, b2.gamma_neg, b2.margin) == (1.0, 2.0, 0.0)
    pb = prior_bias(tg)
    assert pb.dtype == torch.float32
    assert pb.tolist() == pytest.approx([float(torch.log(torch.tensor(v, dtype=F64))) for v in (1 / 7, 2 / 6, 4 / 4, 7 / 1)], rel=1e-6)
    assert prior_bias(tg, smooth=0.5).tolist()[1] == pytest.approx(float(torch.log(torch.tensor(1.5 / 5.5, dtype=F64))), rel=1e-6)


def test_symbols_are_bound_and_declared_and_the_version_stays():
    from scnattn import _lib as L
    h = L.lib()
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    for name in NAMES:
        assert name in L._SIGS and name in L.EXPORTS and hasattr(h, name)
        assert "int %s(void* stream" % name in header
    assert "} scnattn_tag_loss_options;" in header
    assert [f[0] for f in L.TagLossOpts._fields_] == ["gamma_pos", "gamma_neg", "margin"]
    assert h.scnattn_version() == 109 and "#define SCNATTN_VERSION 109" in header


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def test_entry_points_refuse_before_launching():
    import ctypes as C
    from scnattn import _lib as L
    h = L.lib()

    def opts(gp=0.0, gn=4.0, m=0.05):
        return C.byref(L.TagLossOpts(gp, gn, m))

    def fw(B=2, S=8, z=_P, ldz=8, t=_P, ldt=8, w=None, o=None, p=_P, ldp=8, rows=_P, out=_P, **kw):
        return h.scnattn_tagloss_fwd(None, B, S, z, ldz, t, ldt, w, opts(**kw) if o is None else o, p, ldp, rows, out)

    def bw(B=2, S=8, z=_P, ldz=8, t=_P, ldt=8, w=None, o=None, g=_P, dz=_P, lddz=8, **kw):
        return h.scnattn_tagloss_bwd(None, B, S, z, ldz, t, ldt, w, opts(**kw) if o is None else o, g, dz, lddz)

    def refused(rc, text):
        assert rc == -1
        assert text in h.scnattn_last_error(), h.scnattn_last_error()

    for f in (fw, bw):
        refused(f(gp=-1.0), b"[0, 16]")
        refused(f(gp=16.5), b"[0, 16]")
        refused(f(gn=float("nan")), b"[0, 16]")
        refused(f(gn=float("inf")), b"[0, 16]")
        refused(f(gp=float("nan")), b"[0, 16]")
        refused(f(m=1.0), b"[0, 1)")
        refused(f(m=-0.5), b"[0, 1)")
        refused(f(m=float("nan")), b"[0, 1)")
        refused(f(m=0.05, gn=0.5), b"unbounded")
        refused(f(o=C.POINTER(L.TagLossOpts)()), b"options are NULL")
        refused(f(B=0), b"bad shape")
        refused(f(S=0), b"bad shape")
        refused(f(z=None), b"null argument")
        refused(f(t=None), b"null argument")
        refused(f(ldz=7), b"leading dimension")
        refused(f(ldt=7), b"leading dimension")
        refused(f(B=4097, S=4096, ldz=4096, ldt=4096, ldp=4096) if f is fw else f(B=4097, S=4096, ldz=4096, ldt=4096, lddz=4096),
                b"2^24")
    refused(fw(p=None), b"null argument")
    refused(fw(rows=None), b"null argument")
    refused(fw(out=None), b"null argument")
    refused(fw(ldp=7), b"leading dimension")
    refused(bw(g=None), b"null argument")
    refused(bw(dz=None), b"null argument")
    refused(bw(lddz=7), b"leading dimension")


def test_cpu_tensors_raise():
    from scnattn import functional as SF
    from models.encoders.tagger import EncoderTagger
    from scnattn.resnet import resnet152_trunk
    from trains.harness import TaggerTrainStep, validate_tagger
    x4, W, b, t = torch.randn(2, 8, 2, 2), torch.randn(3, 8), torch.randn(3), torch.rand(2, 3)
    for loss in (SF.TagLoss.asl(), SF.TagLoss(torch.ones(3)), SF.TagLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SF.tag_head_loss(x4, None, W, b, t, loss=loss)
    with pytest.raises(TypeError):
        SF.tag_head_loss(x4, None, W, b, t, loss="focal")
    m = EncoderTagger(semantic_size=5)
    m.resnet = resnet152_trunk(depths=(1, 1, 1, 1), keep_avgpool=True)
    imgs, tags = torch.randn(2, 3, 64, 64), (torch.rand(40, 5) < 0.2).float()
    ts = TaggerTrainStep(device="cpu", encoder=m, semantic_size=5, loss=SF.TagLoss.asl(), prior_bias_from=tags)
    assert torch.equal(m.linear.bias.detach(), SF.prior_bias(tags)) and ts.loss.margin == 0.05
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.step(imgs, tags[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validate_tagger([(imgs, tags[:2])], m, loss=SF.TagLoss.focal())
    with pytest.raises(TypeError):
        TaggerTrainStep(device="cpu", encoder=m, semantic_size=5, loss="asl")
