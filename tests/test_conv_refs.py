"""The fp64 convolution references (tests/conv_refs.py), their judges and the case table of tests/test_gpu_conv_kernels.py,
without a GPU:
  * the references -- index tables written out by hand -- equal torch's fp64 conv2d / autograd (einsum for the 1x1 forms) to
    1e-12 at every row of the table;
  * the bounds are attainable: torch's own CPU fp32 convolution, with the prologue, the statistics, the mask and the eval
    epilogue formed in fp32, passes every judge at every row (the worst err / bound is printed; 0.21 for the GEMM families);
  * the judges are sensitive: a copy of the reference with one planted defect fails at least one row, for each defect of
    DEFECTS;
  * the library names the instance and the second launch each row reaches (test_gpu_conv_kernels.dispatch: the row's own
    call through scnattn_plan_next on host windows, rendered by conv_refs.name); every instance of REQUIRED appears."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
import test_gpu_conv_kernels as T  # noqa: F401 (the GPU module must import -- and collect -- without a GPU)

IDS = [R.case_id(c) for c in R.CASES]


# ==== torch's own convolution ============================================================================================
def _maps(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def torch_product(c, I, dt):
    """the product of a case by torch in dtype dt: conv2d / autograd for the 3x3 forms, einsum for the 1x1 forms"""
    x, dy, w = I["x"].to(dt), I["dy"].to(dt), I["w"].to(dt)
    if c.pro:
        x = torch.relu(x * I["ss"][:, 0].to(dt) + I["ss"][:, 1].to(dt))
    Ho, Wo = R.out_hw(c)
    if c.op in ("f1", "w1"):
        xs = x.reshape(c.N, c.Hi, c.Wi, c.Cin)[:, ::c.s, ::c.s].reshape(-1, c.Cin)
        return torch.einsum("rk,ok->ro", xs, w) if c.op == "f1" else torch.einsum("ro,rk->ok", dy, xs)
    if c.op == "d1":
        dx = torch.einsum("ro,ok->rk", dy, w)
        return dx + I["dx0"].to(dt) if "b" in c.var else dx
    w4 = w.reshape(c.Cout, 3, 3, c.Cin).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    x4 = _maps(x, c.N, c.Hi, c.Wi).contiguous().requires_grad_(True)
    y = F.conv2d(x4, w4, stride=c.s, padding=1)
    if c.op == "f3":
        return _rows(y.detach())
    y.backward(_maps(dy, c.N, Ho, Wo))
    if c.op in ("d3", "s3"):
        return _rows(x4.grad)
    return w4.grad.permute(0, 2, 3, 1).reshape(c.Cout, 9 * c.Cin)


def finish(c, I, prod, dt, on=None):
    """the epilogue of a case on a product `prod`, every step in dtype dt -> (out fp32, partials fp32 or None)"""
    prod = prod.to(dt)
    part = None
    if c.epi == 1:
        d = prod.float().to(dt) - (I["shift"].to(dt) if "s" in c.var else 0.0)          # of the STORED output
        part = torch.stack([R.block_sums(d), R.block_sums(d * d)])
    elif c.epi == 2:
        mask, xhat = R.mask_of(c, I)      # an fp32 fma the only way numpy can form it: exact in fp64, its sign taken
        on = mask if on is None else on
        prod = torch.where(on, prod, torch.zeros((), dtype=dt))
        g = prod.float().to(dt)
        part = torch.stack([R.block_sums(g), R.block_sums(g * xhat.to(dt))])
    elif c.epi == 3:
        scale = I["bn_gamma"].to(dt) / torch.sqrt(I["bn_var"].to(dt) + torch.tensor(R.BN_EPS, dtype=torch.float32).to(dt))
        prod = prod * scale + (I["bn_beta"].to(dt) - I["bn_mean"].to(dt) * scale)
        if "r" in c.var:
            prod = prod + I["res"].to(dt)
        if "l" in c.var:
            prod = torch.relu(prod)
    return prod.float(), (None if part is None else part.float())


class Worst:
    def __init__(self):
        self.ratio, self.where = 0.0, None

    def ok(self, kernel, name, got, want, bound, kind="sum"):
        want, bound = want.double(), bound.double().expand(want.shape)
        err = (got.double().reshape(want.shape) - want).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30).nan_to_num(1e30)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        if worst > self.ratio:
            self.ratio, self.where = worst, (kernel, name)
        assert bool((err <= bound).all()), "%s %s: worst err/bound %.3f" % (kernel, name, worst)


def _passes(c, I, out, part, tab=None):
    try:
        R.judge(c, I, out, part, R.case_id(c), Worst().ok, tab=tab)
        return True
    except AssertionError:
        return False


# ==== the references =====================================================================================================
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_reference_equals_torch_fp64(c):
    I = R.inputs(c)
    ref = R.reference(c, I)["out"]
    assert float((ref - torch_product(c, I, torch.float64)).abs().max()) <= 1e-12


def test_cpu_fp32_passes_every_judge():
    w, failed = Worst(), []
    for c in R.CASES:
        I = R.inputs(c)
        out, part = finish(c, I, torch_product(c, I, torch.float32), torch.float32)
        try:
            R.judge(c, I, out, part, R.case_id(c), w.ok)
        except AssertionError as e:
            failed.append(str(e))
    print("CPU fp32 evaluation of %d rows: worst err/bound %.3f at %s" % (len(R.CASES), w.ratio, w.where))
    assert not failed and w.ratio < 1.0, failed[:5]


def test_mask_inputs_hold_the_edges():
    """every epi = 2 row with >= 8 channels: an element where the expression is exactly 0 (masked), one on and one off beside it,
    and one where only the fused evaluation is positive"""
    f32 = np.float32
    for c in R.CASES:
        if c.epi != 2 or c.Cin < 8:
            continue
        I = R.inputs(c)
        on, xhat = R.mask_of(c, I)
        folded = "f" in c.var
        a, b = (I["ss"][:, 0], I["ss"][:, 1]) if folded else (I["gamma"], I["beta"])
        t = (I["z"] if folded else xhat).numpy().astype(np.float64)
        exact = t * a.numpy().astype(np.float64) + b.numpy().astype(np.float64)
        assert (exact[0, :4] == 0).all() and not on[0, :4].any(), R.case_id(c)
        if rows_ge(c, 3):
            assert (on[1, :4] != on[2, :4]).all(), R.case_id(c)
        unfused = (t.astype(f32) * a.numpy().astype(f32)).astype(f32) + b.numpy().astype(f32)
        if rows_ge(c, 8):
            assert ((unfused <= 0) & on.numpy())[:, 4].any(), R.case_id(c)


def rows_ge(c, n):
    return R.rows_in(c) >= n


# ==== planted defects: a copy of the reference, one thing wrong ==========================================================
def bad_fwd_taps(N, Hi, Wi, s, defect):
    """conv_refs.fwd_taps with `defect`: "border" a tap above / left of the image reads the border pixel instead of zero;
    "image" a tap below the last row reads on in memory (the next image's first row)"""
    n, ho, wo = R._grid(N, (Hi - 1) // s + 1, (Wi - 1) // s + 1)
    cols = []
    for dh in range(3):
        for dw in range(3):
            hi, wi = ho * s + dh - 1, wo * s + dw - 1
            if defect == "border":
                hi, wi = hi.clamp_min(0), wi.clamp_min(0)
            ok = (hi >= 0) & (wi >= 0) & (wi < Wi) & ((hi < Hi) | ((n + 1 < N) if defect == "image" else False))
            cols.append(torch.where(ok, (n * Hi + hi) * Wi + wi, torch.full_like(n, -1)))
    return torch.stack(cols, 1)


def bad_gather_rows(N, Hi, Wi, s):
    """conv_refs.gather_rows with Wo where Wi belongs"""
    Wo = (Wi - 1) // s + 1
    n, ho, wo = R._grid(N, (Hi - 1) // s + 1, Wo)
    return (n * Hi + ho * s) * Wo + wo * s


def bad_dgrad_taps(N, Hi, Wi, s):
    """conv_refs.dgrad_taps with the tap set of parity class (1, 1) taken for dh mirrored"""
    Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
    n, hi, wi = R._grid(N, Hi, Wi)
    cols = []
    for dh in range(3):
        for dw in range(3):
            odd = (hi % 2 == 1) & (wi % 2 == 1)
            th, tw = hi + 1 - torch.where(odd, 2 - dh, dh), wi + 1 - dw
            ok = (th >= 0) & (tw >= 0) & (th % s == 0) & (tw % s == 0)
            ho, wo = torch.div(th, s, rounding_mode="floor"), torch.div(tw, s, rounding_mode="floor")
            ok = ok & (ho < Ho) & (wo < Wo)
            cols.append(torch.where(ok, (n * Ho + ho) * Wo + wo, torch.full_like(n, -1)))
    return torch.stack(cols, 1)


def _unfused_mask(c, I, ge=False):
    f32 = np.float32
    _, xhat = R.mask_of(c, I)
    folded = "f" in c.var
    a, b = (I["ss"][:, 0], I["ss"][:, 1]) if folded else (I["gamma"], I["beta"])
    t = (I["z"] if folded else xhat).numpy().astype(f32)
    if ge:
        v = t.astype(np.float64) * a.numpy().astype(np.float64) + b.numpy().astype(np.float64)
        return torch.from_numpy(v >= 0)
    return torch.from_numpy(((t * a.numpy().astype(f32)).astype(f32) + b.numpy().astype(f32)) > 0)


def _defective(defect, c, I):
    """(out, partials) of case c with the defect, evaluated in fp64 so that nothing else is wrong; None where the defect
    does not apply to the case"""
    dt = torch.float64
    if defect in ("border tap not zeroed", "tap read across the image boundary"):
        if c.op not in ("f3", "w3", "h3"):
            return None
        tab = {"idx": bad_fwd_taps(c.N, c.Hi, c.Wi, c.s, "border" if "border" in defect else "image")}
        return finish(c, I, R.reference(c, I, dt, tab)["out"], dt)
    if defect == "gather with Wo for Wi":
        if c.op not in ("f1", "w1") or c.s == 1:
            return None
        return finish(c, I, R.reference(c, I, dt, {"rows": bad_gather_rows(c.N, c.Hi, c.Wi, c.s)})["out"], dt)
    if defect == "a parity class with the wrong tap set":
        if c.op != "s3":
            return None
        return finish(c, I, R.reference(c, I, dt, {"idx": bad_dgrad_taps(c.N, c.Hi, c.Wi, c.s)})["out"], dt)
    if defect == "partial one block slot off":
        if c.epi not in (1, 2) or R.row_tiles(R.stat_rows(c)) < 2:
            return None
        out, part = finish(c, I, R.reference(c, I, dt)["out"], dt)
        moved = part.roll(1, dims=2)
        assert torch.allclose(moved.sum(2), part.sum(2), atol=1e-4)          # the old check's column sums cannot tell
        return out, moved
    if defect in ("mask without the fused rounding", "mask from >= 0"):
        if c.epi != 2:
            return None
        return finish(c, I, R.reference(c, I, dt)["out"], dt, on=_unfused_mask(c, I, ge=">=" in defect))
    if defect == "last k-granule dropped":
        if c.op != "f1" or c.s > 1 or c.epi == 3:
            return None
        a = R.prologue(I["x"].to(dt), I["ss"].to(dt)) if c.pro else I["x"].to(dt)
        w = I["w"].to(dt)
        return finish(c, I, R.reference(c, I, dt)["out"] - a[:, -4:] @ w[:, -4:].t(), dt)
    raise ValueError(defect)


DEFECTS = ["border tap not zeroed", "tap read across the image boundary", "partial one block slot off",
           "mask without the fused rounding", "mask from >= 0", "gather with Wo for Wi", "a parity class with the wrong tap set",
           "last k-granule dropped"]


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.replace(" ", "_") for d in DEFECTS])
def test_planted_defect_fails(defect):
    applied = caught = 0
    for c in R.CASES:
        I = R.inputs(c)
        bad = _defective(defect, c, I)
        if bad is None:
            continue
        good = finish(c, I, R.reference(c, I)["out"], torch.float64)
        assert _passes(c, I, *good), "the defect-free evaluation of %s fails" % R.case_id(c)
        applied += 1
        caught += not _passes(c, I, *bad)
    print("%s: caught at %d of %d rows" % (defect, caught, applied))
    assert applied and caught >= 1


# ==== the dispatch, asked of the library ===============================================================================
def _required():
    req = set()
    for mi in (1, 2, 4):
        for pro in (0, 1):
            for g in (0, 1):
                req.add(("cgemm<MI%d NT PRO%d EPI1 G%d C3_0>" % (mi, pro, g), None))
        req.add(("cgemm<MI%d NN PRO0 EPI2 G0 C3_0>" % mi, None))
        for c3 in (1, 2, 4):
            req.add(("cgemm<MI%d %s PRO0 EPI0 G0 C3_%d>" % (mi, "NT" if c3 == 1 else "NN", c3), None))
    req |= {("cgemm<MI1 TN PRO0 EPI0 G0 C3_3>", None), ("cgemm<MI2 TN PRO0 EPI0 G0 C3_3>", None),
            ("cgemm<MI2 TN PRO0 EPI0 G0 C3_3>", "creduce<1>")}
    return req


# any row tile: (what the instance name must hold, the second launch)
REQUIRED_ANY_MI = [
    ("NT PRO0 EPI1 G0 C3_1", None), ("NN PRO0 EPI2 G0 C3_2", None), ("NT PRO0 EPI3 G0 C3_0", None), ("NT PRO0 EPI3 G1 C3_0", None),
    ("NT PRO0 EPI3 G0 C3_1", None), ("TN PRO2 EPI0 G0 C3_0", None), ("TN PRO2 EPI0 G1 C3_0", None), ("TN PRO0 EPI0 G0 C3_0", None),
    ("TN PRO0 EPI0 G1 C3_0", None), ("NT PRO1 EPI0 G0 C3_0", None), ("NT PRO1 EPI0 G0 C3_0", "cstats<1> from slabs"),
    ("NN PRO0 EPI0 G0 C3_0", "cstats<2> from slabs"), ("NT PRO0 EPI0 G0 C3_0", "cstats<2> from C"),
    ("NT PRO0 EPI0 G0 C3_1", "creduce<1>"), ("NT PRO0 EPI0 G0 C3_1", "cstats<1> from slabs"),
    ("NN PRO0 EPI0 G0 C3_2", "cstats<2> from slabs"),
    ("conv3_wgrad<16>", None), ("conv3_wgrad<16>", "creduce<1>"), ("conv3_wgrad<8>", None), ("conv3_wgrad<8>", "creduce<1>"),
]


def test_table_reaches_every_instance():
    seen = {T.dispatch(c)[:2] for c in R.CASES}
    missing = sorted(_required() - seen, key=str)
    missing += [r for r in REQUIRED_ANY_MI if not any(r[0] in inst and r[1] == second for inst, second in seen)]
    assert not missing, missing


def test_table_holds_the_edges_the_issue_names():
    info = {R.case_id(c): (c, T.dispatch(c)) for c in R.CASES}
    rows = list(info.values())
    # a 3x3 K-slice boundary inside a tap
    assert any(c.op == "f3" and m[2]["S"] > 1 and m[2]["kper"] % c.Cin for c, m in rows)
    # deeper than cgemm_combine_max; a second slice whose prologue pairs start at kbeg != 0
    assert any(c.op == "f1" and c.pro == 1 and m[2]["S"] == 9 and not m[2]["comb"] for c, m in rows)
    assert any(c.op == "f1" and c.pro == 1 and c.epi == 1 and m[2]["S"] in (2, 3) and m[2]["comb"] for c, m in rows)
    # the halo kernel with fewer strip lines than waves, and every forced split legal
    assert {m[2]["Q"] for c, m in rows if c.op == "h3"} >= {1, 2, 32, 54}
    assert {m[2]["S"] for c, m in rows if c.op == "h3"} == {1, 2, 3}
    # gathers on the non-square odd map, with both prologues; stat_shift NULL and given; both mask forms on each layout
    assert any(c.op == "f1" and c.s == 2 and c.pro == 1 and (c.Hi, c.Wi) == (7, 5) for c, m in rows)
    assert any(c.op == "w1" and c.s == 2 and c.pro == 2 and (c.Hi, c.Wi) == (7, 5) for c, m in rows)
    for op in ("f1", "f3"):
        assert {("s" in c.var) for c, m in rows if c.op == op and c.epi == 1} == {True, False}
    for op in ("d1", "d3"):
        assert {("f" in c.var) for c, m in rows if c.op == op and c.epi == 2} == {True, False}
    assert any(c.op == "d1" and "t" in c.var and c.epi == 2 and m[1] == "cstats<2> from C" for c, m in rows)
    # the 128 x 64 tile picked by the policy itself
    assert any(c.op == "f1" and c.mi == 0 and m[2]["mi"] == 4 for c, m in rows)
    assert any(c.op == "s3" and c.mi == 0 and not c.opts and m[2]["mi"] == 4 for c, m in rows)


def test_refusals_are_what_the_mirror_refuses():
    """the library refuses every row of REFUSALS with the message the row names: the argument checks run on host windows"""
    for what, c, wsf, msg in T.REFUSALS:
        with pytest.raises(RuntimeError, match=msg):
            T._run(T.CPU, c, wsf=wsf)
