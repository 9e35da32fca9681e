"""GPU tests (``-m gpu``) of the reward-weighted loss, scnattn_caption_loss_weighted_fwd / _bwd (csrc/loss.hip), through the C
ABI: per element against fp64 the way tests/test_gpu_train_tail_kernels.py judges the unweighted pair (row_lse within 16 u of
the largest log-sum-exp, d scores by the derived bound of tests/train_tail_refs.py times |w[b]| plus the one further rounding,
sm1 and d alphas by the sum rule), and BIT FOR BIT against scnattn_caption_loss_fwd / _bwd when every weight is 1.0.

B = 3, T = 4, V = 37 (scalar form) and 1003 is odd too, so V = 1004 joins it for the vector form; P = 9; lengths (4, 0, 2): a
row of length 0, whose weight is NaN and must not be read; negative and zero weights; NaN in every undecoded score row."""
import pytest
import torch

import rollout_refs as RR
import train_tail_refs as TT
from kernel_harness import GBuf, GBufI, U, _bound_ok, _call, _sum_ok, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "reward-weighted caption loss vs fp64: worst |got - ref| / bound over all cases"

B, T, P, LDT = 3, 4, 9, 6
LENS = (4, 0, 2)
ALPHA_C = TT.f32(0.7)
GOUT = 2.5
WEIGHTS = ((-1.5, float("nan"), 0.0), (2.25, float("nan"), -0.5))
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _case(V, lens=LENS):
    g = torch.Generator().manual_seed(300 + V)
    scores = (torch.randn(B, T, V, generator=g) * 3.0).float()
    targets = torch.full((B, LDT), V + 5, dtype=torch.int64)
    for b in range(B):
        for t in range(lens[b]):
            targets[b, t] = int(torch.randint(0, V, (1,), generator=g))
        scores[b, lens[b]:] = NAN
    targets[0, 0], targets[0, 1] = 0, V - 1
    alphas = (torch.rand(B, T, P, generator=g) * 0.5).float()
    return scores, targets, alphas


def _fwd(dev, name, scores, targets, alphas, lens, weight, ms=0):
    V = scores.shape[2]
    sb, ab = GBuf(dev, (B, T, V), vals=scores, mis=ms), GBuf(dev, (B, T, P), vals=alphas, mis=1)
    tb, dl = GBufI(dev, B * LDT, vals=targets, wide=True), GBufI(dev, B, vals=torch.tensor(lens, dtype=torch.int32))
    outs = [GBuf(dev, s, out=True) for s in ((B * T,), (B * T,), (B, P), (B,), (1,))]
    head = (B, T, V, P, sb.ptr, tb.ptr, LDT, dl.ptr, sum(lens))
    tail = (ab.ptr, ALPHA_C) + tuple(o.ptr for o in outs)
    if weight is None:
        _call(name, dev, *head, *tail)
    else:
        wb = GBuf(dev, (B,), vals=weight, mis=1)
        _call(name, dev, *head, wb.ptr, *tail)
    return tuple(o.read(n) for o, n in zip(outs, ("row_lse", "row_loss", "sm1", "reg_part", "loss")))


def _bwd(dev, name, scores, targets, lens, weight, row_lse, sm1, ms=0, md=0):
    V = scores.shape[2]
    sb, tb = GBuf(dev, (B, T, V), vals=scores, mis=ms), GBufI(dev, B * LDT, vals=targets, wide=True)
    dl, lb = GBufI(dev, B, vals=torch.tensor(lens, dtype=torch.int32)), GBuf(dev, (B * T,), vals=row_lse.reshape(-1))
    gb, mb = GBuf(dev, (1,), vals=torch.tensor([GOUT])), GBuf(dev, (B, P), vals=sm1)
    ds, da = GBuf(dev, (B, T, V), out=True, mis=md), GBuf(dev, (B, T, P), out=True, mis=1)
    head = (B, T, V, P, sb.ptr, tb.ptr, LDT, dl.ptr, sum(lens))
    tail = (lb.ptr, mb.ptr, ALPHA_C, gb.ptr, ds.ptr, da.ptr)
    if weight is None:
        _call(name, dev, *head, *tail)
    else:
        wb = GBuf(dev, (B,), vals=weight, mis=1)
        _call(name, dev, *head, wb.ptr, *tail)
    return ds.read("dscores"), da.read("dalphas")


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", (37, 1003, 1004))
def test_weighted_loss_vs_fp64(dev, V):
    scores, targets, alphas = _case(V)
    live = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        live[b, :LENS[b]] = True
    for wi, w in enumerate(WEIGHTS):
        weight = torch.tensor(w, dtype=torch.float32)
        for ms, md in ((0, 0), (1, 0), (0, 1)):
            form = "ce weighted %s" % ("vector" if V % 4 == 0 and not ms and not md else "scalar")
            row_lse, row_loss, sm1, reg_part, loss = _fwd(dev, "scnattn_caption_loss_weighted_fwd", scores, targets, alphas, LENS,
                                                          weight, ms)
            ref = RR.weighted_loss(torch.nan_to_num(scores).double(), targets, LENS, torch.nan_to_num(weight).double(),
                                   alphas.double(), ALPHA_C)
            row_lse, row_loss = row_lse.reshape(B, T), row_loss.reshape(B, T)
            assert bool((_bits(row_lse)[~live] == 0).all()) and bool((_bits(row_loss)[~live] == 0).all())
            lse_bound = 16 * U * float(ref["row_lse"].abs().max())
            dlse = torch.where(live, (row_lse.double() - ref["row_lse"]).abs(), torch.zeros(B, T, dtype=torch.float64))
            assert float(dlse.max()) <= lse_bound, (float(dlse.max()), lse_bound)
            # row_loss = fl(fl(lse - x[tg]) * w): the log-sum-exp's distance, one rounding of the difference, one of the product
            wabs = torch.nan_to_num(weight).double().abs().unsqueeze(1)
            nll_abs = torch.zeros(B, T, dtype=torch.float64)
            for b in range(B):
                for t in range(LENS[b]):
                    nll_abs[b, t] = (ref["row_lse"][b, t] - scores[b, t, int(targets[b, t])].double()).abs()
            rl_bound = torch.where(live, wabs * (lse_bound + U * nll_abs) + U * ref["row_loss"].abs(), torch.zeros(B, T, dtype=torch.float64))
            _bound_ok(form, "row_loss", row_loss, ref["row_loss"], rl_bound, "=|w| (16 u max|lse| + u |nll|) + u |w nll|")
            _sum_ok("alpha_reg_fwd (weighted)", "sm1", sm1, TT.alpha_reg_ref(alphas))
            # loss: the row bounds, B*T + 8 roundings of their sum, and the regulariser's (sum rule over its B*P squares, each
            # square carrying twice the relative error of its sm1)
            n = sum(LENS)
            ar = TT.alpha_reg_ref(alphas)
            sq_err = 2.0 * ar["sm1"].abs() * (ar["sm1_n"] + 8) * U * ar["sm1_abs"] + 2 * U * ar["sm1"] ** 2
            reg = float((ar["sm1"] ** 2).sum()) * ALPHA_C / (B * P)
            bound = (float(rl_bound.sum()) + (B * T + 8) * U * float(ref["row_loss"].abs().sum())) / n \
                + ALPHA_C / (B * P) * float(sq_err.sum()) + (B * P + B + 12) * U * reg + 4 * U * abs(float(ref["loss"]))
            _bound_ok(form, "loss", loss, ref["loss"].reshape(1), torch.tensor([bound], dtype=torch.float64),
                      "=sum of the row bounds / n + the sum rule over the rows and over the regulariser's squares")
            # the backward at the fp32 rounding of the fp64 log-sum-exp (the forward kernel is not in the loop)
            lse32 = ref["row_lse"].float()
            ds, da = _bwd(dev, "scnattn_caption_loss_weighted_bwd", scores, targets, LENS, weight, lse32, sm1, ms, md)
            ds = ds.reshape(B, T, V)
            assert bool((_bits(ds)[~live] == 0).all()), "d scores of an undecoded row is not +0.0 everywhere"
            want, dbound = RR.weighted_bwd(torch.nan_to_num(scores), targets, lse32, torch.nan_to_num(weight), LENS, GOUT)
            _bound_ok(form, "dscores", ds, want, dbound, "=|w| x the bound of ce_bwd + u |want|")
            if wi == 0:
                assert bool((_bits(ds[2]) << 1 == 0).all()), "a zero weight must give zero gradients"      # +0.0 or -0.0
            _sum_ok("alpha_reg_bwd (weighted)", "dalphas", da, TT.dalphas_ref(sm1, T, GOUT, ALPHA_C))


@pytest.mark.parametrize("V", (37, 1003, 1004))
def test_unit_weights_give_the_bits_of_the_unweighted_pair(dev, V):
    lens = (4, 2, 1)
    scores, targets, alphas = _case(V, lens)
    ones = torch.ones(B)
    for ms, md in ((0, 0), (1, 0), (0, 1)):
        a = _fwd(dev, "scnattn_caption_loss_fwd", scores, targets, alphas, lens, None, ms)
        b = _fwd(dev, "scnattn_caption_loss_weighted_fwd", scores, targets, alphas, lens, ones, ms)
        for name, x, y in zip(("row_lse", "row_loss", "sm1", "reg_part", "loss"), a, b):
            assert torch.equal(_bits(x), _bits(y)), "%s differs in bits (V = %d, offset %d)" % (name, V, ms)
        da = _bwd(dev, "scnattn_caption_loss_bwd", scores, targets, lens, None, a[0], a[2], ms, md)
        db = _bwd(dev, "scnattn_caption_loss_weighted_bwd", scores, targets, lens, ones, a[0], a[2], ms, md)
        for name, x, y in zip(("dscores", "dalphas"), da, db):
            assert torch.equal(_bits(x), _bits(y)), "%s differs in bits (V = %d, offsets %d / %d)" % (name, V, ms, md)
    # and the weights do something: twice the weight, twice the cross-entropy part of the loss
    c = _fwd(dev, "scnattn_caption_loss_weighted_fwd", scores, targets, alphas, lens, ones * 2, 0)
    assert torch.equal(_bits(c[1]), _bits(a[1] * 2)) and not torch.equal(_bits(c[4]), _bits(a[4]))


def test_functional_caption_loss_weighted(dev):
    """scnattn.functional.caption_loss_weighted: forward and autograd against the fp64 formula in torch; unit weights equal
    caption_loss bit for bit, loss and gradients"""
    from scnattn import functional as SF
    V, lens = 1003, (4, 2, 1)
    scores, targets, alphas = _case(V, lens)
    scores = torch.nan_to_num(scores)
    caps = torch.cat([torch.zeros(B, 1, dtype=torch.long), targets.clamp(0, V - 1)], dim=1).to(dev)
    w = torch.tensor([-1.5, 0.0, 2.0])

    def run(fn, *extra):
        s, a = scores.to(dev).requires_grad_(True), alphas.to(dev).requires_grad_(True)
        loss = fn(s, caps, list(lens), *extra, alphas=a, alpha_c=ALPHA_C)
        loss.backward()
        return loss.detach().cpu(), s.grad.cpu(), a.grad.cpu()
    got = run(SF.caption_loss_weighted, w.to(dev))
    s64, a64 = scores.double().requires_grad_(True), alphas.double().requires_grad_(True)
    n = sum(lens)
    want = sum(w[b].double() * (torch.logsumexp(s64[b, t], 0) - s64[b, t, caps[b, t + 1].cpu()]) for b in range(B) for t in range(lens[b])) / n \
        + ALPHA_C * ((1.0 - a64.sum(dim=1)) ** 2).mean()
    want.backward()
    want = want.detach()
    assert abs(float(got[0]) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    assert float((got[1].double() - s64.grad).abs().max()) <= 1e-6 * float(s64.grad.abs().max())
    assert float((got[2].double() - a64.grad).abs().max()) <= 1e-6 * float(a64.grad.abs().max())
    one = run(SF.caption_loss_weighted, torch.ones(B, device=dev))
    plain = run(SF.caption_loss)
    for x, y in zip(one, plain):
        assert torch.equal(_bits(x), _bits(y))
    with pytest.raises(RuntimeError, match="row_weight"):
        SF.caption_loss_weighted(scores.to(dev), caps, list(lens), torch.ones(B + 1, device=dev))
