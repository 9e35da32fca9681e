"""GPU tests (``-m gpu``) of the scoring kernel of csrc/rollout.hip through the C ABI, alone: scnattn_rollout_score per row
against the fp64 reference of tests/scoring_refs.py run on the device's own fp32 y (the bound of logp: its docstring; rank, best,
token, sum_logp and the counters exactly).  EVERY record of EVERY row is compared: nothing is left out.

Buffers are guarded windows (tests/kernel_harness.py): NaN around the logits and in the gap ld - V of every row, the sentinel
around and inside every record.  A case (tests/scoring_cases.py: the flavours of a row, the load paths, how rows close) walks
three steps on one state.  The kernel has ONE form for every V (it reads the L2-resident row twice and holds nothing in
registers), so there is no force_passes switch and no second set of bits to compare; the four load paths of a case must
agree bit for bit instead."""
import ctypes as C

import pytest
import torch

import scoring_cases as SC
from kernel_harness import GBuf, GBufI, SENTI, _call, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "scoring kernel vs fp64: worst |got - ref| / bound over all cases (tests/scoring_refs.py: the bound)"
STEPS = SC.STEPS
RECORDS = SC.RECORDS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run_case(dev, V, case, steps=STEPS, target=None):
    """-> host copies of every buffer after `steps` steps (guards checked); the records as [STEPS, R]"""
    N, K = case["N"], case["K"]
    R = N * K
    ntok, nsrc = case["ntok"], case["nsrc"]
    target = case["target"] if target is None else target
    nopen = torch.where(nsrc > 0, (ntok.view(N, K) > 0).sum(dim=1).to(torch.int32), torch.zeros_like(nsrc))
    bufs = dict(open_rows=GBufI(dev, 1, vals=nopen.sum()), nsrc=GBufI(dev, N, vals=nsrc), nopen=GBufI(dev, N, vals=nopen),
                ntok=GBufI(dev, R, vals=ntok), sum_logp=GBuf(dev, (R,), vals=torch.zeros(R), out=True),
                token=GBufI(dev, STEPS * R), logp=GBuf(dev, (STEPS, R), out=True), rank=GBufI(dev, STEPS * R),
                best=GBufI(dev, STEPS * R), target=GBufI(dev, STEPS * R, vals=target))
    arr = (C.c_void_p * 7)(*[bufs[k].ptr for k in ("open_rows", "nsrc", "nopen", "ntok", "sum_logp", "token", "logp")])
    at = lambda name, t: C.c_void_p(bufs[name].ptr.value + 4 * t * R)      # noqa: E731
    for t in range(steps):
        lb = GBuf(dev, (R, V), (case["ld"], 1), vals=case["logits"][t], mis=case["mis"])
        _call("scnattn_rollout_score", dev, N, K, V, lb.ptr, case["ld"], case["inv_temp"], t, STEPS, arr, at("target", t),
              at("rank", t), at("best", t))
    got = {k: b.read(k) for k, b in bufs.items()}
    for k in RECORDS + ("target",):
        got[k] = got[k].view(STEPS, R)
    got["nopen0"] = nopen
    return got


bits, judge = SC.bits, SC.judge


@pytest.mark.parametrize("cfg", sorted(SC.CONFIGS))
@pytest.mark.parametrize("V", SC.VS)
def test_rollout_score(dev, V, cfg):
    total = {}
    first = {}
    for run in range(len(SC.RUNS)):
        case = SC.gen_case(V, cfg, run)
        got = run_case(dev, V, case)
        seen = judge(V, case, got, case["form"])
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        again = run_case(dev, V, case)          # determinism: two runs give equal bits
        for k in RECORDS + ("sum_logp", "nopen", "open_rows"):
            assert torch.equal(bits(got[k]), bits(again[k])), (case["form"], k)
        # the load paths add the same numbers in the same order: the case of this temperature through another path
        f, it = SC.RUNS[run]
        if f == 0:
            first[it] = (case, got)
        else:
            moved = run_case(dev, V, dict(first[it][0], ld=case["ld"], mis=case["mis"]))
            for k in RECORDS + ("sum_logp",):
                assert torch.equal(bits(first[it][1][k]), bits(moved[k])), ("load paths differ", case["form"], k)
    N, K, closed = SC.CONFIGS[cfg]
    print("%s V=%d: %s" % (cfg, V, total))
    assert total["open"] > 0 and total["zero"] > 0 and total["closing"] > 0
    assert (total["closed_image"] > 0) == (closed is not None)
    if V > 1:
        assert total["ties"] > 0
    if V > 1 and N * K > 1:
        assert total["inf"] > 0 and total["pzero"] > 0 and total["allequal"] > 0, total


def test_target_outside_the_vocabulary(dev):
    """logp = NaN and rank = V, best still the row's; the rows beside it are what they are without it"""
    V, cfg = 257, "N1K3"
    case = SC.gen_case(V, cfg, 2)
    case["ntok"] = torch.tensor([3, 3, 3], dtype=torch.int32)
    clean = run_case(dev, V, case)
    judge(V, case, clean, "clean")
    bad = case["target"].clone()
    bad[0, 1], bad[1, 1], bad[2, 0] = V, -1, SENTI
    got = run_case(dev, V, case, target=bad)
    for t in range(STEPS):
        for r in range(3):
            if int(bad[t, r]) == int(case["target"][t, r]):       # a step's records do not depend on the steps before it
                for k in RECORDS:
                    assert int(bits(got[k])[t, r]) == int(bits(clean[k])[t, r]), (t, r, k)
            else:
                assert int(got["token"][t, r]) == int(bad[t, r]) and int(got["rank"][t, r]) == V, (t, r)
                assert bool(torch.isnan(got["logp"][t, r])) and int(got["best"][t, r]) == int(clean["best"][t, r]), (t, r)
    assert bool(torch.isnan(got["sum_logp"][:2]).all()) and int(bits(got["sum_logp"])[2]) == int(bits(clean["sum_logp"])[2])
    assert torch.equal(got["nopen"], clean["nopen"]) and int(got["open_rows"]) == int(clean["open_rows"])


def test_refusals(dev):
    V, case = 5, SC.gen_case(5, "N1K3", 0)
    lb = GBuf(dev, (3, V), (case["ld"], 1), vals=case["logits"][0])
    ib = GBufI(dev, 3 * STEPS, vals=torch.zeros(3 * STEPS))
    fb = GBuf(dev, (3 * STEPS,), vals=torch.zeros(3 * STEPS), out=True)
    arr = (C.c_void_p * 7)(ib.ptr, ib.ptr, ib.ptr, ib.ptr, fb.ptr, ib.ptr, fb.ptr)
    for args in ((1, 9, V, lb.ptr, case["ld"], 1.0, 0, STEPS, arr, ib.ptr, ib.ptr, ib.ptr),             # K > 8
                 (1, 3, V, lb.ptr, case["ld"], 0.0, 0, STEPS, arr, ib.ptr, ib.ptr, ib.ptr),             # inv_temp
                 (1, 3, V, lb.ptr, case["ld"], float("inf"), 0, STEPS, arr, ib.ptr, ib.ptr, ib.ptr),
                 (1, 3, V, lb.ptr, V - 1, 1.0, 0, STEPS, arr, ib.ptr, ib.ptr, ib.ptr),                  # ld < V
                 (1, 3, V, lb.ptr, case["ld"], 1.0, STEPS, STEPS, arr, ib.ptr, ib.ptr, ib.ptr),         # step beyond the records
                 (1, 3, V, lb.ptr, case["ld"], 1.0, 0, STEPS, arr, None, ib.ptr, ib.ptr)):              # a null record
        with pytest.raises(RuntimeError):
            _call("scnattn_rollout_score", dev, *args)
    assert bool((ib.read("untouched") == 0).all())
