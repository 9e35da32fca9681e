"""CPU tests of tests/eval16_refs.py, the yardstick of tests/test_gpu_eval16_kernels.py: torch's own evaluation passes the
derived per-element bound at every case, every planted defect fails it, and the launch plans of the cases' own calls
(test_gpu_eval16_kernels.dispatch: scnattn_plan_next on host windows) show that the case table reaches every new kernel
instance, the eval reducer, and both the forced and the policy-chosen split."""
import pytest
import torch

import eval16_refs as E
import test_gpu_eval16_kernels as T

_REFS = {}


def _ref(i):
    if i not in _REFS:
        c = E.CASES[i]
        I = E.inputs(c, i)
        _REFS[i] = (I, E.reference(c, I))
    return _REFS[i]


def test_case_ids_are_unique():
    ids = [E.case_id(c) for c in E.CASES]
    assert len(set(ids)) == len(ids)


def test_torch_cpu_evaluation_passes_the_bound_at_every_case():
    worst = 0.0
    for i, c in enumerate(E.CASES):
        I, ref = _ref(i)
        ok, ratio = E.judge(E.cpu_eval(c, I), ref)
        print("%-60s err/bound %.3f" % (E.case_id(c), ratio))
        worst = max(worst, ratio)
        assert ok, "%s: err/bound %.3f" % (E.case_id(c), ratio)
    print("torch CPU evaluation: worst err/bound %.3f over %d cases" % (worst, len(E.CASES)))


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_planted_defect_fails(defect):
    n = 0
    for i, c in enumerate(E.CASES):
        if not E.applies(defect, c):
            continue
        I, ref = _ref(i)
        ok, ratio = E.judge(E.cpu_eval(c, I, defect), ref)
        assert not ok, "%s slipped through at %s (err/bound %.3f)" % (defect, E.case_id(c), ratio)
        n += 1
    assert n >= 2, "%s: planted at %d cases only" % (defect, n)


def test_reference_is_the_fp64_module_arithmetic():
    """The index-table reference against F.conv2d + the BatchNorm formula in fp64 (an independent construction)."""
    for i, c in enumerate(E.CASES):
        if c.op != "f3" or c.split > 1:
            continue
        I, ref = _ref(i)
        x4 = I["x"].double().view(c.N, c.Hi, c.Hi, c.Cin).permute(0, 3, 1, 2)
        w4 = I["w"].double().view(c.Cout, 3, 3, c.Cin).permute(0, 3, 1, 2)
        z = torch.nn.functional.conv2d(x4, w4, stride=c.s, padding=1)
        y = torch.nn.functional.batch_norm(z, I["mean"].double(), I["var"].double(), I["gamma"].double(), I["beta"].double(),
                                           False, 0.0, float(torch.tensor(c.eps, dtype=torch.float32)))
        y = y.permute(0, 2, 3, 1).reshape(c.R, c.Cout)
        if I["res"] is not None:
            y = y + I["res"].double()
        assert (y - ref["pre"]).abs().max() <= 1e-12 * ref["pre"].abs().max()


def test_case_table_reaches_every_instance_and_both_splits():
    m = [T.dispatch(c) for c in E.CASES]
    insts = {d["inst"] for d in m}
    # cgemm16_kernel<MI, EPI 3, GATHER, OBF, C3>: plain and gathered 1x1, 3x3, each at both row tiles
    for want in [(mi, 3, gather, 0) for mi in (1, 2) for gather in (False, True)] + [(mi, 3, False, 1) for mi in (1, 2)]:
        assert want in insts, "no case reaches cgemm16_kernel<MI %d, EPI %d, GATHER %s, C3 %d>" % want
    split = [d for d in m if d["S"] > 1]
    assert all(d["reduce"] == "eval" and d["inst"][1] == 0 for d in split)
    assert any(d["forced"] and d["S"] == 2 for d in split) and any(d["forced"] and d["S"] == 4 for d in split)
    assert any(not d["forced"] for d in split), "no case the policy splits by itself"
    assert any(d["inst"][3] == 1 for d in split) and any(d["inst"][2] for d in split)      # a split 3x3, a split gather
    # the shape the issue names: R = 128, 1024 -> 256 is split by the policy
    d = T.dispatch(E.f1(128, 1024, 256, True, True))
    assert (d["mi"], d["S"], d["kper"], d["forced"]) == (1, 4, 256, False)
    # kper in whole 32-k stages, every slab non-empty
    for c, d in zip(E.CASES, m):
        K = E.mkn(c)[2]
        assert d["kper"] % 32 == 0 and (d["S"] - 1) * d["kper"] < K <= d["S"] * d["kper"], E.case_id(c)
        assert d["S"] * c.R * c.Cout <= E.WS_FLOATS
