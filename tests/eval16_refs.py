"""fp64 references, case table, inputs, judge and instance description of the eval BatchNorm epilogue on bf16 maps
(include/scnattn.h scnattn_conv1x1_fwd_bn_eval16 / scnattn_conv3x3_fwd_bn_eval16; csrc/cgemm16.hip EPI 3 and the eval
form of creduce16_kernel).  Shared by tests/test_eval16_refs.py (CPU) and tests/test_gpu_eval16_kernels.py.

Reference: conv_refs.bn_eval on the fp64 product of the bf16 operands widened exactly.  The operands are generated as
bf16, so every product term is exact in fp32 and fp64; the residual is bf16, widened.

Bound, per element, derived and not measured: b = (n + 16) * 2^-24 * mag is conv_refs.bn_eval's bound of the fp32
pre-activation (n + 8 for the fp32 accumulation of n exact terms, 8 for what the epilogue rounds), then

    |got - ref| <= b + 2^-8 * (|pre| + b)

the second term being the single round-to-nearest-even to bf16 of a value within b of pre (8 significant bits: unit
roundoff 2^-8).  ReLU is 1-Lipschitz and commutes with the rounding, so the bound holds after the clamp and no element is
excluded.

`describe` reads the launch plan of a case's own call (scnattn_plan_next; test_gpu_eval16_kernels.dispatch) through
conv16_refs.names: row tile mi, S, kper in whole 32s, and where the epilogue runs -- inside the product launch when S == 1
(EPI 3), else EPI 0 + the eval creduce16.  The policy itself is cgemm16_plan (csrc/cgemm16.hip)."""
from collections import namedtuple

import torch

import conv16_refs as C16
import conv_refs as CR

BF = torch.bfloat16
U8 = 2.0 ** -8
WS_FLOATS = 4 << 20         # the workspace the GPU test passes

# op f1: 1x1 on R rows (gather = (N, Hi, s): rows gathered from an N x Hi x Hi map at stride s, R follows);
# op f3: 3x3 / pad 1 on an N x Hi x Hi map at stride s.  res: a bf16 residual with ldres = Cout + 8.  eps: the BatchNorm's.
Case = namedtuple("Case", "op R N Hi s Cin Cout relu res mi split eps gather")


def f1(R, Cin, Cout, relu, res, mi=0, split=0, eps=1e-5, gather=None):
    N, Hi, s = gather if gather else (0, 0, 1)
    if gather:
        Ho = (Hi - 1) // s + 1
        R = N * Ho * Ho
    return Case("f1", R, N, Hi, s, Cin, Cout, relu, res, mi, split, eps, gather is not None)


def f3(N, Hi, s, Cin, Cout, relu, res, mi=0, split=0, eps=1e-5):
    Ho = (Hi - 1) // s + 1
    return Case("f3", N * Ho * Ho, N, Hi, s, Cin, Cout, relu, res, mi, split, eps, False)


def case_id(c):
    return "%s-R%d-%dx%d-s%d-%dto%d-%s%s-mi%d-S%d-eps%g%s" % (c.op, c.R, c.N, c.Hi, c.s, c.Cin, c.Cout, "l" if c.relu else "",
                                                               "r" if c.res else "", c.mi, c.split, c.eps, "-g" if c.gather else "")


# The smallest shapes at which a path can go wrong: rows 16 / 64 / 65 / 200 (below, at, one past a 64-row tile, several
# tiles), Cin 40 (a partial 32-k stage) / 64 / 1024, Cout 72 (an edge inside a wave's 64 columns) / 256 (two column tiles).
CASES = [
    # un-split 1x1: ReLU x residual, both row tiles
    f1(16, 40, 72, True, True),
    f1(64, 64, 72, True, False),
    f1(65, 40, 256, False, True, mi=1),
    f1(65, 40, 256, False, True, mi=2),
    f1(200, 64, 72, True, True, mi=1),
    f1(200, 64, 72, True, False, mi=2),
    f1(200, 64, 72, False, True, mi=2, eps=0.1),
    f1(200, 64, 72, False, False, mi=1),
    f1(200, 1024, 256, True, True, split=1),            # deep K kept in one launch
    # the gathered 1x1 (downsample) on odd maps
    f1(0, 64, 72, False, False, mi=1, gather=(2, 7, 2)),
    f1(0, 64, 72, True, True, mi=2, gather=(2, 7, 2)),
    f1(0, 40, 256, False, False, mi=2, gather=(3, 9, 2)),
    f1(0, 40, 256, True, True, mi=1, gather=(3, 9, 2), eps=0.1),
    # split-K through the eval creduce16: forced 2 / 4 at K = 1024, and one shape the policy splits by itself
    f1(200, 1024, 256, True, True, mi=1, split=2),
    f1(200, 1024, 256, False, True, mi=2, split=4),
    f1(65, 1024, 72, True, False, split=4),
    f1(16, 1024, 72, False, False, split=2),
    f1(128, 1024, 256, True, True),                     # policy: 4 tiles -> S = 4
    f1(0, 1024, 72, False, True, split=2, gather=(3, 9, 2)),
    # 3x3: maps 8 / 7 / 3 at stride 1 and 2, Cin 32 / 64 (Cin 64 is K = 576: the policy splits it, split = 1 keeps it whole)
    f3(2, 8, 1, 32, 72, True, False, mi=1),
    f3(2, 8, 2, 64, 72, True, True, mi=2, split=1),
    f3(2, 7, 1, 64, 72, False, True, mi=1, split=1),
    f3(2, 7, 2, 32, 72, True, True, mi=2),
    f3(2, 3, 1, 32, 72, True, False, mi=2, eps=0.1),
    f3(2, 3, 2, 64, 72, False, False, mi=1, split=1),
    f3(2, 7, 1, 64, 72, True, True, split=2),
    f3(2, 8, 2, 64, 72, True, False),                   # policy: K = 576 -> S = 2
]


def mkn(c):
    return c.R, c.Cout, (9 if c.op == "f3" else 1) * c.Cin


def describe(c, plan):
    """the launch plan of the case's call -> dict(mi, S, kper, inst = (MI, EPI, GATHER, C3) of the product launch,
    reduce = 'eval' | None, forced = the case asks for its split)"""
    d = C16.names(plan)
    mi, kepi, gather, obf, c3 = d["inst"]
    assert obf
    return dict(mi=mi, S=d["S"], kper=d["kper"], inst=(mi, kepi, gather, c3), reduce=d["reduce"], forced=c.split > 0)


# ==== inputs and the reference ===========================================================================================
def inputs(c, seed=0):
    """bf16 operands (x: the whole input map, w [Cout][taps][Cin], res [R][Cout] or None) and the fp32 BatchNorm vectors."""
    g = torch.Generator().manual_seed(1000 + seed)
    taps = 9 if c.op == "f3" else 1
    rows_in = c.N * c.Hi * c.Hi if (c.gather or c.op == "f3") else c.R
    x = torch.randn(rows_in, c.Cin, generator=g).to(BF)
    w = (torch.randn(c.Cout, taps, c.Cin, generator=g) / (taps * c.Cin) ** 0.5).to(BF)
    res = torch.randn(c.R, c.Cout, generator=g).to(BF) if c.res else None
    gamma = torch.rand(c.Cout, generator=g) + 0.5
    beta = torch.randn(c.Cout, generator=g) * 0.5
    mean = torch.randn(c.Cout, generator=g) * 0.5
    var = torch.rand(c.Cout, generator=g) * 1.5 + 0.5
    return dict(x=x, w=w, res=res, gamma=gamma, beta=beta, mean=mean, var=var)


def rows_of(c, wrong_width=False):
    """source rows of the gathered 1x1; wrong_width plants the Wo-for-Wi defect"""
    if not c.gather:
        return None
    if not wrong_width:
        return CR.gather_rows(c.N, c.Hi, c.Hi, c.s)
    Ho = (c.Hi - 1) // c.s + 1
    n, ho, wo = CR._grid(c.N, Ho, Ho)
    return (n * c.Hi + ho * c.s) * Ho + wo * c.s


def reference(c, I):
    """-> dict(out, pre, bound): fp64, bound = the whole per-element bound of the stored bf16 value"""
    x, w = I["x"].double(), I["w"].double()
    if c.op == "f3":
        prod = CR.conv3_fwd(x, w, CR.fwd_taps(c.N, c.Hi, c.Hi, c.s))
    else:
        prod = CR.conv1x1_fwd(x, w[:, 0], rows_of(c))
    r = CR.bn_eval(prod, I["gamma"], I["beta"], I["mean"], I["var"], c.eps, I["res"], c.relu)
    b = r["bound"]
    return dict(out=r["out"], pre=r["pre"], bound=b + U8 * (r["pre"].abs() + b))


def judge(got, ref):
    """-> (ok, worst err / bound); a NaN (an element never written) fails"""
    err = (got.double() - ref["out"]).abs()
    ratio = (err / ref["bound"].clamp_min(1e-300)).nan_to_num(1e30)
    return bool((err <= ref["bound"]).all()), float(ratio.max())


# ==== torch's own evaluation on the CPU, and the planted defects =========================================================
DEFECTS = ("res_last_group", "no_eps", "no_relu", "truncate", "shift_neighbour", "k_granule", "gather_wo")


def applies(defect, c):
    return {"res_last_group": c.res, "no_relu": c.relu, "gather_wo": c.gather, "no_eps": c.eps >= 0.1}.get(defect, True)


def cpu_eval(c, I, defect=None):
    """fp32 matmul / conv2d of the widened operands, the epilogue in fp32 steps, then .bfloat16(); `defect` plants one."""
    x, w = I["x"].float(), I["w"].float()
    if defect == "k_granule":           # the last 8 k of the product never added
        w = w.clone()
        w[:, -1, -8:] = 0
    if c.op == "f3":
        x4 = x.view(c.N, c.Hi, c.Hi, c.Cin).permute(0, 3, 1, 2)
        w4 = w.view(c.Cout, 3, 3, c.Cin).permute(0, 3, 1, 2)
        z = torch.nn.functional.conv2d(x4, w4, stride=c.s, padding=1).permute(0, 2, 3, 1).reshape(c.R, c.Cout)
    else:
        rows = rows_of(c, defect == "gather_wo")
        z = (x if rows is None else x[rows]) @ w[:, 0].t()
    scale = I["gamma"] * (1.0 / torch.sqrt(I["var"] + (0.0 if defect == "no_eps" else c.eps)))
    shift = I["beta"] - I["mean"] * scale
    if defect == "shift_neighbour":
        shift = shift.roll(1)
    y = z * scale + shift
    if c.res is not None and I["res"] is not None:
        r = I["res"].float()
        if defect == "res_last_group":
            r = r.clone()
            r[:, -8:] = 0
        y = y + r
    if c.relu and defect != "no_relu":
        y = torch.relu(y)
    if defect == "truncate":
        return (y.view(torch.int32) & -65536).view(torch.float32).to(BF)
    return y.to(BF)
