"""fp64 references, cases and judges of the tagger head kernels (csrc/taghead.hip: scnattn_tag_pool_fwd / _bwd, scnattn_bce_fwd /
_bwd) and of the whole head (scnattn.functional.tag_head_loss), shared by tests/test_taghead_refs.py (CPU: the references
against torch's own fp64 ops, the judges against torch's CPU fp32 evaluation and against planted defects) and
tests/test_gpu_taghead_kernels.py (the kernels).  The references are index arithmetic, not the torch ops they are held to.

What is computed (the reference's nn.AdaptiveAvgPool2d(1) -> Dropout -> Linear -> Sigmoid -> nn.BCELoss, binary_accuracy):
    pooled[b][c] = (sum_q x[b,q,c]) / HW * ks[b][c]                       ks: pre-scaled keep mask (0 or 1/(1-p)), or none
    dx[b,q,c]    = dpooled[b][c] * ks[b][c] / HW
    p            = 1 / (1 + exp(-z))
    term         = -( t * max(log p, -100) + (1 - t) * max(log1p(-p), -100) )   at the ROUNDED fp32 p, clamp before multiply
    loss         = sum(term) / (B * S);  agree = #((p >= 0.5) == (t >= 0.5))
    dz           = g / (B * S) * (p - t) * p(1-p) / max(p(1-p), 1e-12)

Bounds (u = 2^-24):
    pooled   (HW + 8) u |ks| sum_q|x| / HW                any summation order of HW terms plus the division and the mask
             (bf16 = 2, the mean rounded to bf16 before the mask: b + 2^-8 (|ref| + b))
    dx       fp32 8 u |ref|;  bf16 b + 2^-8 (|ref| + b), b = 8 u |ref|      one round to nearest even on top of the fp32 value
    p        min(4 x worst element error of torch's CPU fp32 sigmoid on the case, 1e-4 x row max): a result behind expf
    row sum  (S + 8) u sum(|t log p| + |(1-t) log1p(-p)|) against the fp64 terms AT THE STORED p
    loss     (B + 8) u sum|row| / (B * S) against the fp64 mean of the stored row sums
    agree    exactly the count recomputed from the stored p
    dz       8 u |ref| at the stored p (g / n, p - t, p(1-p), the quotient and two products: six roundings)"""
import torch

from kernel_harness import U, _bound_ok, _note

BF = torch.bfloat16
F64 = torch.float64

POOL_SHAPES = ((1, 1, 4), (3, 4, 20), (2, 49, 264), (5, 64, 2048))          # (B, HW, C)
BCE_SHAPES = ((1, 1), (3, 37), (2, 1001), (32, 1000))                        # (B, S)
KEEP = 1.0 / 0.85                                                            # Dropout(0.15)'s scale
EPS = float(torch.tensor(1e-12, dtype=torch.float32))     # binary_cross_entropy_backward's EPSILON is the FLOAT 1e-12, in fp64 too


# ---- cases --------------------------------------------------------------------------------------------------------------
def gen_pool(B, HW, C, bf16, with_ks, seed=0):
    """x [B, HW, C] (bf16 maps are generated as bf16: the fp32 values are exactly representable), ks [B, C] of zeros and
    1/0.85 or None, dp [B, C]: all float32 tensors holding the values the kernels are given"""
    g = torch.Generator().manual_seed(1000 * seed + B * 131 + HW * 17 + C)
    x = torch.randn(B, HW, C, generator=g)
    if bf16:
        x = x.to(BF).float()
    ks = None
    if with_ks:
        ks = (torch.rand(B, C, generator=g) >= 0.15).float() * torch.tensor(KEEP, dtype=torch.float32)
        ks[0, 0] = 0.0
        ks[-1, -1] = KEEP
    dp = torch.randn(B, C, generator=g)
    return x, ks, dp


def gen_bce(B, S, seed=0):
    """z uniform in [-8, 8], t in {0, 1} with a tenth fractional; S >= 37: the planted elements of row 0 (`planted`)"""
    g = torch.Generator().manual_seed(2000 * seed + B * 7919 + S)
    z = (torch.rand(B, S, generator=g) * 16.0 - 8.0).float()
    t = (torch.rand(B, S, generator=g) >= 0.5).float()
    frac = torch.rand(B, S, generator=g) < 0.1
    t = torch.where(frac, torch.rand(B, S, generator=g), t).float()
    planted = {}
    if S >= 37:
        plan = (("half_eq", 0.0, 0.5), ("half_lt", 0.0, 0.49), ("sat1_t0", 120.0, 0.0), ("sat1_t1", 120.0, 1.0),
                ("sat0_t0", -120.0, 0.0), ("sat0_t1", -120.0, 1.0), ("tiny_t0", -30.0, 0.0), ("tiny_t1", -30.0, 1.0),
                ("frac", None, 0.3), ("half_t1a", 0.0, 1.0), ("half_t1b", 0.0, 1.0))      # two more at p = 0.5: a `>` on p, on
        # t or on both then moves the count (with the first two alone, `>` on p alone cancels: -1 and +1)
        for k, (name, zv, tv) in enumerate(plan):
            s = 1 + 3 * k                        # spread over the vector lanes
            if zv is not None:
                z[0, s] = zv
            t[0, s] = tv
            planted[name] = s
    return z, t, planted


# ---- fp64 references (index arithmetic) -----------------------------------------------------------------------------------
def pool_fwd_ref(x, ks):
    x = x.to(F64)
    B, HW, C = x.shape
    s, a = torch.zeros(B, C, dtype=F64), torch.zeros(B, C, dtype=F64)
    for q in range(HW):
        s += x[:, q, :]
        a += x[:, q, :].abs()
    k = torch.ones(B, C, dtype=F64) if ks is None else ks.to(F64)
    return dict(pooled=s / HW * k, pooled_abs=a / HW * k.abs(), pooled_n=HW)


def pool_bwd_ref(dp, ks, HW):
    dp = dp.to(F64)
    k = torch.ones_like(dp) if ks is None else ks.to(F64)
    row = dp * k / HW
    out = torch.empty(dp.shape[0], HW, dp.shape[1], dtype=F64)
    for q in range(HW):
        out[:, q, :] = row
    return out


def sigmoid_ref(z):
    return 1.0 / (1.0 + torch.exp(-z.to(F64)))


def bce_parts(p, t):
    """the two clamped products of the term at probability p (fp64 arithmetic on the values given)"""
    p, t = p.to(F64), t.to(F64)
    lp = torch.log(p).clamp_min(-100.0)
    lq = torch.log1p(-p).clamp_min(-100.0)
    return t * lp, (1.0 - t) * lq


def bce_fwd_ref(p, t):
    """rows, loss and agreement count of probabilities p (the fp64 sigmoid, or a kernel's stored fp32 p)"""
    a, b = bce_parts(p, t)
    terms = -(a + b)
    B, S = terms.shape
    rows, rows_abs = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
    for s in range(S):
        rows += terms[:, s]
        rows_abs += a[:, s].abs() + b[:, s].abs()
    agree = int(((p.to(F64) >= 0.5) == (t.to(F64) >= 0.5)).sum())
    return dict(terms=terms, rows=rows, rows_abs=rows_abs, loss=rows.sum() / (B * S), agree=agree)


def bce_bwd_ref(p, t, g):
    p, t = p.to(F64), t.to(F64)
    q = p * (1.0 - p)
    return float(g) / p.numel() * (p - t) * q / q.clamp_min(EPS)


def head_ref(x, ks, W, b, t):
    """the whole head in fp64 with its hand-written gradient: x [B, HW, C] -> probs, loss, agree, z, dx, dW, db"""
    x, W, b, t = x.to(F64), W.to(F64), b.to(F64), t.to(F64)
    B, HW, C = x.shape
    xd = pool_fwd_ref(x, ks)["pooled"]
    z = torch.zeros(B, W.shape[0], dtype=F64)
    for c in range(C):
        z += xd[:, c:c + 1] * W[:, c].unsqueeze(0)
    z += b
    p = sigmoid_ref(z)
    f = bce_fwd_ref(p, t)
    dz = bce_bwd_ref(p, t, 1.0)
    dW = torch.zeros_like(W)
    dxd = torch.zeros_like(xd)
    for i in range(B):
        dW += dz[i].unsqueeze(1) * xd[i].unsqueeze(0)
        dxd[i] = (dz[i].unsqueeze(1) * W).sum(0)
    return dict(z=z, probs=p, loss=f["loss"], agree=f["agree"], dx=pool_bwd_ref(dxd, ks, HW), dW=dW, db=dz.sum(0))


# ---- judges: each asserts per element and returns nothing; the worst err / bound goes to the harness's report -----------------
def judge_pool_fwd(kernel, got, x, ks, round16=False):
    """round16 (bf16 = 2 of scnattn_tag_pool_fwd): the mean is rounded to bf16 before the mask: one round to nearest even on
    top of the fp32 value, b + 2^-8 (|ref| + b), the form of the bf16 outputs in tests/conv16_refs.py"""
    r = pool_fwd_ref(x, ks)
    b = (r["pooled_n"] + 8) * U * r["pooled_abs"]
    _bound_ok(kernel, "pooled", got, r["pooled"], b + 2.0 ** -8 * (r["pooled"].abs() + b) if round16 else b)
    if round16 and ks is None:      # without a mask every stored mean is a bf16 value
        assert bool((got.float().contiguous().view(torch.int32) & 0xFFFF == 0).all()), "%s: a mean is not a bf16 value" % kernel


def judge_pool_bwd(kernel, got, dp, ks, HW, bf16):
    """got [B, HW, C] as float32 (a bf16 map widened); every pixel of an image must hold the same bits for a channel"""
    want = pool_bwd_ref(dp, ks, HW)
    b = 8 * U * want.abs()
    _bound_ok(kernel, "dx", got, want, b + 2.0 ** -8 * (want.abs() + b) if bf16 else b)
    g32 = got.float().contiguous().view(torch.int32)
    assert bool((g32 == g32[:, :1, :]).all()), "%s: the pixels of an image differ for a channel" % kernel


def sigmoid_yard(z):
    """worst element error of torch's CPU fp32 sigmoid on this case"""
    return float((torch.sigmoid(z.float()).to(F64) - sigmoid_ref(z)).abs().max())


def judge_probs(kernel, p, z, planted):
    want = sigmoid_ref(z)
    yard = sigmoid_yard(z)
    bar = torch.minimum(torch.full_like(want, 4.0 * yard), 1e-4 * want.abs().max(dim=1, keepdim=True)[0].expand_as(want))
    err = (p.to(F64) - want).abs()
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), (err > 0).to(F64) * 1e30).nan_to_num(1e30)
    print("%s probs: worst err/bar %.3f (CPU fp32 worst element error %.3e)" % (kernel, float(ratio.max()), yard))
    assert bool((err <= bar).all()), "%s probs: worst err/bar %.3f at %d" % (kernel, float(ratio.max()), int(ratio.argmax()))
    _note(kernel, "probs", float(ratio.max()), "1e-4", yard)
    for name, s in planted.items():
        if name.startswith("sat1"):
            assert float(p[0, s]) == 1.0, name
        if name.startswith("sat0"):
            assert float(p[0, s]) == 0.0, name
        if name.startswith("half"):
            assert float(p[0, s]) == 0.5, name
        if name.startswith("tiny"):
            assert 0.0 < float(p[0, s]) < 1e-12, name


def judge_rows(kernel, rows, p, t):
    """row sums against the fp64 terms at the stored p"""
    r = bce_fwd_ref(p, t)
    _bound_ok(kernel, "rows", rows, r["rows"], (p.shape[1] + 8) * U * r["rows_abs"])


def judge_loss(kernel, loss, rows, B, S):
    """out[0] against the fp64 mean of the stored row sums"""
    rows = rows.to(F64)
    _bound_ok(kernel, "loss", loss.reshape(1), (rows.sum() / (B * S)).reshape(1),
              ((B + 8) * U * rows.abs().sum() / (B * S)).reshape(1))


def judge_agree(kernel, agree, p, t):
    want = int(((p >= 0.5) == (t >= 0.5)).sum())
    assert float(agree) == float(want), "%s: agreement count %r, recomputed from the stored p %d" % (kernel, float(agree), want)
    _note(kernel, "agree", 0.0, "sum")


def judge_bce_bwd(kernel, dz, p, t, g, planted):
    want = bce_bwd_ref(p, t, g)
    _bound_ok(kernel, "dz", dz, want, 8 * U * want.abs())
    for name, s in planted.items():
        if name.startswith("sat"):
            assert float(dz[0, s]) == 0.0, name
        if name.startswith("tiny"):
            assert float(dz[0, s]) != 0.0 and abs(float(want[0, s])) < 0.2 * abs(float(g)) / p.numel(), name


# ---- torch's CPU fp32 evaluation of the same formulas (what the bounds must not exclude) ---------------------------------------
def cpu32_pool_fwd(x, ks, round16=False):
    y = x.float().sum(dim=1) / x.shape[1]
    if round16:
        y = y.to(BF).float()
    return y if ks is None else y * ks


def cpu32_pool_bwd(dp, ks, HW, bf16):
    row = (dp if ks is None else dp * ks) / HW
    out = row.unsqueeze(1).expand(-1, HW, -1).contiguous()
    return out.to(BF).float() if bf16 else out


def cpu32_bce_fwd(z, t):
    """p, row sums, loss, agreement count in torch CPU float32"""
    p = torch.sigmoid(z.float())
    terms = -(t * torch.log(p).clamp_min(-100.0) + (1.0 - t) * torch.log1p(-p).clamp_min(-100.0))
    rows = terms.sum(dim=1)
    agree = ((p >= 0.5) == (t >= 0.5)).float().sum()
    return p, rows, rows.sum() / terms.numel(), agree


def cpu32_bce_bwd(p, t, g):
    q = p * (1.0 - p)
    return (torch.tensor(g, dtype=torch.float32) / p.numel()) * (p - t) * (q / q.clamp_min(1e-12))
