"""Plain-torch references of the three GEMM families of the C ABI (include/scnattn.h:163-193 and :307-313): the dense product
with its epilogue (scnattn_sgemm / _sgemm_ws / _cgemm) and the skinny product with its K-slice slabs (scnattn_skinny_gemm,
_bf16w, _bf16).

Written from the header comments, not from the kernels.  Like tests/decoder_kernel_refs.py every function computes in the
dtype of its operands: called with fp64 tensors it is the reference, called with fp32 tensors it is "the same product
evaluated by torch on the CPU in fp32".  For every result `x` the dict carries `x_abs`, the sum of the absolute values of
the terms of each element, and `x_n`, their number: what kernel_harness._sum_ok judges with
|got - ref| <= (n + 8) * 2^-24 * S per element.
"""
import torch

from scnattn import _lib as L


def cdiv(a, b):
    return -(-a // b)


def bf16_round(x):
    """fp32 -> bf16 (torch: round to nearest even) -> widened exactly, in the dtype of x"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def bf16_bits(x):
    """the raw 16-bit elements of the bf16 copy of x (what scnattn_f32_to_bf16 writes)"""
    return x.to(torch.float32).to(torch.bfloat16).view(torch.int16)


# ---- dense --------------------------------------------------------------------------------------------------------------
def gemm(a, b, ta=False, tb=False, alpha=1.0, beta=0.0, c0=None, bias=None, rowmask=None):
    """C[z] = alpha * op(A[z]) . op(B[z]) + beta * C0[z] + bias[n]; rows with rowmask[m] == 0 are 0.
    a [batch, M, K] ([batch, K, M] with ta), b [batch, K, N] ([batch, N, K] with tb), c0 [batch, M, N] (read only when
    beta != 0; may hold NaN in masked rows), bias [N], rowmask [M]; 2-d operands are one batch.
    Terms of an element: the K products alpha*a*b, beta*c0 and bias -> n = K + one per optional term present."""
    squeeze = a.dim() == 2
    if squeeze:
        a, b, c0 = a.unsqueeze(0), b.unsqueeze(0), (None if c0 is None else c0.unsqueeze(0))
    A = a.transpose(1, 2) if ta else a
    B = b.transpose(1, 2) if tb else b
    K = A.shape[2]
    c = alpha * torch.matmul(A, B)
    c_abs = abs(alpha) * torch.matmul(A.abs(), B.abs())
    n = K
    if beta != 0.0:
        c, c_abs, n = c + beta * c0, c_abs + (beta * c0).abs(), n + 1
    if bias is not None:
        c, c_abs, n = c + bias, c_abs + bias.abs(), n + 1
    if rowmask is not None:
        keep = (rowmask != 0).reshape(1, -1, 1)
        zero = torch.zeros((), dtype=c.dtype)
        c, c_abs = torch.where(keep, c, zero), torch.where(keep, c_abs, zero)      # where, not *: C0 may be NaN there
    if squeeze:
        c, c_abs = c[0], c_abs[0]
    return {"c": c, "c_abs": c_abs, "c_n": n}


# ---- instance names, rendered from the launch plan of the real call (scnattn_plan_next) -------------------------------
def skinny_name(p):
    """"nb<NB> c<chunks> v<XVEC> e<empty slices> z<grid.z>" of a skinny plan"""
    assert p.family == L.PLAN_SKINNY and (p.wbf != 2 or p.nb % 2 == 0)
    return "nb%d c%d v%d e%d z%d" % (p.nb, p.chunks, p.vec, p.empty, p.grid_z)


def dense_name(p):
    """"sgemm v<VEC> S<S>" or "cgemm mi<mi> S<S> <-|comb|red> <vst|sst>" of a plain dense product's plan"""
    if p.family == L.PLAN_SGEMM:
        assert (p.second == L.SECOND_SPLITK_REDUCE) == (p.S > 1)
        return "sgemm v%d S%d" % (p.vec, p.S)
    assert p.family == L.PLAN_CGEMM and (p.pro, p.epi, p.gather, p.c3) == (0, 0, 0, 0)
    assert p.second in (L.SECOND_NONE, L.SECOND_CREDUCE)
    assert p.S == 1 or bool(p.in_launch) != bool(p.second)
    return "cgemm mi%d S%d %s %s" % (p.mi, p.S, "-" if p.S == 1 else "comb" if p.in_launch else "red", "vst" if p.vec else "sst")


# ---- skinny -------------------------------------------------------------------------------------------------------------
KW = 64     # KW of csrc/skinny.hip, k per wave per chunk


def skinny_blocking(K, ksplit, form):
    """skinny_plan of csrc/skinny.hip: k per wave `per` = ceil(ceil(K / ksplit) / 4) in whole 8-k blocks (whole 16-k blocks for the
    bf16 matrix instruction, form "bf16"), in whole 64-k chunks when above 64; kslice = 4 * per.
    -> (per, nb = 8-k blocks per wave per chunk, chunks, kslice)"""
    per = cdiv(cdiv(K, ksplit), 4)
    per = (per + 7) & ~7
    if form == "bf16":
        per = (per + 15) & ~15
    if per > KW:
        per = cdiv(per, KW) * KW
    nb = KW // 8 if per > KW else per // 8
    return per, nb, cdiv(per, KW), 4 * per


def skinny_slices(K, ksplit, form):
    """[(kbeg, kend)] per slab; a slice that starts past K is empty (kbeg == kend)"""
    kslice = skinny_blocking(K, ksplit, form)[3]
    return [(min(K, s * kslice), min(K, (s + 1) * kslice)) for s in range(ksplit)]


def skinny(X, W, slices):
    """X [rows, groups, K], W [groups, K, N] -> Y[s][g][r][n] = sum over k in slice s of X[r][g][k] * W[g][k][n].
    `y_n` is a list (slice lengths); `sum` is the all-slab sum (n = K)."""
    y, y_abs = [], []
    for kb, ke in slices:
        xs, ws = X[:, :, kb:ke], W[:, kb:ke]
        y.append(torch.einsum("rgk,gkn->grn", xs, ws))
        y_abs.append(torch.einsum("rgk,gkn->grn", xs.abs(), ws.abs()))
    y, y_abs = torch.stack(y), torch.stack(y_abs)
    return {"y": y, "y_abs": y_abs, "y_n": [ke - kb for kb, ke in slices],
            "sum": y.sum(0), "sum_abs": y_abs.sum(0), "sum_n": X.shape[2]}


def slab(ref, s):
    """slab s of a skinny() result in the dict shape _sum_ok consumes"""
    return {"y": ref["y"][s], "y_abs": ref["y_abs"][s], "y_n": ref["y_n"][s]}


def slab_sum_f32(Y):
    """the consumer's sum: slabs added one after the other, in slab order, in the dtype of Y"""
    acc = Y[0].clone()
    for s in range(1, Y.shape[0]):
        acc += Y[s]
    return acc


def skinny_operands(X, W, form):
    """the operands the kernel multiplies: "bf16w" reads W as bf16, "bf16" rounds X as well (products of two bf16 numbers
    are exact in fp32, so the same bound holds)"""
    if form != "f32":
        W = bf16_round(W)
    if form == "bf16":
        X = bf16_round(X)
    return X, W
