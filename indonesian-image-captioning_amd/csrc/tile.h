// Tile machinery shared by the trunk's convolution kernels and their bf16 twins, and the BatchNorm expressions they share
// with csrc/batchnorm.hip (internal; gfx950 only):
// csrc/cgemm.hip + csrc/cgemm16.hip (GEMM / implicit 3x3) and csrc/conv3.hip + csrc/wgrad16.hip (wave-split weight
// gradients).  Everything here is force-inlined into its caller: block order, convolution geometry, the BatchNorm
// forward / backward expressions and ReLU-mask term, the slab reducers' column-sum tail and the weight gradients' split policy, each written once.
#pragma once
#include "common.h"
#include "kernels.h"

namespace scn {

// ---- XCD-aware block order (speed only): hardware blocks b, b+8, b+16 ... share an XCD; give each XCD a contiguous run
// of `total` virtual ids, so that what neighbouring ids share (an activation panel, a K slice) is fetched into ONE L2 ------
__device__ __forceinline__ int xcd_order(int bid, int total) {
    const int q = total >> 3, r = total & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- convolution geometry --------------------------------------------------------------------------------------------
// The maps a product's rows live on: a member of the GEMM kernels' argument structs, filled from ConvExtra here.
struct ConvGeom {
    int Hi, Wi, Ho, Wo, s;        // row gather (strided 1x1 convolution); s == 0: none.  3x3: source / destination maps
    int c3c;                      // 3x3 modes: channels per tap of the gathered operand (Cin forward / wgrad, Cout dgrad)
    long src_rows;                // 3x3 modes: rows of the gathered map (N * Hi * Wi)
    int dHi, dWi;                 // mode 4: extent of the d-input map the rows are scattered into
};
static inline ConvGeom conv_geom(const ConvExtra& ex) {
    ConvGeom g{};
    g.Hi = ex.Hi; g.Wi = ex.Wi; g.Ho = ex.Ho; g.Wo = ex.Wo; g.s = (ex.stride > 1 || ex.c3) ? ex.stride : 0;
    g.c3c = ex.c3c; g.src_rows = ex.c3_src_rows;
    if (ex.c3 == 4) { g.Hi = ex.Ho; g.Wi = ex.Wo; g.dHi = ex.Hi; g.dWi = ex.Wi; }   // gathered map = dY (Ho x Wo)
    return g;
}

struct Pixel { int n, h, w; };
// row r of an [N][Ho][Wo] grid; Row: int, or long where the caller's row index is one
template <class Row> __device__ __forceinline__ Pixel pixel_of(Row r, int Ho, int Wo) {
    const int hw = Ho * Wo, n = (int)(r / hw), rem = (int)(r - (Row)n * hw), h = rem / Wo;
    return {n, h, rem - h * Wo};
}
// output row (n, ho, wo) of a strided 1x1 convolution -> input row (n, ho*s, wo*s)
__device__ __forceinline__ long gather_row(const ConvGeom& g, int r) {
    if (g.s == 0) return r;
    const Pixel p = pixel_of(r, g.Ho, g.Wo);
    return (long)p.n * g.Hi * g.Wi + (long)(p.h * g.s) * g.Wi + p.w * g.s;
}
// class row m = (n, ho', wo') of parity class (ph, pw) of the stride-2 d input -> d-input row (n, 2 ho' + ph, 2 wo' + pw)
__device__ __forceinline__ long class_row_scatter(const ConvGeom& g, int m, int ph, int pw) {
    const Pixel p = pixel_of(m, g.Ho, g.Wo);
    return ((long)p.n * g.dHi + 2 * p.h + ph) * g.dWi + 2 * p.w + pw;
}

// ---- BatchNorm pieces of csrc/batchnorm.hip and of the GEMM epilogues, each expression written once ----------------------
__device__ __forceinline__ float bn_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
// The forward expression.  Every ReLU mask that the backward pass recomputes from z is right only while it is THIS
// expression bit for bit, so the forward kernels and the masks all come through here.
__device__ __forceinline__ float bn_norm(float z, float mean, float invstd, float gamma, float beta) {
    return fmaf(bn_xhat(z, mean, invstd), gamma, beta);
}
// Eval mode (running statistics): the BatchNorm folded to y = fma(z, scale, shift), as EPI 3 of csrc/cgemm.hip forms it.
__device__ __forceinline__ void bn_eval_fold(float gamma, float beta, float mean, float var, float eps, float& scale, float& shift) {
    scale = gamma * (1.f / sqrtf(var + eps));
    shift = beta - mean * scale;
}
// ReLU mask of a BatchNorm recomputed from its pre-activation z: the function the forward pass evaluated was
// relu(bn_norm(z, ...)), or -- folded -- relu(fma(z, scale, shift)); (a, b) is that pair.  xhat is handed back for
// the g * xhat sum.  Not folded, this IS bn_norm(z, mean, invstd, a, b) > 0: the same fma of the same bn_xhat; it selects
// the operand and not the result, so that a run-time `folded` costs one fma.
__device__ __forceinline__ bool bn_relu_on(float z, float mean, float invstd, float a, float b, bool folded, float& xhat) {
    xhat = bn_xhat(z, mean, invstd);
    return fmaf(folded ? z : xhat, a, b) > 0.f;
}
// The backward expression (batch statistics): dz from the masked gradient g, dbeta = sum g, dgamma = sum g * xhat, 1 / R.
__device__ __forceinline__ float bn_dz(float g, float xhat, float gamma, float invstd, float dbeta, float dgamma, float inv_n) {
    return gamma * invstd * (g - dbeta * inv_n - xhat * dgamma * inv_n);
}

// Args: the kernel's argument struct (stat_partial, ldp, N).
// Tail of the 64 x 64 slab reducers (256 threads; thread (rl, cl) holds the sums of 4 columns over its 4 rows): the 16 row
// groups meet in LDS and are added in row-group order, one partial per (column, 64-row block blockIdx.y).
template <class Args>
__device__ __forceinline__ void slab_colsum_tail(const Args& g, float (&red)[16][2][64 + 1], const float (&s1)[4], const float (&s2)[4]) {
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        red[rl][0][cl * 4 + k] = s1[k];
        red[rl][1][cl * 4 + k] = s2[k];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int which = threadIdx.x >> 6, cc = threadIdx.x & 63;
        if (blockIdx.x * 64 + cc < g.N) {
            float t = red[0][which][cc];
#pragma unroll
            for (int i = 1; i < 16; ++i) t += red[i][which][cc];
            g.stat_partial[((long)which * g.N + blockIdx.x * 64 + cc) * g.ldp + blockIdx.y] = t;
        }
    }
}

// ---- wave-split weight gradients: the four waves of a workgroup own the SAME output block and split K ---------------------
// Workgroup-level K split of those kernels: aim for `target` workgroups over `ntiles` output blocks, at least 4 of the Q
// lines per wave, and no more slabs (mn floats each) than the workspace holds.  force_split > 0 replaces the aim; the
// caller checks that it survived the clamps.
static inline int wgrad_split(int ntiles, int Q, int target, long mn, bool ws, long ws_floats, int force_split) {
    int S = force_split > 0 ? force_split : (target + ntiles / 2) / ntiles;
    const int smax = Q / 16 > 0 ? Q / 16 : 1;
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    while (S > 1 && (!ws || (long)S * mn > ws_floats)) --S;
    return S;
}
// Their launch plan: Q lines of `seg` pixels, ntiles output blocks, S slabs of mn floats summed by cgemm_reduce when S > 1.
static inline LaunchPlan wgrad_plan(int family, int seg, int Q, int ntiles, int target, long mn, bool ws, long ws_floats,
                                    int force_split) {
    LaunchPlan p{};
    p.family = family; p.seg = seg; p.Q = Q; p.ntiles = ntiles; p.tiles = ntiles;
    p.S = wgrad_split(ntiles, Q, target, mn, ws, ws_floats, force_split);
    p.grid_x = ntiles * p.S; p.grid_y = p.grid_z = 1;
    if (p.S > 1) p.second = SCNATTN_SECOND_CGEMM_REDUCE;
    return p;
}

}  // namespace scn
