// The head of the tagger step (models/encoders/tagger.py, trains/tagger.py:161-176) around the Linear layer, which stays
// on the GEMM:
//     pooled = AdaptiveAvgPool2d(1)(x).float().flatten(1)           tag_pool_fwd  (the dropout keep mask rides on it)
//     probs  = Sigmoid()(Linear(Dropout(pooled)))                    bce_fwd
//     loss   = BCELoss()(probs, targets); acc = binary_accuracy      bce_fwd + its finalize
// and their backward (bce_bwd writes d logits, tag_pool_bwd broadcasts d pooled over the map in the map's own dtype).
// The loss is the reference's function of the ROUNDED fp32 probability, quirks included: both logarithms are clamped
// at -100 BEFORE they meet t or 1 - t (0 * -inf would be NaN), and the gradient is BCELoss's (p - t) / max(p(1-p), 1e-12)
// times the sigmoid's p(1-p) -- exactly 0 where p saturated to 0 or 1, not the p - t of the logits form.
// All four are bound by HBM or by their launch: the pool reads the map once (16.8 MB at B=32, 8x8, C=2048, half of that
// in bf16), one workgroup per image and 256 columns (256 workgroups there), whose pixel groups meet once in LDS in group
// order.  Every sum has a fixed order; no atomics.
// bf16 == 2 (tag_pool_fwd): the mean of a bf16 map is rounded to bf16 (nearest even) before the mask, as
// nn.AdaptiveAvgPool2d on a bf16 map returns it -- what EncoderTagger.forward computes under bf16 autocast, so that the
// fused step trains the function that forward() evaluates.  The stored value stays fp32.
#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

template <typename T, int VEC>
__device__ __forceinline__ void load_cols(const T* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = ld1(p);
    } else if constexpr (sizeof(T) == 4) {             // 4 fp32 columns: one 16-byte load
        const f32x4 q = ld4(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q[j];
    } else {                                            // 8 bf16 columns: one 16-byte load
        const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __builtin_bit_cast(float, u[j] << 16);
            v[2 * j + 1] = __builtin_bit_cast(float, u[j] & 0xffff0000u);
        }
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void store_cols(T* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        if constexpr (sizeof(T) == 4) *p = v[0];
        else *p = (bf16_t)(pack2(v[0], 0.f) & 0xffffu);
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        *reinterpret_cast<u32x4*>(p) = u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    }
}

// One workgroup = image blockIdx.y x COLS = LPR * VEC columns; LPR lanes cover a pixel row of them, the 256 / LPR pixel
// groups take every NPG-th pixel, four rows in flight per lane, and meet in LDS in group order.
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(256) void tag_pool_fwd_kernel(int HW, int C, const T* __restrict__ x, long sb, long sp, long sc,
                                                           const float* __restrict__ ks, long ldk,
                                                           float* __restrict__ out, long ldo, int round16) {
    constexpr int NPG = 256 / LPR, COLS = LPR * VEC;
    __shared__ __attribute__((aligned(16))) float part[NPG][COLS];
    const int b = blockIdx.y, pg = threadIdx.x / LPR, lc = (threadIdx.x % LPR) * VEC;
    const int c0 = blockIdx.x * COLS + lc;
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (c0 < C) {                                       // VEC > 1: C is a multiple of VEC, so c0 + VEC <= C
        const T* xp = x + (long)b * sb + (long)c0 * sc;
        int q = pg;
        for (; q + 3 * NPG < HW; q += 4 * NPG) {
            float v[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) load_cols<T, VEC>(xp + (long)(q + u * NPG) * sp, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] += v[u][j];
        }
        for (; q < HW; q += NPG) {
            float v[VEC];
            load_cols<T, VEC>(xp + (long)q * sp, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) part[pg][lc + j] = acc[j];
    __syncthreads();
    const int c = blockIdx.x * COLS + threadIdx.x;
    if (threadIdx.x < COLS && c < C) {
        float s = part[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < NPG; ++g) s += part[g][threadIdx.x];
        s = s / (float)HW;
        if (round16) s = bf16_to_f32(pack2(s, 0.f) & 0xffffu);      // the mean as a bf16 pool hands it on, before the mask
        if (ks) s *= ks[(long)b * ldk + c];
        out[(long)b * ldo + c] = s;
    }
}

// dx[b][q][c] = dpooled[b][c] * ks[b][c] / HW for every pixel q, same decomposition
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(256) void tag_pool_bwd_kernel(int HW, int C, const float* __restrict__ dp, long ldd,
                                                           const float* __restrict__ ks, long ldk, T* __restrict__ dx,
                                                           long sb, long sp, long sc) {
    constexpr int NPG = 256 / LPR, COLS = LPR * VEC;
    const int b = blockIdx.y, pg = threadIdx.x / LPR;
    const int c0 = blockIdx.x * COLS + (threadIdx.x % LPR) * VEC;
    if (c0 >= C) return;
    float v[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        float g = dp[(long)b * ldd + c0 + j];
        if (ks) g *= ks[(long)b * ldk + c0 + j];
        v[j] = g / (float)HW;
    }
    T* o = dx + (long)b * sb + (long)c0 * sc;
    for (int q = pg; q < HW; q += NPG) store_cols<T, VEC>(o + (long)q * sp, v);
}

// the reference's term at the rounded probability: clamp first, multiply second
__device__ __forceinline__ float bce_term(float p, float t) {
    const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
    return -(t * lp + (1.f - t) * lq);
}

// one workgroup per row: probs, the row's sum of terms and its count of (p >= 0.5) == (t >= 0.5)
template <bool VEC>
__global__ __launch_bounds__(256) void bce_fwd_kernel(int S, const float* __restrict__ z, long ldz, const float* __restrict__ t,
                                                      long ldt, float* __restrict__ probs, long ldp,
                                                      float* __restrict__ row_sum, float* __restrict__ row_agree) {
    const int b = blockIdx.x;
    const float* zr = z + (long)b * ldz;
    const float* tr = t + (long)b * ldt;
    float* pr = probs + (long)b * ldp;
    float acc = 0.f;
    int n = 0;
    if (VEC) {
        for (int s = threadIdx.x * 4; s < S; s += 1024) {
            const f32x4 zv = ld4(zr + s), tv = ld4(tr + s);
            f32x4 pv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pv[j] = sigmoidf_(zv[j]);
                acc += bce_term(pv[j], tv[j]);
                n += (pv[j] >= 0.5f) == (tv[j] >= 0.5f) ? 1 : 0;
            }
            *reinterpret_cast<f32x4*>(pr + s) = pv;
        }
    } else {
        for (int s = threadIdx.x; s < S; s += 256) {
            const float p = sigmoidf_(zr[s]), tt = tr[s];
            pr[s] = p;
            acc += bce_term(p, tt);
            n += (p >= 0.5f) == (tt >= 0.5f) ? 1 : 0;
        }
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __shared__ float pa[4];
    __shared__ int pn[4];
    if ((threadIdx.x & 63) == 0) { pa[threadIdx.x >> 6] = acc; pn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        row_sum[b] = (pa[0] + pa[1]) + (pa[2] + pa[3]);
        row_agree[b] = (float)((pn[0] + pn[1]) + (pn[2] + pn[3]));       // <= S <= 2^24: exact
    }
}

// out[0] = sum(row_sum) / (B*S), out[1] = sum(row_agree) (integers below 2^24: exact in any order); one workgroup
__global__ __launch_bounds__(256) void bce_finalize_kernel(int B, const float* __restrict__ row_sum,
                                                           const float* __restrict__ row_agree, float count,
                                                           float* __restrict__ out) {
    float a = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) { a += row_sum[i]; c += row_agree[i]; }
    a = wave_sum(a);
    c = wave_sum(c);
    __shared__ float pa[4], pc[4];
    if ((threadIdx.x & 63) == 0) { pa[threadIdx.x >> 6] = a; pc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = ((pa[0] + pa[1]) + (pa[2] + pa[3])) / count;
        out[1] = (pc[0] + pc[1]) + (pc[2] + pc[3]);
    }
}

// d loss / d logit from the stored probability: BCELoss's backward times the sigmoid's
__device__ __forceinline__ float bce_grad(float p, float t, float scale) {
    const float q = p * (1.f - p);
    return scale * (p - t) * (q / fmaxf(q, 1e-12f));
}

template <bool VEC>
__global__ __launch_bounds__(256) void bce_bwd_kernel(int S, const float* __restrict__ probs, long ldp,
                                                      const float* __restrict__ t, long ldt, const float* __restrict__ g,
                                                      float count, float* __restrict__ dz, long lddz) {
    const int b = blockIdx.x;
    const float* pr = probs + (long)b * ldp;
    const float* tr = t + (long)b * ldt;
    float* dr = dz + (long)b * lddz;
    const float scale = g[0] / count;
    if (VEC) {
        for (int s = threadIdx.x * 4; s < S; s += 1024) {
            const f32x4 pv = ld4(pr + s), tv = ld4(tr + s);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = bce_grad(pv[j], tv[j], scale);
            *reinterpret_cast<f32x4*>(dr + s) = o;
        }
    } else {
        for (int s = threadIdx.x; s < S; s += 256) dr[s] = bce_grad(pr[s], tr[s], scale);
    }
}

inline bool rows16(const void* p, long ld) { return aligned16(p) && ld % 4 == 0; }

template <typename T>
bool pool_vec_ok(const void* x, int C, long sb, long sp, long sc) {
    constexpr int V = 16 / (int)sizeof(T);
    return sc == 1 && C % V == 0 && sp % V == 0 && sb % V == 0 && aligned16(x);
}

}  // namespace

int tag_pool_fwd(hipStream_t st, int B, int HW, int C, const void* x, int bf16, long sb, long sp, long sc, const float* ks,
                 long ldk, float* out, long ldo) {
    SCN_ARG(B > 0 && B <= 65535 && HW > 0 && C > 0, "tag_pool_fwd: bad shape (B in [1, 65535], HW > 0, C > 0)");
    SCN_ARG(x && out, "tag_pool_fwd: null map or output");
    SCN_ARG(bf16 >= 0 && bf16 <= 2, "tag_pool_fwd: bf16 must be 0 (fp32 map), 1 (bf16 map) or 2 (bf16 map, bf16-rounded mean)");
    SCN_ARG(sb >= 0 && sp >= 0 && sc >= 0, "tag_pool_fwd: negative stride");
    SCN_ARG(ldo >= C && (!ks || ldk >= C), "tag_pool_fwd: leading dimension below the width");
#define SCN_TAG_FWD(T, VEC, LPR)                                                                                          \
    hipLaunchKernelGGL((tag_pool_fwd_kernel<T, VEC, LPR>), dim3(cdiv(C, VEC * LPR), B), dim3(256), 0, st, HW, C,          \
                       reinterpret_cast<const T*>(x), sb, sp, sc, ks, ldk, out, ldo, bf16 == 2 ? 1 : 0)
    if (bf16) {
        if (pool_vec_ok<bf16_t>(x, C, sb, sp, sc)) SCN_TAG_FWD(bf16_t, 8, 32);
        else SCN_TAG_FWD(bf16_t, 1, 64);
    } else {
        if (pool_vec_ok<float>(x, C, sb, sp, sc)) SCN_TAG_FWD(float, 4, 64);
        else SCN_TAG_FWD(float, 1, 64);
    }
#undef SCN_TAG_FWD
    SCN_LAUNCH_CHECK();
    return 0;
}

int tag_pool_bwd(hipStream_t st, int B, int HW, int C, const float* dpooled, long ldd, const float* ks, long ldk, void* dx,
                 int bf16, long sb, long sp, long sc) {
    SCN_ARG(B > 0 && B <= 65535 && HW > 0 && C > 0, "tag_pool_bwd: bad shape (B in [1, 65535], HW > 0, C > 0)");
    SCN_ARG(dpooled && dx, "tag_pool_bwd: null gradient or map");
    SCN_ARG(sc > 0 && (sp > 0 || HW == 1) && (sb > 0 || B == 1), "tag_pool_bwd: the map's elements must be distinct");
    SCN_ARG(ldd >= C && (!ks || ldk >= C), "tag_pool_bwd: leading dimension below the width");
#define SCN_TAG_BWD(T, VEC, LPR)                                                                                          \
    hipLaunchKernelGGL((tag_pool_bwd_kernel<T, VEC, LPR>), dim3(cdiv(C, VEC * LPR), B), dim3(256), 0, st, HW, C, dpooled, \
                       ldd, ks, ldk, reinterpret_cast<T*>(dx), sb, sp, sc)
    if (bf16) {
        if (pool_vec_ok<bf16_t>(dx, C, sb, sp, sc)) SCN_TAG_BWD(bf16_t, 8, 32);
        else SCN_TAG_BWD(bf16_t, 1, 64);
    } else {
        if (pool_vec_ok<float>(dx, C, sb, sp, sc)) SCN_TAG_BWD(float, 4, 64);
        else SCN_TAG_BWD(float, 1, 64);
    }
#undef SCN_TAG_BWD
    SCN_LAUNCH_CHECK();
    return 0;
}

int bce_fwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, float* probs, long ldp,
            float* rows, float* out) {
    SCN_ARG(B > 0 && S > 0, "bce_fwd: bad shape");
    SCN_ARG((long)B * S <= (1L << 24), "bce_fwd: B*S above 2^24 (the agreement count is kept as a float)");
    SCN_ARG(z && t && probs && rows && out, "bce_fwd: null argument");
    SCN_ARG(ldz >= S && ldt >= S && ldp >= S, "bce_fwd: leading dimension below the width");
    const bool vec = S % 4 == 0 && rows16(z, ldz) && rows16(t, ldt) && rows16(probs, ldp);
    if (vec) hipLaunchKernelGGL(bce_fwd_kernel<true>, dim3(B), dim3(256), 0, st, S, z, ldz, t, ldt, probs, ldp, rows, rows + B);
    else     hipLaunchKernelGGL(bce_fwd_kernel<false>, dim3(B), dim3(256), 0, st, S, z, ldz, t, ldt, probs, ldp, rows, rows + B);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, st, B, rows, rows + B, (float)((long)B * S), out);
    SCN_LAUNCH_CHECK();
    return 0;
}

int bce_bwd(hipStream_t st, int B, int S, const float* probs, long ldp, const float* t, long ldt, const float* g, float* dz,
            long lddz) {
    SCN_ARG(B > 0 && S > 0, "bce_bwd: bad shape");
    SCN_ARG((long)B * S <= (1L << 24), "bce_bwd: B*S above 2^24");
    SCN_ARG(probs && t && g && dz, "bce_bwd: null argument");
    SCN_ARG(ldp >= S && ldt >= S && lddz >= S, "bce_bwd: leading dimension below the width");
    const bool vec = S % 4 == 0 && rows16(probs, ldp) && rows16(t, ldt) && rows16(dz, lddz);
    const float count = (float)((long)B * S);
    if (vec) hipLaunchKernelGGL(bce_bwd_kernel<true>, dim3(B), dim3(256), 0, st, S, probs, ldp, t, ldt, g, count, dz, lddz);
    else     hipLaunchKernelGGL(bce_bwd_kernel<false>, dim3(B), dim3(256), 0, st, S, probs, ldp, t, ldt, g, count, dz, lddz);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace scn
