// The head of the tagger step (models/encoders/tagger.py, trains/tagger.py:161-176) around the Linear layer, which stays
// on the GEMM:
//     pooled = AdaptiveAvgPool2d(1)(x).float().flatten(1)           tag_pool_fwd  (the dropout keep mask rides on it)
//     probs  = Sigmoid()(Linear(Dropout(pooled)))                    bce_fwd
//     loss   = BCELoss()(probs, targets); acc = binary_accuracy      bce_fwd + its finalize
// and their backward (bce_bwd writes d logits, tag_pool_bwd broadcasts d pooled over the map in the map's own dtype).
// The loss is the reference's function of the ROUNDED fp32 probability, quirks included: both logarithms are clamped
// at -100 BEFORE they meet t or 1 - t (0 * -inf would be NaN), and the gradient is BCELoss's (p - t) / max(p(1-p), 1e-12)
// times the sigmoid's p(1-p) -- exactly 0 where p saturated to 0 or 1, not the p - t of the logits form.
// tagloss_fwd / tagloss_bwd put the weighted, focal and asymmetric terms ON THE LOGITS in the place of the BCE pair
// (include/scnattn.h: "Tagger losses for rare tags"): the same decomposition, probabilities and count, another term.
// All are bound by HBM or by their launch: the pool reads the map once (16.8 MB at B=32, 8x8, C=2048, half of that
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

// ---- the weighted / focal / asymmetric family on the logits (include/scnattn.h: "Tagger losses for rare tags") ----------------
// FORM is uniform per launch and picked on the host: 0 both gammas 0 and no margin (BCE with logits, weighted), 1 a gamma,
// no margin (focal), 2 a margin (asymmetric).  HASW: pos_weight is given.  No branch on the options inside the element loop
// but gamma_neg == 0 under a margin, which is uniform over the launch (0^0 := 1).
struct TagLossOpt { float gp, gn, m; };

// sp(z) = -log(1 - p), sp(-z) = -log p, p and q = 1 - p from one expf, one log1pf and one division; q is never a difference.
// The three element functions round every operation once (no contraction into fma): they evaluate the header's expressions
// as a plain fp32 evaluation does, which is what their per-element test measures them against.
struct LogitParts { float spz, spn, p, q; };
__device__ __forceinline__ LogitParts logit_parts(float z) {
#pragma clang fp contract(off)
    const float e = expf(-fabsf(z)), l = log1pf(e), r = 1.f / (1.f + e);
    const bool pos = z >= 0.f;
    return {fmaxf(z, 0.f) + l, fmaxf(-z, 0.f) + l, pos ? r : e * r, pos ? e * r : r};
}

// p: the stored probability sigmoidf_(z), which the margin is taken from
template <int FORM>
__device__ __forceinline__ float tagloss_term(float z, float p, float t, float w, const TagLossOpt o) {
#pragma clang fp contract(off)
    const LogitParts a = logit_parts(z);
    float lp = a.spn, ln = a.spz;
    if (FORM != 0) lp *= expf(-o.gp * a.spz);
    if (FORM == 1) ln *= expf(-o.gn * a.spn);
    if (FORM == 2) {
        const float pm = fmaxf(p - o.m, 0.f);
        const float pw = o.gn == 0.f ? 1.f : (pm > 0.f ? expf((o.gn - 1.f) * logf(pm)) * pm : 0.f);
        ln = pw * -log1pf(-pm);
    }
    return t * w * lp + (1.f - t) * ln;
}

template <int FORM>
__device__ __forceinline__ float tagloss_grad(float z, float t, float w, const TagLossOpt o, float scale) {
#pragma clang fp contract(off)
    const LogitParts a = logit_parts(z);
    float dp = -a.q, dn = a.p;
    if (FORM != 0) dp = -expf(-o.gp * a.spz) * (o.gp * a.p * a.spn + a.q);
    if (FORM == 1) dn = expf(-o.gn * a.spn) * (o.gn * a.q * a.spz + a.p);
    if (FORM == 2) {
        const float p = sigmoidf_(z), pm = p - o.m;
        dn = 0.f;
        if (pm > 0.f) {
            float pw1 = 0.f, pw = 1.f;          // p_m^(gamma - 1) and p_m^gamma; gamma_neg is 0 or >= 1 here
            if (o.gn != 0.f) { pw1 = expf((o.gn - 1.f) * logf(pm)); pw = pw1 * pm; }
            dn = (o.gn * pw1 * -log1pf(-pm) + pw / (1.f - pm)) * p * a.q;
        }
    }
    return scale * (t * w * dp + (1.f - t) * dn);
}

// bce_fwd_kernel's decomposition, probabilities and count; the term alone differs
template <bool VEC, bool HASW, int FORM>
__global__ __launch_bounds__(256) void tagloss_fwd_kernel(int S, const float* __restrict__ z, long ldz, const float* __restrict__ t,
                                                          long ldt, const float* __restrict__ w, TagLossOpt o,
                                                          float* __restrict__ probs, long ldp, float* __restrict__ row_sum,
                                                          float* __restrict__ row_agree) {
    const int b = blockIdx.x;
    const float* zr = z + (long)b * ldz;
    const float* tr = t + (long)b * ldt;
    float* pr = probs + (long)b * ldp;
    float acc = 0.f;
    int n = 0;
    if (VEC) {
        for (int s = threadIdx.x * 4; s < S; s += 1024) {
            const f32x4 zv = ld4(zr + s), tv = ld4(tr + s);
            f32x4 wv = {1.f, 1.f, 1.f, 1.f};
            if (HASW) wv = ld4(w + s);
            f32x4 pv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pv[j] = sigmoidf_(zv[j]);
                acc += tagloss_term<FORM>(zv[j], pv[j], tv[j], wv[j], o);
                n += (pv[j] >= 0.5f) == (tv[j] >= 0.5f) ? 1 : 0;
            }
            *reinterpret_cast<f32x4*>(pr + s) = pv;
        }
    } else {
        for (int s = threadIdx.x; s < S; s += 256) {
            const float zz = zr[s], p = sigmoidf_(zz), tt = tr[s];
            pr[s] = p;
            acc += tagloss_term<FORM>(zz, p, tt, HASW ? w[s] : 1.f, o);
            n += (p >= 0.5f) == (tt >= 0.5f) ? 1 : 0;
        }
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int o_ = 32; o_ > 0; o_ >>= 1) n += __shfl_xor(n, o_, 64);
    __shared__ float pa[4];
    __shared__ int pn[4];
    if ((threadIdx.x & 63) == 0) { pa[threadIdx.x >> 6] = acc; pn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        row_sum[b] = (pa[0] + pa[1]) + (pa[2] + pa[3]);
        row_agree[b] = (float)((pn[0] + pn[1]) + (pn[2] + pn[3]));
    }
}

template <bool VEC, bool HASW, int FORM>
__global__ __launch_bounds__(256) void tagloss_bwd_kernel(int S, const float* __restrict__ z, long ldz, const float* __restrict__ t,
                                                          long ldt, const float* __restrict__ w, TagLossOpt o,
                                                          const float* __restrict__ g, float count, float* __restrict__ dz,
                                                          long lddz) {
    const int b = blockIdx.x;
    const float* zr = z + (long)b * ldz;
    const float* tr = t + (long)b * ldt;
    float* dr = dz + (long)b * lddz;
    const float scale = g[0] / count;
    if (VEC) {
        for (int s = threadIdx.x * 4; s < S; s += 1024) {
            const f32x4 zv = ld4(zr + s), tv = ld4(tr + s);
            f32x4 wv = {1.f, 1.f, 1.f, 1.f};
            if (HASW) wv = ld4(w + s);
            f32x4 d;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = tagloss_grad<FORM>(zv[j], tv[j], wv[j], o, scale);
            *reinterpret_cast<f32x4*>(dr + s) = d;
        }
    } else {
        for (int s = threadIdx.x; s < S; s += 256) dr[s] = tagloss_grad<FORM>(zr[s], tr[s], HASW ? w[s] : 1.f, o, scale);
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

// the refusals of the options (the comparisons are false for a NaN) and the kernel form they select
static int tagloss_form(const scnattn_tag_loss_options* o, TagLossOpt& k) {
    SCN_ARG(o, "tagloss: the options are NULL");
    SCN_ARG(o->gamma_pos >= 0.f && o->gamma_pos <= 16.f && o->gamma_neg >= 0.f && o->gamma_neg <= 16.f,
            "tagloss: gamma_pos and gamma_neg must be finite and in [0, 16]");
    SCN_ARG(o->margin >= 0.f && o->margin < 1.f, "tagloss: the margin must be in [0, 1)");
    SCN_ARG(!(o->margin > 0.f && o->gamma_neg > 0.f && o->gamma_neg < 1.f),
            "tagloss: a margin with 0 < gamma_neg < 1 has an unbounded gradient at p -> margin");
    k = TagLossOpt{o->gamma_pos, o->gamma_neg, o->margin};
    return o->margin > 0.f ? 2 : (o->gamma_pos != 0.f || o->gamma_neg != 0.f) ? 1 : 0;
}

#define SCN_TAGLOSS_FORMS(KERNEL, VEC, HASW, ...)                                                                          \
    do {                                                                                                                  \
        if (form == 0) hipLaunchKernelGGL((KERNEL<VEC, HASW, 0>), dim3(B), dim3(256), 0, st, __VA_ARGS__);                \
        else if (form == 1) hipLaunchKernelGGL((KERNEL<VEC, HASW, 1>), dim3(B), dim3(256), 0, st, __VA_ARGS__);           \
        else hipLaunchKernelGGL((KERNEL<VEC, HASW, 2>), dim3(B), dim3(256), 0, st, __VA_ARGS__);                          \
    } while (0)
#define SCN_TAGLOSS_LAUNCH(KERNEL, ...)                                                                                    \
    do {                                                                                                                  \
        if (vec && w) SCN_TAGLOSS_FORMS(KERNEL, true, true, __VA_ARGS__);                                                 \
        else if (vec) SCN_TAGLOSS_FORMS(KERNEL, true, false, __VA_ARGS__);                                                \
        else if (w) SCN_TAGLOSS_FORMS(KERNEL, false, true, __VA_ARGS__);                                                  \
        else SCN_TAGLOSS_FORMS(KERNEL, false, false, __VA_ARGS__);                                                        \
    } while (0)

int tagloss_fwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, const float* w,
                const scnattn_tag_loss_options* opt, float* probs, long ldp, float* rows, float* out) {
    SCN_ARG(B > 0 && S > 0, "tagloss_fwd: bad shape");
    SCN_ARG((long)B * S <= (1L << 24), "tagloss_fwd: B*S above 2^24 (the agreement count is kept as a float)");
    SCN_ARG(z && t && probs && rows && out, "tagloss_fwd: null argument");
    SCN_ARG(ldz >= S && ldt >= S && ldp >= S, "tagloss_fwd: leading dimension below the width");
    TagLossOpt k;
    const int form = tagloss_form(opt, k);
    if (form < 0) return -1;
    const bool vec = S % 4 == 0 && rows16(z, ldz) && rows16(t, ldt) && rows16(probs, ldp) && (!w || aligned16(w));
    SCN_TAGLOSS_LAUNCH(tagloss_fwd_kernel, S, z, ldz, t, ldt, w, k, probs, ldp, rows, rows + B);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, st, B, rows, rows + B, (float)((long)B * S), out);
    SCN_LAUNCH_CHECK();
    return 0;
}

int tagloss_bwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, const float* w,
                const scnattn_tag_loss_options* opt, const float* g, float* dz, long lddz) {
    SCN_ARG(B > 0 && S > 0, "tagloss_bwd: bad shape");
    SCN_ARG((long)B * S <= (1L << 24), "tagloss_bwd: B*S above 2^24");
    SCN_ARG(z && t && g && dz, "tagloss_bwd: null argument");
    SCN_ARG(ldz >= S && ldt >= S && lddz >= S, "tagloss_bwd: leading dimension below the width");
    TagLossOpt k;
    const int form = tagloss_form(opt, k);
    if (form < 0) return -1;
    const bool vec = S % 4 == 0 && rows16(z, ldz) && rows16(t, ldt) && rows16(dz, lddz) && (!w || aligned16(w));
    const float count = (float)((long)B * S);
    SCN_TAGLOSS_LAUNCH(tagloss_bwd_kernel, S, z, ldz, t, ldt, w, k, g, count, dz, lddz);
    SCN_LAUNCH_CHECK();
    return 0;
}
#undef SCN_TAGLOSS_LAUNCH
#undef SCN_TAGLOSS_FORMS

}  // namespace scn
