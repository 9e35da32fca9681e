// The loss of the train step (trains/attention_scn.py:222-236) as five launches instead of ~130:
//     scores  = pack_padded_sequence(scores,  decode_lengths, batch_first=True).data
//     targets = pack_padded_sequence(targets, decode_lengths, batch_first=True).data
//     loss    = CrossEntropyLoss()(scores, targets)                       # mean over N = sum(decode_lengths) rows
//     loss   += alpha_c * ((1. - alphas.sum(dim=1)) ** 2).mean()          # mean over B x P
// Packing only selects the rows (b, t < decode_length[b]) of the (B, T, V) score tensor; the mean does not
// care about their order.  So the cross-entropy runs on the tensor where it lies (no packed copy, whose
// backward alone is 51 row-block copies + a 65 MB zero fill at B=32, T=51, V=10000), one workgroup per
// (b, t) row with an online softmax (one read pass), and the backward writes d scores in place of the
// unpack: (softmax - onehot) * g / N for decoded rows, 0 elsewhere -- the (B*T, V) matrix the fc GEMMs of
// scnattn_seq_bwd consume.  Sums are formed in a fixed order (deterministic).  HBM-bound: forward reads
// 4*B*T*V bytes once, backward reads them once more and writes as many.
// The metrics of the caption loops (top-5 accuracy :255-257 / :338-339, arg-max hypotheses :366-372) are comparisons of the
// same numbers: the metrics form of the forward counts them in that one read pass.
// The reward-weighted form (self-critical training) is the same kernels with row_weight [B]: ONE product per
// row, row_loss[r] * w[b] in the forward and (g / N) * w[b] in the backward, so weights of 1.0 leave every bit as it is;
// row_weight == nullptr is the unweighted loss and multiplies nothing.  The regulariser is never weighted.
#include <climits>

#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void online(float& m, float& s, float x) {
    if (x > m) {
        s = s * expf(m - x) + 1.f;
        m = x;
    } else {
        s += x == -INFINITY ? 0.f : expf(x - m);      // -inf before anything finite: x - m is inf - inf
    }
}

__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * expf(m - mm)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mm));
    m = mm;
}

// (value, index) pairs in the order "value descending, index ascending" -- the beam search's tie rule (csrc/beam.hip)
__device__ __forceinline__ void first_of(float& bm, int& bi, float m2, int i2) {
    if (m2 > bm || (m2 == bm && i2 < bi)) { bm = m2; bi = i2; }
}

// The metrics of a row, counted in the sweep that feeds the online softmax (MET): xt = x[target] is read before the sweep,
//     cnt = #{v : x[v] > xt} + #{v < tg : x[v] == xt}      the target's position in that order (top k <=> cnt < k)
//     (bm, bi) = the first element in that order           the arg-max, lowest index among equal maxima
// Pure comparisons of the stored numbers: exact, whatever the order of the merges.
struct RowMetrics {
    float xt, bm;
    int tg, cnt, bi;
    __device__ __forceinline__ void see(float x, int v) {
        cnt += (x > xt || (x == xt && v < tg)) ? 1 : 0;
        first_of(bm, bi, x, v);
    }
};

// one workgroup per (b, t) row of scores; MET: also row_rank[r] and preds[b][t] (scnattn_caption_loss_metrics_fwd)
template <bool VEC, bool MET>
__global__ __launch_bounds__(256) void ce_fwd_kernel(int T, int V, const float* __restrict__ scores,
                                                     const long long* __restrict__ targets, long ldt,
                                                     const int* __restrict__ dl, float* __restrict__ row_lse,
                                                     float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                     int* __restrict__ preds, long ldp,
                                                     const float* __restrict__ row_weight) {
    const int r = blockIdx.x, b = r / T, t = r - b * T;
    if (t >= dl[b]) {                         // not decoded: not part of the packed batch
        if (threadIdx.x == 0) {
            row_lse[r] = 0.f; row_loss[r] = 0.f;
            if (MET) { row_rank[r] = -1; preds[(long)b * ldp + t] = 0; }
        }
        return;
    }
    const float* x = scores + (long)r * V;
    float m = -INFINITY, s = 0.f;
    RowMetrics q = {0.f, -INFINITY, 0, 0, INT_MAX};
    bool valid = false;
    if (MET) {
        const long long tg = targets[(long)b * ldt + t];
        valid = tg >= 0 && tg < V;
        q.tg = valid ? (int)tg : 0;
        q.xt = x[q.tg];                        // a bad label counts against x[0]; its rank is not reported
    }
    if (VEC) {
        for (int v = threadIdx.x * 4; v < V; v += 1024) {
            const f32x4 e = *reinterpret_cast<const f32x4*>(x + v);
            online(m, s, e[0]); online(m, s, e[1]); online(m, s, e[2]); online(m, s, e[3]);
            if (MET) { q.see(e[0], v); q.see(e[1], v + 1); q.see(e[2], v + 2); q.see(e[3], v + 3); }
        }
    } else {
        for (int v = threadIdx.x; v < V; v += 256) {
            const float e = x[v];
            online(m, s, e);
            if (MET) q.see(e, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
    if (MET) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            q.cnt += __shfl_xor(q.cnt, o);
            first_of(q.bm, q.bi, __shfl_xor(q.bm, o), __shfl_xor(q.bi, o));
        }
    }
    __shared__ float sm[4], ss[4];
    __shared__ float qm[MET ? 4 : 1];
    __shared__ int qc[MET ? 4 : 1], qi[MET ? 4 : 1];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[w] = m; ss[w] = s;
        if (MET) { qm[w] = q.bm; qc[w] = q.cnt; qi[w] = q.bi; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = sm[0]; s = ss[0];
        merge(m, s, sm[1], ss[1]); merge(m, s, sm[2], ss[2]); merge(m, s, sm[3], ss[3]);
        const float lse = m + logf(s);
        const long long tg = targets[(long)b * ldt + t];
        row_lse[r] = lse;
        const float nll = (tg >= 0 && tg < V) ? lse - x[tg] : __builtin_nanf("");   // bad label poisons the loss, no fault
        row_loss[r] = row_weight ? nll * row_weight[b] : nll;
        if (MET) {
            first_of(q.bm, q.bi, qm[1], qi[1]); first_of(q.bm, q.bi, qm[2], qi[2]); first_of(q.bm, q.bi, qm[3], qi[3]);
            row_rank[r] = valid ? (qc[0] + qc[1]) + (qc[2] + qc[3]) : INT_MAX;
            preds[(long)b * ldp + t] = q.bi < V ? q.bi : 0;      // a row of NaN alone has no first element
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ce_bwd_kernel(int T, int V, const float* __restrict__ scores,
                                                     const long long* __restrict__ targets, long ldt,
                                                     const int* __restrict__ dl, const float* __restrict__ row_lse,
                                                     const float* __restrict__ gout, float inv_n,
                                                     const float* __restrict__ row_weight,
                                                     float* __restrict__ dscores) {
    const int r = blockIdx.x, b = r / T, t = r - b * T;
    float* d = dscores + (long)r * V;
    const bool on = t < dl[b];
    const float* x = scores + (long)r * V;
    const float lse = on ? row_lse[r] : 0.f;
    const float gn = on ? gout[0] * inv_n : 0.f;
    const float g = (on && row_weight) ? gn * row_weight[b] : gn;
    const long long tl = on ? targets[(long)b * ldt + t] : -1;
    const int tg = (tl >= 0 && tl < V) ? (int)tl : -1;      // compared in 64 bits: 2^32 + 3 is a bad label, not label 3
    if (VEC) {
        for (int v = threadIdx.x * 4; v < V; v += 1024) {
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (on) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(x + v);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (expf(q[j] - lse) - (v + j == tg ? 1.f : 0.f)) * g;
            }
            *reinterpret_cast<f32x4*>(d + v) = o;
        }
    } else {
        for (int v = threadIdx.x; v < V; v += 256) d[v] = on ? (expf(x[v] - lse) - (v == tg ? 1.f : 0.f)) * g : 0.f;
    }
}

// sm1[b][p] = sum_t alphas[b][t][p] - 1 ; reg_part[b] = sum_p sm1^2
__global__ __launch_bounds__(256) void alpha_reg_fwd_kernel(int T, int P, const float* __restrict__ alphas,
                                                            float* __restrict__ sm1, float* __restrict__ reg_part) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int p = threadIdx.x; p < P; p += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += alphas[((long)b * T + t) * P + p];
        s -= 1.f;
        sm1[(long)b * P + p] = s;
        acc += s * s;
    }
    acc = wave_sum(acc);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) reg_part[b] = (part[0] + part[1]) + (part[2] + part[3]);
}

// loss = sum(row_loss)/N + alpha_c * sum(reg_part)/(B*P); one workgroup, fixed order
// MET: also hits[0] = #{0 <= row_rank < k}, hits[1] = #{row_rank == 0} (integer sums: exact in any order)
template <bool MET>
__global__ __launch_bounds__(256) void loss_finalize_kernel(long nrows, const float* __restrict__ row_loss, float inv_n,
                                                            int B, const float* __restrict__ reg_part, float reg_scale,
                                                            float* __restrict__ loss, const int* __restrict__ row_rank, int k,
                                                            int* __restrict__ hits) {
    float a = 0.f, c = 0.f;
    int hk = 0, h1 = 0;
    for (long i = threadIdx.x; i < nrows; i += 256) {
        a += row_loss[i];
        if (MET) {
            const int rk = row_rank[i];
            hk += (rk >= 0 && rk < k) ? 1 : 0;
            h1 += rk == 0 ? 1 : 0;
        }
    }
    if (reg_part)
        for (int i = threadIdx.x; i < B; i += 256) c += reg_part[i];
    a = wave_sum(a);
    c = wave_sum(c);
    if (MET) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { hk += __shfl_xor(hk, o); h1 += __shfl_xor(h1, o); }
    }
    __shared__ float pa[4], pc[4];
    __shared__ int pk[MET ? 4 : 1], p1[MET ? 4 : 1];
    if ((threadIdx.x & 63) == 0) {
        pa[threadIdx.x >> 6] = a; pc[threadIdx.x >> 6] = c;
        if (MET) { pk[threadIdx.x >> 6] = hk; p1[threadIdx.x >> 6] = h1; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = ((pa[0] + pa[1]) + (pa[2] + pa[3])) * inv_n + ((pc[0] + pc[1]) + (pc[2] + pc[3])) * reg_scale;
        if (MET) { hits[0] = (pk[0] + pk[1]) + (pk[2] + pk[3]); hits[1] = (p1[0] + p1[1]) + (p1[2] + p1[3]); }
    }
}

// dalphas[b][t][p] = g * alpha_c * 2 * sm1[b][p] / (B*P)   (every t: alphas.sum(dim=1) runs over all T)
__global__ __launch_bounds__(256) void alpha_reg_bwd_kernel(long n, int T, int P, const float* __restrict__ sm1,
                                                            const float* __restrict__ gout, float scale,
                                                            float* __restrict__ dalphas) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / ((long)T * P);
    const int p = (int)(i % P);
    dalphas[i] = gout[0] * scale * sm1[b * P + p];
}

}  // namespace

namespace {

// the forward launches; row_rank == nullptr: the loss alone
int loss_fwd_launch(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                    const int* dl, long n_tokens, const float* alphas, float alpha_c, float* row_lse, float* row_loss,
                    float* sm1, float* reg_part, float* loss, int k, int* row_rank, int* preds, long ldp, int* hits,
                    const float* row_weight) {
    const bool vec = (V % 4 == 0) && aligned16(scores);
    const bool met = row_rank != nullptr;
#define SCN_CE_FWD(VEC, MET)                                                                                                 \
    hipLaunchKernelGGL((ce_fwd_kernel<VEC, MET>), dim3(B * T), dim3(256), 0, st, T, V, scores, targets, ldt, dl, row_lse, \
                       row_loss, row_rank, preds, ldp, row_weight)
    if (met) { if (vec) SCN_CE_FWD(true, true); else SCN_CE_FWD(false, true); }
    else     { if (vec) SCN_CE_FWD(true, false); else SCN_CE_FWD(false, false); }
#undef SCN_CE_FWD
    SCN_LAUNCH_CHECK();
    if (alphas) {
        hipLaunchKernelGGL(alpha_reg_fwd_kernel, dim3(B), dim3(256), 0, st, T, P, alphas, sm1, reg_part);
        SCN_LAUNCH_CHECK();
    }
    const float inv_n = 1.f / (float)n_tokens, reg_scale = alphas ? alpha_c / ((float)B * (float)P) : 0.f;
    if (met)
        hipLaunchKernelGGL(loss_finalize_kernel<true>, dim3(1), dim3(256), 0, st, (long)B * T, row_loss, inv_n, B,
                           alphas ? reg_part : nullptr, reg_scale, loss, row_rank, k, hits);
    else
        hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(256), 0, st, (long)B * T, row_loss, inv_n, B,
                           alphas ? reg_part : nullptr, reg_scale, loss, nullptr, 0, nullptr);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int caption_loss_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                     const int* dl, long n_tokens, const float* alphas, float alpha_c, float* row_lse, float* row_loss,
                     float* sm1, float* reg_part, float* loss) {
    SCN_ARG(B > 0 && T > 0 && V > 0 && n_tokens > 0, "caption_loss_fwd: bad shape");
    SCN_ARG(scores && targets && dl && row_lse && row_loss && loss && ldt >= T, "caption_loss_fwd: bad argument");
    SCN_ARG(!alphas || (P > 0 && sm1 && reg_part), "caption_loss_fwd: alphas without workspace");
    return loss_fwd_launch(st, B, T, V, P, scores, targets, ldt, dl, n_tokens, alphas, alpha_c, row_lse, row_loss, sm1,
                           reg_part, loss, 0, nullptr, nullptr, 0, nullptr, nullptr);
}

int caption_loss_weighted_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                              long ldt, const int* dl, long n_tokens, const float* row_weight, const float* alphas,
                              float alpha_c, float* row_lse, float* row_loss, float* sm1, float* reg_part, float* loss) {
    SCN_ARG(B > 0 && T > 0 && V > 0 && n_tokens > 0, "caption_loss_weighted_fwd: bad shape");
    SCN_ARG(scores && targets && dl && row_lse && row_loss && loss && ldt >= T, "caption_loss_weighted_fwd: bad argument");
    SCN_ARG(row_weight, "caption_loss_weighted_fwd: row_weight is NULL");
    SCN_ARG(!alphas || (P > 0 && sm1 && reg_part), "caption_loss_weighted_fwd: alphas without workspace");
    return loss_fwd_launch(st, B, T, V, P, scores, targets, ldt, dl, n_tokens, alphas, alpha_c, row_lse, row_loss, sm1,
                           reg_part, loss, 0, nullptr, nullptr, 0, nullptr, row_weight);
}

int caption_loss_metrics_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                             long ldt, const int* dl, long n_tokens, const float* alphas, float alpha_c, float* row_lse,
                             float* row_loss, float* sm1, float* reg_part, float* loss, int k, int* row_rank, int* preds,
                             long ldp, int* hits) {
    SCN_ARG(B > 0 && T > 0 && V > 0 && n_tokens > 0, "caption_loss_metrics_fwd: bad shape");
    SCN_ARG(scores && targets && dl && row_lse && row_loss && loss && ldt >= T, "caption_loss_metrics_fwd: bad argument");
    SCN_ARG(!alphas || (P > 0 && sm1 && reg_part), "caption_loss_metrics_fwd: alphas without workspace");
    SCN_ARG(k >= 1, "caption_loss_metrics_fwd: k must be >= 1");
    SCN_ARG(row_rank && preds && hits && ldp >= T, "caption_loss_metrics_fwd: bad metrics output");
    return loss_fwd_launch(st, B, T, V, P, scores, targets, ldt, dl, n_tokens, alphas, alpha_c, row_lse, row_loss, sm1,
                           reg_part, loss, k, row_rank, preds, ldp, hits, nullptr);
}

namespace {

int loss_bwd_launch(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                    const int* dl, long n_tokens, const float* row_lse, const float* sm1, float alpha_c, const float* gout,
                    float* dscores, float* dalphas, const float* row_weight) {
    const bool vec = (V % 4 == 0) && aligned16(scores) && aligned16(dscores);
    const float inv_n = 1.f / (float)n_tokens;
    if (vec) hipLaunchKernelGGL(ce_bwd_kernel<true>, dim3(B * T), dim3(256), 0, st, T, V, scores, targets, ldt, dl, row_lse, gout, inv_n, row_weight, dscores);
    else     hipLaunchKernelGGL(ce_bwd_kernel<false>, dim3(B * T), dim3(256), 0, st, T, V, scores, targets, ldt, dl, row_lse, gout, inv_n, row_weight, dscores);
    SCN_LAUNCH_CHECK();
    if (dalphas) {
        const long n = (long)B * T * P;
        hipLaunchKernelGGL(alpha_reg_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, T, P, sm1, gout,
                           2.f * alpha_c / ((float)B * (float)P), dalphas);
        SCN_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

int caption_loss_bwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                     const int* dl, long n_tokens, const float* row_lse, const float* sm1, float alpha_c,
                     const float* gout, float* dscores, float* dalphas) {
    SCN_ARG(B > 0 && T > 0 && V > 0 && n_tokens > 0, "caption_loss_bwd: bad shape");
    SCN_ARG(scores && targets && dl && row_lse && gout && dscores && ldt >= T, "caption_loss_bwd: bad argument");
    SCN_ARG(!dalphas || (P > 0 && sm1), "caption_loss_bwd: dalphas without sm1");
    return loss_bwd_launch(st, B, T, V, P, scores, targets, ldt, dl, n_tokens, row_lse, sm1, alpha_c, gout, dscores, dalphas,
                           nullptr);
}

int caption_loss_weighted_bwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                              long ldt, const int* dl, long n_tokens, const float* row_weight, const float* row_lse,
                              const float* sm1, float alpha_c, const float* gout, float* dscores, float* dalphas) {
    SCN_ARG(B > 0 && T > 0 && V > 0 && n_tokens > 0, "caption_loss_weighted_bwd: bad shape");
    SCN_ARG(scores && targets && dl && row_lse && gout && dscores && ldt >= T, "caption_loss_weighted_bwd: bad argument");
    SCN_ARG(row_weight, "caption_loss_weighted_bwd: row_weight is NULL");
    SCN_ARG(!dalphas || (P > 0 && sm1), "caption_loss_weighted_bwd: dalphas without sm1");
    return loss_bwd_launch(st, B, T, V, P, scores, targets, ldt, dl, n_tokens, row_lse, sm1, alpha_c, gout, dscores, dalphas,
                           row_weight);
}

}  // namespace scn
