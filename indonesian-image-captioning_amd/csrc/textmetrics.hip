// Caption text metrics over token ids: the n-gram statistics of BLEU-1..4, LCS / ROUGE-L and CIDEr-D (n = 1..4, sigma = 6,
// x10) -- what the reference's eval_caption.py:135-165 obtains from NLGEval after the beam search, and the counting half of
// utils/metric.py::corpus_bleu (validate()).  Definitions and output layouts: include/scnattn.h.
//
// One workgroup of TM_NT = SCNATTN_TEXT_MAX_LEN = 128 threads (two waves) per image: thread i owns position i of the sequence at
// hand.  A sequence is first COMPACTED into LDS -- tokens on the caller's skip list are dropped, the order kept -- with one
// ballot per wave; everything after that reads LDS only.  Counting needs no table and no hash: thread i walks the other
// sequence once, keeping a window of four tokens in registers, and takes the length m <= 4 of the common prefix of "my
// n-grams" and "the n-grams at j"; the n-gram of order n occurs at j exactly when m >= n, so ONE walk counts all four orders.
// Token values are compared and packed, never used as indices.  Lengths read from memory are clamped to [0, padded width].
// Sums are integer, or fp64 reduced in a fixed order (wave butterfly, then wave 0 + wave 1): the kernels are deterministic,
// there is no floating-point atomic.
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {
namespace {

constexpr int TM_NT = SCNATTN_TEXT_MAX_LEN;        // threads of a workgroup = longest compacted sequence
constexpr int TM_LD = TM_NT + 4;                   // LDS row: four zero tokens behind the last one (the register window reads them)
constexpr int TM_MAXR = SCNATTN_TEXT_MAX_REFS;
constexpr int TM_TOKEN_MAX = SCNATTN_TEXT_CIDER_MAX_TOKEN;
constexpr long long TM_SENTINEL = -1;              // 0xffff in all four fields: no admitted token is 0xffff
static_assert(TM_NT == 128, "two waves per workgroup are assumed below");

struct Skip {
    int n;
    int id[4];
};

__device__ __forceinline__ bool skipped(const Skip& s, int tok) {
    bool r = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= (k < s.n) & (tok == s.id[k]);
    return r;
}

// src[0 .. clamp(len_mem, 0, width)) without the skipped ids -> dst[0 .. ret), zeros up to dst[TM_LD).  Every thread calls it.
__device__ int load_compact(const int32_t* __restrict__ src, int len_mem, int width, const Skip& sk, int* dst, int* wcnt) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int len = min(max(len_mem, 0), width);
    const int tok = t < len ? src[t] : 0;
    const bool keep = t < len && !skipped(sk, tok);
    const unsigned long long b = __ballot(keep);
    __syncthreads();                                // the previous user of dst / wcnt is done
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    const int c0 = wcnt[0], total = c0 + wcnt[1];
    const int pos = __popcll(b & ((1ull << lane) - 1ull)) + (wave ? c0 : 0);
    if (keep) dst[pos] = tok;
    if (t >= total) dst[t] = 0;
    if (t < 4) dst[TM_NT + t] = 0;
    __syncthreads();
    return total;
}

// Thread-local view of "my" up to four tokens at position i of a sequence of length la.
struct Mine {
    int h0, h1, h2, h3, nv;     // nv = min(4, la - i), <= 0: no n-gram starts here
};
__device__ __forceinline__ Mine mine_at(const int* a, int la, int i) {
    Mine m;
    m.nv = min(4, la - i);
    const int ii = min(i, TM_NT - 1);
    m.h0 = a[ii]; m.h1 = a[ii + 1]; m.h2 = a[ii + 2]; m.h3 = a[ii + 3];
    return m;
}

// cnt[n-1] += occurrences of my n-gram among positions [0, jend) of b (length lb); before[n-1] |= one of them lies in [0, jbefore)
__device__ __forceinline__ void count_in(const Mine& me, const int* b, int lb, int jend, int jbefore, int cnt[4], bool before[4]) {
    if (me.nv <= 0) return;
    int w0 = b[0], w1 = b[1], w2 = b[2], w3 = b[3];
    for (int j = 0; j < jend; ++j) {
        const int lim = min(me.nv, lb - j);
        const bool e0 = lim > 0 && me.h0 == w0;
        const bool e1 = e0 && lim > 1 && me.h1 == w1;
        const bool e2 = e1 && lim > 2 && me.h2 == w2;
        const bool e3 = e2 && lim > 3 && me.h3 == w3;
        cnt[0] += e0; cnt[1] += e1; cnt[2] += e2; cnt[3] += e3;
        const bool bf = j < jbefore;
        before[0] |= bf && e0; before[1] |= bf && e1; before[2] |= bf && e2; before[3] |= bf && e3;
        w0 = w1; w1 = w2; w2 = w3; w3 = b[j + 4];        // j + 4 <= TM_NT + 3 < TM_LD
    }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- kernel a: n-gram statistics ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_NT) void text_ngram_stats_kernel(int R, const int32_t* __restrict__ hyp, int Lh,
                                                                 const int32_t* __restrict__ hyp_len,
                                                                 const int32_t* __restrict__ ref, int Lr,
                                                                 const int32_t* __restrict__ ref_len, Skip sk_h, Skip sk_r,
                                                                 int32_t* __restrict__ stats) {
    __shared__ int sh[TM_LD], sr[TM_LD], wcnt[2], red[2][4];
    const long img = blockIdx.x;
    const int t = threadIdx.x;
    const int lh = load_compact(hyp + img * Lh, hyp_len[img], Lh, sk_h, sh, wcnt);
    const Mine me = mine_at(sh, lh, t);
    int tf[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
    bool dup[4] = {false, false, false, false};
    count_in(me, sh, lh, lh, t, tf, dup);
    int best = -1;                                  // closest reference length; a tie goes to the shorter one
    for (int r = 0; r < R; ++r) {
        const int lmem = ref_len[img * R + r];
        if (lmem < 0) continue;                     // absent slot (uniform over the workgroup)
        const int lr = load_compact(ref + (img * R + r) * Lr, lmem, Lr, sk_r, sr, wcnt);
        int c[4] = {0, 0, 0, 0};
        bool unused[4] = {false, false, false, false};
        count_in(me, sr, lr, lr, 0, c, unused);
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = max(mx[k], c[k]);
        if (best < 0 || abs(lr - lh) < abs(best - lh) || (abs(lr - lh) == abs(best - lh) && lr < best)) best = lr;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = (me.nv > k && !dup[k]) ? min(tf[k], mx[k]) : 0;
        const int s = wave_sum_i(v);
        if ((t & 63) == 0) red[t >> 6][k] = s;
    }
    __syncthreads();
    if (t < 4) {
        stats[img * 10 + t] = red[0][t] + red[1][t];
        stats[img * 10 + 4 + t] = max(0, lh - t);   // guesses of order t + 1
    }
    if (t == 4) stats[img * 10 + 8] = lh;
    if (t == 5) stats[img * 10 + 9] = max(best, 0);
}

// ---- kernel b: LCS by the bit-parallel recurrence on a 128-bit word, ROUGE-L --------------------------------------------------
__global__ __launch_bounds__(TM_NT) void text_lcs_kernel(int R, const int32_t* __restrict__ hyp, int Lh,
                                                         const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ ref,
                                                         int Lr, const int32_t* __restrict__ ref_len, Skip sk_h, Skip sk_r,
                                                         int32_t* __restrict__ lcs, double* __restrict__ score) {
    __shared__ int sh[TM_LD], sr[TM_LD], wcnt[2];
    __shared__ unsigned long long mlo[TM_NT], mhi[TM_NT];
    const long img = blockIdx.x;
    const int t = threadIdx.x;
    const int lh = load_compact(hyp + img * Lh, hyp_len[img], Lh, sk_h, sh, wcnt);
    double P = 0.0, Rc = 0.0;                       // thread 0 only
    for (int r = 0; r < R; ++r) {
        const int lmem = ref_len[img * R + r];
        if (lmem < 0) {
            if (t == 0) lcs[img * R + r] = 0;
            continue;
        }
        const int lr = load_compact(ref + (img * R + r) * Lr, lmem, Lr, sk_r, sr, wcnt);
        // bit i of M_j: hyp[i] == ref[j]
        unsigned long long lo = 0, hi = 0;
        if (t < lr) {
            const int tok = sr[t];
            for (int i = 0; i < min(lh, 64); ++i) lo |= (unsigned long long)(sh[i] == tok) << i;
            for (int i = 64; i < lh; ++i) hi |= (unsigned long long)(sh[i] == tok) << (i - 64);
        }
        mlo[t] = lo; mhi[t] = hi;
        __syncthreads();
        if (t == 0) {
            // V starts all ones; per reference token U = V & M, V = (V + U) | (V & ~U); the zeros of V below bit lh count the LCS
            unsigned long long vlo = ~0ull, vhi = ~0ull;
            for (int j = 0; j < lr; ++j) {
                const unsigned long long ulo = vlo & mlo[j], uhi = vhi & mhi[j];
                const unsigned long long slo = vlo + ulo;
                const unsigned long long shi = vhi + uhi + (slo < vlo ? 1ull : 0ull);
                vlo = slo | (vlo & ~ulo);
                vhi = shi | (vhi & ~uhi);
            }
            const unsigned long long zlo = ~vlo & (lh >= 64 ? ~0ull : ((1ull << lh) - 1ull));
            const unsigned long long zhi = lh > 64 ? (~vhi & (lh >= 128 ? ~0ull : ((1ull << (lh - 64)) - 1ull))) : 0ull;
            const int l = __popcll(zlo) + __popcll(zhi);
            lcs[img * R + r] = l;
            if (lh > 0) P = fmax(P, (double)l / (double)lh);
            if (lr > 0) Rc = fmax(Rc, (double)l / (double)lr);
        }
    }
    if (t == 0) {
        const double beta2 = 1.2 * 1.2;
        score[img] = (P > 0.0 && Rc > 0.0) ? ((1.0 + beta2) * P * Rc) / (Rc + beta2 * P) : 0.0;
    }
}

// ---- kernels c and d: CIDEr-D -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool token_ok(int tok) { return tok >= 0 && tok <= TM_TOKEN_MAX; }
__device__ __forceinline__ long long pack_key(const Mine& m, int n) {       // n <= m.nv
    unsigned long long k = (unsigned long long)(m.h0 & 0xffff);
    if (n > 1) k |= (unsigned long long)(m.h1 & 0xffff) << 16;
    if (n > 2) k |= (unsigned long long)(m.h2 & 0xffff) << 32;
    if (n > 3) k |= (unsigned long long)(m.h3 & 0xffff) << 48;
    return (long long)k;
}

// All references of the image, compacted, in LDS.  Returns through lens[] (-1: absent); flags out-of-range tokens.
__device__ void load_refs(int R, const int32_t* __restrict__ ref, int Lr, const int32_t* __restrict__ ref_len, long img,
                          const Skip& sk, int (*srs)[TM_LD], int* lens, int* wcnt, int32_t* flag) {
    const int t = threadIdx.x;
    for (int r = 0; r < R; ++r) {
        const int lmem = ref_len[img * R + r];
        if (lmem < 0) {
            if (t == 0) lens[r] = -1;
            continue;
        }
        const int lr = load_compact(ref + (img * R + r) * Lr, lmem, Lr, sk, srs[r], wcnt);
        if (t == 0) lens[r] = lr;
        if (t < lr && !token_ok(srs[r][t])) *flag = 1;
    }
    __syncthreads();
}

// kernel c: keys[img][r][j] = the n-gram at position j of reference r, TM_SENTINEL where none starts there or where the same
// n-gram stands earlier in this image's references (an earlier slot, or an earlier position of this slot)
__global__ __launch_bounds__(TM_NT) void text_ref_keys_kernel(int n, int R, const int32_t* __restrict__ ref, int Lr,
                                                              const int32_t* __restrict__ ref_len, Skip sk,
                                                              long long* __restrict__ keys, int32_t* __restrict__ flag) {
    __shared__ int srs[TM_MAXR][TM_LD], lens[TM_MAXR], wcnt[2];
    const long img = blockIdx.x;
    const int t = threadIdx.x;
    load_refs(R, ref, Lr, ref_len, img, sk, srs, lens, wcnt, flag);
    for (int r = 0; r < R; ++r) {
        const int lr = lens[r];
        long long key = TM_SENTINEL;
        if (lr >= 0) {
            const Mine me = mine_at(srs[r], lr, t);
            if (me.nv >= n) {
                int c[4] = {0, 0, 0, 0};
                bool unused[4] = {false, false, false, false};
                for (int q = 0; q < r; ++q)
                    if (lens[q] >= 0) count_in(me, srs[q], lens[q], lens[q], 0, c, unused);
                count_in(me, srs[r], lr, t, 0, c, unused);
                if (c[n - 1] == 0) key = pack_key(me, n);
            }
        }
        if (t < Lr) keys[(img * R + r) * Lr + t] = key;
    }
}

struct DfTable {
    const long long* keys[4];
    const int32_t* df[4];
    int len[4];
};

// df of a key: binary search of the sorted unique keys (signed order, as the host sorted them); 0 when absent
__device__ __forceinline__ int df_of(const DfTable& tb, int k, long long key) {
    int lo = 0, hi = tb.len[k];
    const long long* __restrict__ a = tb.keys[k];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < tb.len[k] && a[lo] == key) ? tb.df[k][lo] : 0;
}

// sums of v[0..NV) over the workgroup, fixed order; every thread receives them
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double (*red)[8]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum_d(v[k]);
        if ((t & 63) == 0) red[t >> 6][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = red[0][k] + red[1][k];
}

// kernel d: score[img] = 10 / |refs| * sum_refs 1/4 sum_n  clip-cosine_n(hyp, ref) * exp(-(lh - lr)^2 / (2 sigma^2))
__global__ __launch_bounds__(TM_NT) void text_cider_kernel(int R, const int32_t* __restrict__ hyp, int Lh,
                                                           const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ ref,
                                                           int Lr, const int32_t* __restrict__ ref_len, Skip sk_h, Skip sk_r,
                                                           DfTable tb, double n_images, double* __restrict__ score,
                                                           int32_t* __restrict__ flag) {
    __shared__ int sh[TM_LD], srs[TM_MAXR][TM_LD], lens[TM_MAXR], wcnt[2];
    __shared__ double red[2][8];
    const long img = blockIdx.x;
    const int t = threadIdx.x;
    const double log_n = log(n_images);             // the same log as the one applied to df: df = n_images gives exactly 0
    const int lh = load_compact(hyp + img * Lh, hyp_len[img], Lh, sk_h, sh, wcnt);
    if (t < lh && !token_ok(sh[t])) *flag = 1;
    load_refs(R, ref, Lr, ref_len, img, sk_r, srs, lens, wcnt, flag);

    // hypothesis side: tf, first occurrence, idf and weight of my n-grams
    const Mine me = mine_at(sh, lh, t);
    int tfh[4] = {0, 0, 0, 0};
    bool duph[4] = {false, false, false, false};
    count_in(me, sh, lh, lh, t, tfh, duph);
    double idf[4], wh[4], nh2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool live = me.nv > k && !duph[k];
        idf[k] = live ? log_n - log((double)max(1, df_of(tb, k, pack_key(me, k + 1)))) : 0.0;
        wh[k] = live ? (double)tfh[k] * idf[k] : 0.0;
        nh2[k] = wh[k] * wh[k];
    }
    block_sum_d<4>(nh2, red);

    double acc[4] = {0.0, 0.0, 0.0, 0.0};           // thread 0: sum over references of the per-order values
    int nref = 0;
    for (int r = 0; r < R; ++r) {
        const int lr = lens[r];
        if (lr < 0) continue;
        ++nref;
        // v[0..4): clipped dot products over my hypothesis n-grams; v[4..8): squared weights of my reference n-grams
        double v[8];
        int c[4] = {0, 0, 0, 0};
        bool unused[4] = {false, false, false, false};
        count_in(me, srs[r], lr, lr, 0, c, unused);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double wr = (double)c[k] * idf[k];
            v[k] = fmin(wh[k], wr) * wr;            // wh = 0 for the positions that do not count
        }
        const Mine rm = mine_at(srs[r], lr, t);
        int tfr[4] = {0, 0, 0, 0};
        bool dupr[4] = {false, false, false, false};
        count_in(rm, srs[r], lr, lr, t, tfr, dupr);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double w = 0.0;
            if (rm.nv > k && !dupr[k])
                w = (double)tfr[k] * (log_n - log((double)max(1, df_of(tb, k, pack_key(rm, k + 1)))));
            v[4 + k] = w * w;
        }
        block_sum_d<8>(v, red);
        if (t == 0) {
            const double d = (double)(lh - lr);
            const double pen = exp(-(d * d) / (2.0 * 6.0 * 6.0));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double val = v[k];
                const double den = sqrt(nh2[k]) * sqrt(v[4 + k]);
                if (den != 0.0) val /= den;
                acc[k] += val * pen;
            }
        }
    }
    if (t == 0) {
        const double s = (((acc[0] + acc[1]) + acc[2]) + acc[3]) / 4.0;
        score[img] = nref > 0 ? s / (double)nref * 10.0 : 0.0;
    }
}

// mean of n doubles in a fixed order: thread t sums elements t, t + 256, ... ascending, then a tree over the 256 partials
__global__ __launch_bounds__(256) void text_mean_kernel(const double* __restrict__ in, long n, double* __restrict__ out) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (long i = t; i < n; i += 256) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) *out = n > 0 ? part[0] / (double)n : 0.0;
}

int make_skip(const char* who, const int32_t* ids, int n, Skip& out) {
    out = Skip{0, {0, 0, 0, 0}};
    if (n < 0 || n > 4) { set_error("%s: invalid argument: a skip list holds 0..4 token ids", who); return -1; }
    if (n > 0 && !ids) { set_error("%s: invalid argument: null skip list with a non-zero count", who); return -1; }
    out.n = n;
    for (int k = 0; k < n; ++k) out.id[k] = ids[k];
    return 0;
}

int check_dims(const char* who, int N, int R, int Lh, int Lr, bool with_hyp) {
    if (N < 0) { set_error("%s: invalid argument: N < 0", who); return -1; }
    if (R < 1 || R > TM_MAXR) { set_error("%s: invalid argument: R outside 1..SCNATTN_TEXT_MAX_REFS", who); return -1; }
    if ((with_hyp && (Lh < 1 || Lh > TM_NT)) || Lr < 1 || Lr > TM_NT) {
        set_error("%s: invalid argument: padded width outside 1..SCNATTN_TEXT_MAX_LEN", who);
        return -1;
    }
    return 0;
}

}  // namespace

int text_max_len() { return TM_NT; }

int text_ngram_stats(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                     int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                     int n_skip_ref, int32_t* stats) {
    const char* who = "scnattn_text_ngram_stats";
    Skip sh, sr;
    if (!(hyp && hyp_len && ref && ref_len && stats)) { set_error("%s: invalid argument: null pointer", who); return -1; }
    SCN_TRY(check_dims(who, N, R, Lh, Lr, true));
    SCN_TRY(make_skip(who, skip_hyp, n_skip_hyp, sh));
    SCN_TRY(make_skip(who, skip_ref, n_skip_ref, sr));
    if (N == 0) return 0;
    hipLaunchKernelGGL(text_ngram_stats_kernel, dim3(N), dim3(TM_NT), 0, st, R, hyp, Lh, hyp_len, ref, Lr, ref_len, sh, sr,
                       stats);
    SCN_LAUNCH_CHECK();
    return 0;
}

int text_lcs(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
             const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
             int32_t* lcs, double* score, double* mean) {
    const char* who = "scnattn_text_lcs";
    Skip sh, sr;
    if (!(hyp && hyp_len && ref && ref_len && lcs && score)) { set_error("%s: invalid argument: null pointer", who); return -1; }
    SCN_TRY(check_dims(who, N, R, Lh, Lr, true));
    SCN_TRY(make_skip(who, skip_hyp, n_skip_hyp, sh));
    SCN_TRY(make_skip(who, skip_ref, n_skip_ref, sr));
    if (N > 0) {
        hipLaunchKernelGGL(text_lcs_kernel, dim3(N), dim3(TM_NT), 0, st, R, hyp, Lh, hyp_len, ref, Lr, ref_len, sh, sr, lcs,
                           score);
        SCN_LAUNCH_CHECK();
    }
    if (mean) {
        hipLaunchKernelGGL(text_mean_kernel, dim3(1), dim3(256), 0, st, score, (long)N, mean);
        SCN_LAUNCH_CHECK();
    }
    return 0;
}

int text_ref_keys(hipStream_t st, int n, int N, int R, const int32_t* ref, int Lr, const int32_t* ref_len,
                  const int32_t* skip_ref, int n_skip_ref, int64_t* keys, int32_t* flag) {
    const char* who = "scnattn_text_ref_keys";
    Skip sr;
    if (!(ref && ref_len && keys && flag)) { set_error("%s: invalid argument: null pointer", who); return -1; }
    if (n < 1 || n > 4) { set_error("%s: invalid argument: n outside 1..4", who); return -1; }
    SCN_TRY(check_dims(who, N, R, 1, Lr, false));
    SCN_TRY(make_skip(who, skip_ref, n_skip_ref, sr));
    SCN_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    if (N == 0) return 0;
    hipLaunchKernelGGL(text_ref_keys_kernel, dim3(N), dim3(TM_NT), 0, st, n, R, ref, Lr, ref_len, sr,
                       reinterpret_cast<long long*>(keys), flag);
    SCN_LAUNCH_CHECK();
    return 0;
}

int text_cider(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
               const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
               const int64_t* table_keys, const int32_t* table_df, const long* table_off, long n_images, double* score,
               double* mean, int32_t* flag) {
    const char* who = "scnattn_text_cider";
    Skip sh, sr;
    if (!(hyp && hyp_len && ref && ref_len && table_off && score && flag)) {
        set_error("%s: invalid argument: null pointer", who);
        return -1;
    }
    SCN_TRY(check_dims(who, N, R, Lh, Lr, true));
    SCN_TRY(make_skip(who, skip_hyp, n_skip_hyp, sh));
    SCN_TRY(make_skip(who, skip_ref, n_skip_ref, sr));
    if (n_images < 1) { set_error("%s: invalid argument: n_images < 1", who); return -1; }
    DfTable tb;
    if (table_off[0] != 0) { set_error("%s: invalid argument: table_off[0] != 0", who); return -1; }
    for (int k = 0; k < 4; ++k) {
        const long len = table_off[k + 1] - table_off[k];
        if (len < 0 || len > 0x7fffffffL) { set_error("%s: invalid argument: table_off is not ascending", who); return -1; }
        tb.len[k] = (int)len;
        tb.keys[k] = reinterpret_cast<const long long*>(table_keys) + table_off[k];
        tb.df[k] = table_df + table_off[k];
    }
    if (table_off[4] > 0 && !(table_keys && table_df)) { set_error("%s: invalid argument: null table", who); return -1; }
    SCN_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    if (N > 0) {
        hipLaunchKernelGGL(text_cider_kernel, dim3(N), dim3(TM_NT), 0, st, R, hyp, Lh, hyp_len, ref, Lr, ref_len, sh, sr, tb,
                           (double)n_images, score, flag);
        SCN_LAUNCH_CHECK();
    }
    if (mean) {
        hipLaunchKernelGGL(text_mean_kernel, dim3(1), dim3(256), 0, st, score, (long)N, mean);
        SCN_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace scn
