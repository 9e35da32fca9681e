// Batched beam search (models/decoders/_common.py:beam_search_batched; the reference's sample(), attention_scn.py:160-296,
// for N images at once).  K = beam_size slots per image, rows of every per-step buffer are n*K + j, nothing shrinks:
//   nsrc[n]  live source beams of image n (slots 0 .. nsrc-1); kk[n] beams still to fill (0: the image is finished)
// The k rows of one image attend over the SAME att1[n] / enc[n]; the two attention kernels here read that map once per
// image and feed K accumulators from every loaded fragment, where the per-image search keeps k materialised copies:
//   beam_attn_scores   e[n*K+j][p] = w . relu(att1[n][p][:] + att2[n*K+j][:]) + b0      (attn_scores_kernel's pixel-row layout)
//   beam_attn_context  K softmaxes over P, awe / z for the K rows from one pass over enc[n] (attn_context_kernel's tiles)
//   beam_row_topk_ens  per live row: per member the log-softmax statistics of its logits row, then the row's top K of
//                      score + c_v, where c_v is the weighted mean of the members' log-probabilities (mode 0) or the log of
//                      the weighted mean of their probabilities (mode 1).  ONE kernel template serves every search: the
//                      single decoder is one member of weight 1 in mode 0 (beam_row_topk, c_v = logit - lse to the bit), and
//                      with EXCLUSIONS (search options) banned words, <end> before min_length and words that
//                      would repeat an n-gram of the row's history are not candidates (a bitmap in LDS)
//   beam_merge         per image: the top kk of the nsrc x K row candidates, <end> picks recorded, the rest compacted
//   beam_merge_groups  the same for a search in G groups of Kg slots (diverse beam search): the groups of an
//                      image in order, each ranking its candidates after a penalty per word the groups before it picked at
//                      this step; nsrc / kk / ncomp / best_* are then per (image, group) and the row selection decides
//                      liveness per group (its Kg parameter)
//   beam_merge_banks   the merge of a CONSTRAINED search: the selection (its CON flavour) also emits per row
//                      the image's unmet required words as 4 candidates of their own; the nsrc x (K + 4) candidates fall
//                      into banks by the number of required words met, the kk picks go round-robin over the banks, and the
//                      per-slot mask `met` is written here, where the parent and the word are both known
//   beam_advance       h / c gathered from the parent slot, next input embedding gathered from the table; with search
//                      options (beam_advance_opt, the same kernel) also the per-beam word history int32 [N*K][max_steps],
//                      gathered from the parent slot and extended
// ORDER (the tie rule): candidates are ranked by (value descending, flat index j*V + v ascending), values compared as the
// fp32 numbers the kernel computes.  Dead slots (j >= nsrc) are never read as candidates and never written by the first
// three kernels; beam_merge / beam_advance fill them with a copy of slot 0 (or zeros), so every row stays finite.
// Plain vector stores only; no kernel waits for another workgroup.
#include <climits>
#include <type_traits>
#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

constexpr int PC = 16;      // pixel rows per workgroup of beam_attn_scores (4 waves x 4 rows)
constexpr int CU = 4;       // encoder rows per wave per load batch of beam_attn_context

template <int KT, bool VEC>
__global__ __launch_bounds__(256) void beam_attn_scores_kernel(int P, int A, const float* __restrict__ att1, Slabs att2,
                                                               const float* __restrict__ bd, const float* __restrict__ w,
                                                               const float* __restrict__ b0, const int* __restrict__ nsrc,
                                                               float* __restrict__ e) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int A4 = (A + 3) & ~3;
    float* ws = sm;             // [A4]
    float* att2s = sm + A4;     // [KT][A4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, p0 = blockIdx.x * PC;
    const int live = min(nsrc[n], KT);
    if (live <= 0) return;      // a finished image: uniform over the workgroup
    const float* rowp[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + wave * 4 + j;
        ok[j] = p < P;
        rowp[j] = att1 + ((long)n * P + (ok[j] ? p : P - 1)) * A;
    }
    for (int a = tid; a < A4; a += 256) {
        const bool in = a < A;
        ws[a] = in ? w[a] : 0.f;
        const float bda = (in && bd) ? bd[a] : 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            att2s[k * A4 + a] = (in && k < live) ? slab_sum(att2.p, (long)(n * KT + k) * att2.ld + a, att2.n, att2.stride) + bda : 0.f;
    }
    __syncthreads();
    float acc[4][KT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[j][k] = 0.f;
    if (VEC) {
        for (int a = lane * 4; a < A; a += 256) {
            const f32x4 ww = *reinterpret_cast<const f32x4*>(ws + a);
            f32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ld4(rowp[j] + a);
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const f32x4 s2 = *reinterpret_cast<const f32x4*>(att2s + k * A4 + a);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[j][k] = fmaf(fmaxf(v[j][c] + s2[c], 0.f), ww[c], acc[j][k]);
            }
        }
    } else {
        for (int a = lane; a < A; a += 64) {
            const float ww = ws[a];
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = rowp[j][a];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float s2 = att2s[k * A4 + a];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j][k] = fmaf(fmaxf(v[j] + s2, 0.f), ww, acc[j][k]);
            }
        }
    }
    const float bias0 = b0 ? b0[0] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const float s = wave_sum(acc[j][k]);
            if (lane == 0 && ok[j] && k < live) e[((long)n * KT + k) * P + p0 + wave * 4 + j] = s + bias0;
        }
}

template <int KT, bool VEC>
__global__ __launch_bounds__(512) void beam_attn_context_kernel(int P, int E, const float* __restrict__ enc,
                                                                const float* __restrict__ e, Slabs gpre,
                                                                const float* __restrict__ bbeta, const int* __restrict__ nsrc,
                                                                float* __restrict__ alpha_out, float* __restrict__ awe,
                                                                float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* part = sm;               // [8][256]
    float* alph = sm + 8 * 256;     // [KT][P]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, e0 = blockIdx.x * 256;
    const int live = min(nsrc[n], KT);
    if (live <= 0) return;
    // wave k: the softmax of slot k (KT <= 8 waves), wave reductions only
    if (wave < KT) {
        float* al = alph + wave * P;
        if (wave < live) {
            const long row = (long)n * KT + wave;
            const float* er = e + row * P;
            float m = -INFINITY;
            for (int p = lane; p < P; p += 64) m = fmaxf(m, er[p]);
            m = wave_max(m);
            float s = 0.f;
            for (int p = lane; p < P; p += 64) {
                const float ex = expf(er[p] - m);
                al[p] = ex;
                s += ex;
            }
            s = wave_sum(s);
            for (int p = lane; p < P; p += 64) {
                const float a = al[p] / s;
                al[p] = a;
                if (blockIdx.x == 0 && alpha_out) alpha_out[row * P + p] = a;
            }
        } else {
            for (int p = lane; p < P; p += 64) al[p] = 0.f;
        }
    }
    __syncthreads();
    const int col = e0 + lane * 4;
    const float* base = enc + (long)n * P * E;
    float acc[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[k][c] = 0.f;
    if (VEC) {
        const int cc = min(col, E - 4);     // columns past E repeat the last fragment; their sums are never stored
        for (int p = wave; p < P; p += 8 * CU) {
            f32x4 v[CU];
#pragma unroll
            for (int j = 0; j < CU; ++j) v[j] = ld4(base + (long)min(p + 8 * j, P - 1) * E + cc);
#pragma unroll
            for (int j = 0; j < CU; ++j) {
                const int pp = p + 8 * j;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float a = pp < P ? alph[k * P + min(pp, P - 1)] : 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[k][c] = fmaf(a, v[j][c], acc[k][c]);
                }
            }
        }
    } else {
        for (int p = wave; p < P; p += 8) {
            float x[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = col + c < E ? base[(long)p * E + col + c] : 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float a = alph[k * P + p];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[k][c] = fmaf(a, x[c], acc[k][c]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < live) {             // uniform over the workgroup
#pragma unroll
            for (int c = 0; c < 4; ++c) part[wave * 256 + lane * 4 + c] = acc[k][c];
            __syncthreads();
            const int c = e0 + tid;
            if (tid < 256 && c < E) {
                float a = part[tid];
#pragma unroll
                for (int w8 = 1; w8 < 8; ++w8) a += part[w8 * 256 + tid];
                const long row = (long)n * KT + k;
                if (awe) awe[row * E + c] = a;
                if (gpre.p) {
                    const float gp = slab_sum(gpre.p, row * gpre.ld + c, gpre.n, gpre.stride) + (bbeta ? bbeta[c] : 0.f);
                    z[row * E + c] = sigmoidf_(gp) * a;
                } else {
                    z[row * E + c] = a;
                }
            }
            __syncthreads();
        }
    }
}

// (value, index) pairs under the search order: larger value first, lower index among equal values
__device__ __forceinline__ bool before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

__device__ __forceinline__ void block_best(float& v, int& i, float* redv, int* redi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if (lane == 0) { redv[wave] = v; redi[wave] = i; }
    __syncthreads();
    v = redv[0]; i = redi[0];
    for (int k = 1; k < nw; ++k)
        if (before(redv[k], redi[k], v, i)) { v = redv[k]; i = redi[k]; }
}

__device__ __forceinline__ float block_sum_max(float v, float* red, bool is_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int k = 1; k < nw; ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
    return r;
}

// ---- the row selection: M decoders, one search state; the single decoder is M = 1, mode 0, w = 1 --------
// elements v0 .. v0+3 of a member's row: one 16-byte load where the row allows it, scalar loads otherwise and for the tail
__device__ __forceinline__ void ens_load4(const float* __restrict__ g, int v0, int V, bool vec, float x[4]) {
    if (vec && v0 + 3 < V) {
        const f32x4 l = ld4(g + v0);
        x[0] = l[0]; x[1] = l[1]; x[2] = l[2]; x[3] = l[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = v0 + c < V ? g[v0 + c] : 0.f;
    }
}

// The log-sum-exp of one member's row g[0 .. V-1]: the maximum over groups of four, the sum over v = tid, tid + 256, ...
// (from LDS when STAGED, else from global memory; that order fixes the bits of lse, the maximum does not depend on its
// order).  STAGED leaves the row in buf; the barriers of the reductions publish it, and the last one also says that every
// thread is done with buf before it is written again.
template <bool STAGED>
__device__ __forceinline__ float ens_row_lse(const float* __restrict__ g, int V, bool vec, float* buf, float* red) {
    const int tid = threadIdx.x, groups = (V + 3) >> 2;
    float mx = -INFINITY;
    for (int q = tid; q < groups; q += 256) {
        float x[4];
        ens_load4(g, q * 4, V, vec, x);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (q * 4 + c < V) {
                if (STAGED) buf[q * 4 + c] = x[c];
                mx = fmaxf(mx, x[c]);
            }
    }
    mx = block_sum_max(mx, red, true);
    const float* src = STAGED ? buf : g;
    float s = 0.f;
    for (int v = tid; v < V; v += 256) s += expf(src[v] - mx);
    s = block_sum_max(s, red, false);
    return mx + logf(s);
}

// c_v from the members' l_mv = x_mv - lse_m.  Products and sums are spelled out (one rounded product, then fused
// multiply-adds in member order), so that the staged and the unstaged kernel compute the same bits -- and, with one member
// of weight 1 in mode 0, exactly x_v - lse.
//   mode 0: sum_m w_m l_mv                                 (weighted geometric mean of the probabilities)
//   mode 1: a + log(sum_m w_m exp(l_mv - a)), a = max_m l_mv      (weighted arithmetic mean; finite when exp(l_mv) underflows)
__device__ __forceinline__ float ens_combine(int M, int mode, const float l[SCN_MAX_ENSEMBLE], const EnsRows& e) {
    if (mode == 0) {
        float c = __fmul_rn(e.w[0], l[0]);
#pragma unroll
        for (int m = 1; m < SCN_MAX_ENSEMBLE; ++m)
            if (m < M) c = fmaf(e.w[m], l[m], c);
        return c;
    }
    float a = l[0];
#pragma unroll
    for (int m = 1; m < SCN_MAX_ENSEMBLE; ++m)
        if (m < M) a = fmaxf(a, l[m]);
    float s = __fmul_rn(e.w[0], expf(l[0] - a));
#pragma unroll
    for (int m = 1; m < SCN_MAX_ENSEMBLE; ++m)
        if (m < M) s = fmaf(e.w[m], expf(l[m] - a), s);
    return a + logf(s);
}

// The M members at the four words of group q: the loads, then c_v of word q*4 + c from them.
struct EnsGroup {
    float x[SCN_MAX_ENSEMBLE][4];
    __device__ __forceinline__ void load(int M, const float* const g[SCN_MAX_ENSEMBLE], int q, int V, unsigned vecmask) {
#pragma unroll
        for (int m = 0; m < SCN_MAX_ENSEMBLE; ++m)
            if (m < M) ens_load4(g[m], q * 4, V, (vecmask >> m) & 1u, x[m]);
    }
    __device__ __forceinline__ float combine(int M, int mode, int c, const float lse[SCN_MAX_ENSEMBLE], const EnsRows& e) const {
        float l[SCN_MAX_ENSEMBLE];
#pragma unroll
        for (int m = 0; m < SCN_MAX_ENSEMBLE; ++m) l[m] = m < M ? x[m][c] - lse[m] : 0.f;
        return ens_combine(M, mode, l, e);
    }
};

// ---- EXCLUSIONS (search options) ----------------------------------------------------------------------------
// LDS words behind the 16 of the reductions: the bitmap of excluded words, then the row's history, both padded to 4
__host__ __device__ inline int excl_bitmap_words(int V) { return (((V + 31) >> 5) + 3) & ~3; }
__host__ __device__ inline int excl_hist_words(int T) { return (T + 3) & ~3; }

__device__ __forceinline__ void excl_set(unsigned* bits, int v, int V) {
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
}
__device__ __forceinline__ bool excl_test(const unsigned* bits, int v) { return (bits[v >> 5] >> (v & 31)) & 1u; }

// The bitmap of the row's excluded words: zeroed, then set from the banned list, <end> before min_length, and -- thread i
// comparing the g-1 words at i with the last g-1 of the history in LDS -- the word that followed every earlier occurrence
// of the open n-gram.  The caller's next barrier completes it.
__device__ __forceinline__ void excl_fill(const BeamExcl& x, long row, int V, unsigned* bits, int* hs) {
    const int tid = threadIdx.x;
    const bool ngram = x.g >= 1 && x.t >= x.g;
    for (int w = tid; w < ((V + 31) >> 5); w += 256) bits[w] = 0u;
    if (ngram)
        for (int i = tid; i < x.t; i += 256) hs[i] = x.hist[row * x.T + i];
    __syncthreads();
    for (int i = tid; i < x.n_banned; i += 256) excl_set(bits, x.banned[i], V);
    if (tid == 0) excl_set(bits, x.end_excl, V);
    if (ngram) {
        const int tail = x.t - x.g + 1;             // the open n-gram: hs[tail .. t-1], g-1 words
        for (int i = tid; i <= x.t - x.g; i += 256) {
            bool same = true;
            for (int q = 0; q < x.g - 1; ++q) same = same && hs[i + q] == hs[tail + q];
            if (same) excl_set(bits, hs[i + x.g - 1], V);
        }
    }
}

struct NoExcl {};       // what the kernel without exclusions takes in place of a BeamExcl: nothing

// One workgroup per live row: per member the log-sum-exp of its row, then K rounds over the candidates score + c_v.  Round r
// takes the best candidate that comes strictly after round r-1's pick in the search order, which is the knock-out without a
// store (and exact on ties: equal values leave in index order).
// STAGED: a member's row passes through LDS for its statistics, then c_v of the whole row is written there once and the K
// rounds run over it.  Otherwise every round recomputes c_v from the M global rows.
// EXCL: the rounds skip the words of the row's bitmap (excl_fill); nothing else differs, so with an empty bitmap the outputs
// are the bits of EXCL = false.  The staged and the unstaged path read the same bitmap.  Without EXCL neither the bitmap nor
// the history takes LDS.
// Kg: the slots per group (K % Kg == 0, nsrc is [N * K/Kg]); Kg = K: no groups, nsrc [N] and the live rows a prefix.
// CON (a constrained search; needs EXCL): once the options' bitmap is complete every thread notes which of
// the image's required words the row may still offer (unmet in the row, not excluded by the options), then the unmet
// required words -- and <end> while one is unmet -- are set in the bitmap as well, so the K rounds run over the row's
// ORDINARY candidates; the 4 required candidates are written from the same expression the rounds use for a word (from buf
// when STAGED, else from EnsGroup::combine: the same bits).  Without CON nothing of this is compiled.
template <bool STAGED, bool EXCL, bool CON = false>
__global__ __launch_bounds__(256) void beam_row_topk_ens_kernel(int K, int Kg, int V, int M, int mode, EnsRows e, unsigned vecmask,
                                                                std::conditional_t<CON, BeamExclCon,
                                                                                   std::conditional_t<EXCL, BeamExcl, NoExcl>> x,
                                                                const float* __restrict__ scores,
                                                                const int* __restrict__ nsrc, float* __restrict__ outv,
                                                                int* __restrict__ outi) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* redv = sm;                               // [4]
    int* redi = reinterpret_cast<int*>(sm + 8);     // [4]
    unsigned* bits = nullptr;                       // [excl_bitmap_words(V)] when EXCL
    float* buf = sm + 16;                           // [V] when STAGED, behind the bitmap and the history [excl_hist_words(T)]
    if constexpr (EXCL) {
        bits = reinterpret_cast<unsigned*>(sm + 16);
        buf += excl_bitmap_words(V) + excl_hist_words(x.T);
    }
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const int n = (int)(row / K), j = (int)(row - (long)n * K);
    const int grp = j / Kg;
    if (j - grp * Kg >= nsrc[n * (K / Kg) + grp]) return;
    const int groups = (V + 3) >> 2;
    const float* g[SCN_MAX_ENSEMBLE];
    float lse[SCN_MAX_ENSEMBLE];
#pragma unroll
    for (int m = 0; m < SCN_MAX_ENSEMBLE; ++m) {
        g[m] = nullptr;
        lse[m] = 0.f;
        if (m < M) {                                // uniform over the workgroup
            g[m] = e.p[m] + row * e.ld[m];
            lse[m] = ens_row_lse<STAGED>(g[m], V, (vecmask >> m) & 1u, buf, redv);
        }
    }
    if constexpr (EXCL) excl_fill(x, row, V, bits, reinterpret_cast<int*>(sm + 16 + excl_bitmap_words(V)));
    int rw[SCN_MAX_REQUIRED];                       // CON: the image's required words, and which of them the row may offer
    unsigned offered = 0;
    if constexpr (CON) {
        const int met = x.c.met[row];
        int full = 0;
#pragma unroll
        for (int c = 0; c < SCN_MAX_REQUIRED; ++c) {
            rw[c] = x.c.req[n * SCN_MAX_REQUIRED + c];
            if (rw[c] >= V) rw[c] = -1;
            if (rw[c] >= 0) full |= 1 << c;
        }
        const int unmet = full & ~met;
        __syncthreads();                            // the options' bitmap is complete
#pragma unroll
        for (int c = 0; c < SCN_MAX_REQUIRED; ++c)
            if (((unmet >> c) & 1) && !excl_test(bits, rw[c])) offered |= 1u << c;
        __syncthreads();                            // ... and read by everyone before the requirements enter it
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < SCN_MAX_REQUIRED; ++c)
                if ((unmet >> c) & 1) excl_set(bits, rw[c], V);
            if (unmet) excl_set(bits, x.c.end_tok, V);      // a caption cannot finish with a requirement open
        }
    }
    if (STAGED) {
        for (int q = tid; q < groups; q += 256) {
            EnsGroup eg;
            eg.load(M, g, q, V, vecmask);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (q * 4 + c < V) buf[q * 4 + c] = eg.combine(M, mode, c, lse, e);
        }
    }
    if (STAGED || EXCL) __syncthreads();            // buf and the bitmap are complete; uniform over the workgroup
    const float sc = scores[row];
    if constexpr (CON) {
        // thread c: required candidate c, the value by the expression of the rounds below
#pragma unroll
        for (int c = 0; c < SCN_MAX_REQUIRED; ++c) {
            if (tid != c) continue;
            float val = -INFINITY;
            int wi = -1;
            if ((offered >> c) & 1u) {
                wi = rw[c];
                if (STAGED) {
                    val = sc + buf[wi];
                } else {
                    EnsGroup eg;
                    eg.load(M, g, wi >> 2, V, vecmask);
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc)
                        if (cc == (wi & 3)) val = sc + eg.combine(M, mode, cc, lse, e);
                }
            }
            x.c.reqv[row * SCN_MAX_REQUIRED + c] = val;
            x.c.reqi[row * SCN_MAX_REQUIRED + c] = wi;
        }
    }
    float pv = INFINITY;
    int pi = -1;
    for (int r = 0; r < K; ++r) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        const auto offer = [&](float val, int v) {
            if ((!EXCL || !excl_test(bits, v)) && before(pv, pi, val, v) && before(val, v, bv, bi)) { bv = val; bi = v; }
        };
        if (STAGED) {
            for (int v = tid; v < V; v += 256) offer(sc + buf[v], v);
        } else {
            for (int q = tid; q < groups; q += 256) {
                EnsGroup eg;
                eg.load(M, g, q, V, vecmask);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (q * 4 + c < V) offer(sc + eg.combine(M, mode, c, lse, e), q * 4 + c);
            }
        }
        block_best(bv, bi, redv, redi);
        if (tid == 0) {
            outv[row * K + r] = bv;
            outi[row * K + r] = bi;
        }
        pv = bv;
        pi = bi;
    }
}

__global__ __launch_bounds__(64) void beam_merge_kernel(int K, int V, int end_tok, int t, const float* __restrict__ candv,
                                                        const int* __restrict__ candi, BeamState s) {
    __shared__ float sv[8];
    __shared__ int sj[8], sw[8];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int ns = s.nsrc[n], k = s.kk[n];
    if (k <= 0) return;         // finished image: a no-op
    const int j = lane / K, r = lane - j * K;
    const bool valid = j < ns;  // ns <= K, so lane < K * K
    const long ci = ((long)n * K + (valid ? j : 0)) * K + r;
    const float v = valid ? candv[ci] : -INFINITY;
    const int w = valid ? candi[ci] : 0;
    const int flat = valid ? j * V + w : INT_MAX;
    int rank = 0;
    for (int l = 0; l < 64; ++l) {
        const float ov = __shfl(v, l, 64);
        const int of = __shfl(flat, l, 64);
        if (of != INT_MAX && before(ov, of, v, flat)) ++rank;
    }
    if (valid && rank < k) { sv[rank] = v; sj[rank] = j; sw[rank] = w; }
    __syncthreads();
    if (lane != 0) return;
    // picks in rank order: <end> picks are recorded as completed, the rest compacted to slots 0 .. nopen-1
    int nopen = 0, nc = s.ncomp[n], bi = s.best_idx[n];
    float bs = s.best_score[n];
    int tok0 = 0, par0 = 0;
    const long r0 = (long)n * K;
    int* token_t = s.token + (long)t * s.R;
    int* parent_t = s.parent + (long)t * s.R;
    for (int q = 0; q < k; ++q) {
        if (sw[q] == end_tok) {
            if (nc < K) {
                s.comp_score[r0 + nc] = sv[q];
                s.comp_step[r0 + nc] = t;
                s.comp_parent[r0 + nc] = sj[q];
                if (bi < 0 || sv[q] > bs) { bs = sv[q]; bi = nc; }     // strictly greater: index(max(...))
                ++nc;
            }
        } else {
            if (nopen == 0) { tok0 = sw[q]; par0 = sj[q]; }
            token_t[r0 + nopen] = sw[q];
            parent_t[r0 + nopen] = sj[q];
            s.scores[r0 + nopen] = sv[q];
            ++nopen;
        }
    }
    for (int d = nopen; d < K; ++d) {       // dead slots: a copy of slot 0 (zeros when nothing is open)
        token_t[r0 + d] = tok0;
        parent_t[r0 + d] = par0;
        s.scores[r0 + d] = 0.f;
    }
    s.ncomp[n] = nc;
    s.best_idx[n] = bi;
    s.best_score[n] = bs;
    s.nsrc[n] = nopen;
    s.kk[n] = nopen;
    if (nopen == 0) atomicAdd(s.open_images, -1);
}

// The merge of a search in G = K / Kg groups: one wave per image walks the groups in order.  Group g owns the
// slots g*Kg .. g*Kg + Kg - 1 of the image and entry n*G + g of nsrc / kk / ncomp / best_idx / best_score; its candidates
// are the nsrc_g x K rows of the row selection (Kg * K <= 64 lanes).  A lane ranks its candidate by
//   a = fmaf(-penalty, c, r),  r = the raw value, c = how many picks of the groups before it at this step carry its word
// under (a descending, flat index j_in_group * V + word ascending); lane 0 then records the kk_g picks as beam_merge_kernel
// does -- with r, not a: nothing of the penalty is stored -- and appends their words, <end> included, to the list in LDS
// (at most K <= 8 words).  A finished group is skipped and penalises nobody.  G = 1: c == 0 and fmaf(-penalty, 0, r) == r,
// so the ranks, and with them every store, are beam_merge_kernel's.
// open_images counts the images with an open group; att_live[n] (when given) is K while image n has one, else 0.
__global__ __launch_bounds__(64) void beam_merge_groups_kernel(int K, int Kg, float penalty, int V, int end_tok, int t,
                                                               const float* __restrict__ candv,
                                                               const int* __restrict__ candi, BeamState s) {
    __shared__ float sv[8];
    __shared__ int sj[8], sw[8];
    __shared__ int pw[8], pc[8];    // the words picked so far at this step, with their counts
    __shared__ int npw;
    const int n = blockIdx.x, lane = threadIdx.x, G = K / Kg;
    if (lane == 0) npw = 0;
    __syncthreads();
    int was_open = 0, still_open = 0;       // lane 0's
    int* token_t = s.token + (long)t * s.R;
    int* parent_t = s.parent + (long)t * s.R;
    for (int g = 0; g < G; ++g) {
        const int sg = n * G + g;
        const int ns = min(s.nsrc[sg], Kg), k = min(s.kk[sg], Kg);
        if (k <= 0) continue;               // a finished group: uniform over the wave
        const int j = lane / K, r = lane - j * K;
        const bool valid = j < ns;          // ns <= Kg, so lane < Kg * K <= 64
        const long ci = ((long)n * K + g * Kg + (valid ? j : 0)) * K + r;
        const float v = valid ? candv[ci] : -INFINITY;
        const int w = valid ? candi[ci] : 0;
        const int flat = valid ? j * V + w : INT_MAX;
        int c = 0;
        for (int i = 0; i < npw; ++i)
            if (pw[i] == w) c = pc[i];
        const float a = valid ? fmaf(-penalty, (float)c, v) : -INFINITY;
        int rank = 0;
        for (int l = 0; l < 64; ++l) {
            const float oa = __shfl(a, l, 64);
            const int of = __shfl(flat, l, 64);
            if (of != INT_MAX && before(oa, of, a, flat)) ++rank;
        }
        if (valid && rank < k) { sv[rank] = v; sj[rank] = j; sw[rank] = w; }
        __syncthreads();
        if (lane == 0) {
            // picks in rank order: <end> picks are recorded as completed, the rest compacted to the group's slots 0 ..
            int nopen = 0, nc = s.ncomp[sg], bi = s.best_idx[sg];
            float bs = s.best_score[sg];
            int tok0 = 0, par0 = 0;
            const long r0 = (long)n * K + g * Kg;
            for (int q = 0; q < k; ++q) {
                if (sw[q] == end_tok) {
                    if (nc < Kg) {
                        s.comp_score[r0 + nc] = sv[q];
                        s.comp_step[r0 + nc] = t;
                        s.comp_parent[r0 + nc] = g * Kg + sj[q];
                        if (bi < 0 || sv[q] > bs) { bs = sv[q]; bi = nc; }     // strictly greater: index(max(...))
                        ++nc;
                    }
                } else {
                    if (nopen == 0) { tok0 = sw[q]; par0 = g * Kg + sj[q]; }
                    token_t[r0 + nopen] = sw[q];
                    parent_t[r0 + nopen] = g * Kg + sj[q];
                    s.scores[r0 + nopen] = sv[q];
                    ++nopen;
                }
                int at = 0;                 // every pick counts, <end> like any other word
                while (at < npw && pw[at] != sw[q]) ++at;
                if (at < npw) {
                    ++pc[at];
                } else if (npw < 8) {
                    pw[npw] = sw[q];
                    pc[npw] = 1;
                    ++npw;
                }
            }
            for (int d = nopen; d < Kg; ++d) {      // dead slots: a copy of the group's slot 0 (zeros when nothing is open)
                token_t[r0 + d] = tok0;
                parent_t[r0 + d] = par0;
                s.scores[r0 + d] = 0.f;
            }
            s.ncomp[sg] = nc;
            s.best_idx[sg] = bi;
            s.best_score[sg] = bs;
            s.nsrc[sg] = nopen;
            s.kk[sg] = nopen;
            was_open = 1;
            still_open |= nopen > 0;
        }
        __syncthreads();                    // the list is complete before the next group counts in it
    }
    if (lane == 0 && was_open && !still_open) {
        atomicAdd(s.open_images, -1);
        if (s.att_live) s.att_live[n] = 0;
    }
}

// The merge of a constrained search: two waves per image, one candidate per thread.  Row j of the image
// brings K + 4 candidates: its K ordinary ones (bank popcount(met_j), the child keeps met_j) and its 4 required ones (entry
// c with a word: bank popcount(met_j) + 1, the child's mask met_j | 1 << c).  A thread ranks its candidate among those of
// its bank by counting through LDS and enters the bank's list when it is among the bank's first K; thread 0 then walks the
// banks round-robin (C_n, C_n - 1, .., 0, and again) for kk picks, puts the picked set into the search order and records it
// exactly as beam_merge_kernel does, with the children's masks.  Every thread has read its row's met before the first
// barrier; thread 0 writes met after the second.  C_n = 0: one bank, nothing required, the stores of beam_merge_kernel.
constexpr int BANK_W = SCN_MAX_BEAM + SCN_MAX_REQUIRED;     // candidates per row at K = 8
constexpr int BANK_NC = SCN_MAX_BEAM * BANK_W;              // 96 candidates per image at most

__global__ __launch_bounds__(128) void beam_merge_banks_kernel(int K, int V, int end_tok, int t, const float* __restrict__ candv,
                                                               const int* __restrict__ candi, const float* __restrict__ reqv,
                                                               const int* __restrict__ reqi, const int* __restrict__ req,
                                                               BeamState s) {
    __shared__ float cv[BANK_NC];
    __shared__ int cf[BANK_NC], cb[BANK_NC], cm[BANK_NC];   // flat index (INT_MAX: no candidate), bank, the child's met
    __shared__ int bl[SCN_MAX_REQUIRED + 1][SCN_MAX_BEAM];  // a bank's first K candidates in the search order (-1: none)
    __shared__ int bp[SCN_MAX_REQUIRED + 1], pk[SCN_MAX_BEAM];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int ns = min(s.nsrc[n], K), k = min(s.kk[n], K);
    if (k <= 0) return;         // finished image: a no-op
    const int W = K + SCN_MAX_REQUIRED, nc = K * W;
    int C = 0;
#pragma unroll
    for (int c = 0; c < SCN_MAX_REQUIRED; ++c) C += req[n * SCN_MAX_REQUIRED + c] >= 0;
    float v = -INFINITY;
    int flat = INT_MAX, bank = 0;
    if (tid < nc) {
        const int j = tid / W, r = tid - j * W;
        int cmet = 0;
        if (j < ns) {
            const long row = (long)n * K + j;
            const int met = s.met[row] & ((1 << SCN_MAX_REQUIRED) - 1);
            if (r < K) {
                v = candv[row * K + r];
                flat = j * V + candi[row * K + r];
                bank = __popc(met);
                cmet = met;
            } else {
                const int c = r - K, w = reqi[row * SCN_MAX_REQUIRED + c];
                if (w >= 0) {
                    v = reqv[row * SCN_MAX_REQUIRED + c];
                    flat = j * V + w;
                    bank = min(__popc(met) + 1, SCN_MAX_REQUIRED);
                    cmet = met | (1 << c);
                }
            }
        }
        cv[tid] = v;
        cf[tid] = flat;
        cb[tid] = bank;
        cm[tid] = cmet;
    }
    if (tid < (SCN_MAX_REQUIRED + 1) * SCN_MAX_BEAM) (&bl[0][0])[tid] = -1;
    if (tid <= SCN_MAX_REQUIRED) bp[tid] = 0;
    __syncthreads();
    if (flat != INT_MAX) {
        int rank = 0;
        for (int l = 0; l < nc; ++l)
            if (cf[l] != INT_MAX && cb[l] == bank && before(cv[l], cf[l], v, flat)) ++rank;
        if (rank < K) bl[bank][rank] = tid;
    }
    __syncthreads();
    if (tid != 0) return;
    int np = 0;
    for (bool any = true; any && np < k;) {         // round-robin over the banks, the highest first
        any = false;
        for (int b = C; b >= 0 && np < k; --b) {
            const int at = bp[b];
            if (at < K && bl[b][at] >= 0) {
                pk[np++] = bl[b][at];
                bp[b] = at + 1;
                any = true;
            }
        }
    }
    for (int a = 1; a < np; ++a) {                  // the picked set in the search order
        const int i = pk[a];
        int q = a;
        while (q > 0 && before(cv[i], cf[i], cv[pk[q - 1]], cf[pk[q - 1]])) { pk[q] = pk[q - 1]; --q; }
        pk[q] = i;
    }
    // picks in that order: <end> picks are recorded as completed, the rest compacted to slots 0 .. nopen-1
    int nopen = 0, ncp = s.ncomp[n], bi = s.best_idx[n];
    float bs = s.best_score[n];
    int tok0 = 0, par0 = 0, met0 = 0;
    const long r0 = (long)n * K;
    int* token_t = s.token + (long)t * s.R;
    int* parent_t = s.parent + (long)t * s.R;
    for (int q = 0; q < np; ++q) {
        const int i = pk[q], j = i / W, w = cf[i] - j * V;
        if (w == end_tok) {
            if (ncp < K) {
                s.comp_score[r0 + ncp] = cv[i];
                s.comp_step[r0 + ncp] = t;
                s.comp_parent[r0 + ncp] = j;
                if (bi < 0 || cv[i] > bs) { bs = cv[i]; bi = ncp; }     // strictly greater: index(max(...))
                ++ncp;
            }
        } else {
            if (nopen == 0) { tok0 = w; par0 = j; met0 = cm[i]; }
            token_t[r0 + nopen] = w;
            parent_t[r0 + nopen] = j;
            s.scores[r0 + nopen] = cv[i];
            s.met[r0 + nopen] = cm[i];
            ++nopen;
        }
    }
    for (int d = nopen; d < K; ++d) {       // dead slots: a copy of slot 0 (zeros when nothing is open)
        token_t[r0 + d] = tok0;
        parent_t[r0 + d] = par0;
        s.scores[r0 + d] = 0.f;
        s.met[r0 + d] = met0;
    }
    s.ncomp[n] = ncp;
    s.best_idx[n] = bi;
    s.best_score[n] = bs;
    s.nsrc[n] = nopen;
    s.kk[n] = nopen;
    if (nopen == 0) atomicAdd(s.open_images, -1);
}

// h / c gathered from the parent slot, the next input embedding from the table.  With hist_d (search options): also the
// row's history for step t+1, the parent slot's t words of hist_s, then this step's word.  A dead slot carries slot 0's
// parent / token records, so it gets slot 0's history.
__global__ __launch_bounds__(256) void beam_advance_kernel(int K, int D, int M, int V, int t, int T,
                                                           const float* __restrict__ hs, const float* __restrict__ cs,
                                                           const int* __restrict__ parent_t, const int* __restrict__ token_t,
                                                           const float* __restrict__ table, const int* __restrict__ hist_s,
                                                           int* __restrict__ hist_d, float* __restrict__ hd,
                                                           float* __restrict__ cd, float* __restrict__ emb) {
    const long row = blockIdx.x;
    const long n = row / K;
    const long src = n * K + min(max(parent_t[row], 0), K - 1);     // an index outside the image's slots cannot leave them
    const long tok = min(max(token_t[row], 0), V - 1);
    for (int d = threadIdx.x; d < D; d += 256) {
        hd[row * D + d] = hs[src * D + d];
        cd[row * D + d] = cs[src * D + d];
    }
    for (int m = threadIdx.x; m < M; m += 256) emb[row * M + m] = table[tok * M + m];
    if (!hist_d) return;                            // uniform over the grid
    for (int i = threadIdx.x; i < t; i += 256) hist_d[row * T + i] = hist_s[src * T + i];
    if (threadIdx.x == 0) hist_d[row * T + t] = (int)tok;
}

// out[n*K + j][:] = in[n][:]
__global__ __launch_bounds__(256) void beam_expand_rows_kernel(long total, int K, int W, const float* __restrict__ in,
                                                               float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / W;
    out[i] = in[(row / K) * W + (i - row * W)];
}

// G groups per image (1: no groups): the per-group arrays hold N*G entries, each group with K/G beams to fill
__global__ __launch_bounds__(256) void beam_state_init_kernel(int N, int K, int G, BeamState s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < s.R) {
        s.scores[i] = 0.f;
        s.comp_score[i] = 0.f;
        s.comp_step[i] = -1;
        s.comp_parent[i] = 0;
    }
    if (i < N * G) {
        s.nsrc[i] = 1;          // the reference selects from scores[0] only at step 1
        s.kk[i] = K / G;
        s.ncomp[i] = 0;
        s.best_idx[i] = -1;
        s.best_score[i] = 0.f;
    }
    if (i < N && s.att_live) s.att_live[i] = K;
    if (i == 0) s.open_images[0] = N;
}

inline bool vec_ok(const float* p, int W) { return W % 4 == 0 && W >= 4 && aligned16(p); }

}  // namespace

#define SCN_BEAM_K_SWITCH(LAUNCH)                                                                             \
    switch (K) {                                                                                              \
        case 1: LAUNCH(1) break; case 2: LAUNCH(2) break; case 3: LAUNCH(3) break; case 4: LAUNCH(4) break;   \
        case 5: LAUNCH(5) break; case 6: LAUNCH(6) break; case 7: LAUNCH(7) break; default: LAUNCH(8) break;  \
    }

int beam_attn_scores(hipStream_t st, int N, int K, int P, int A, const float* att1, Slabs att2, const float* bd,
                     const float* w, const float* b0, const int* nsrc, float* e) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM, "beam_attn_scores: beam size out of range");
    SCN_ARG(att1 && att2.p && w && nsrc && e && P > 0 && A > 0, "beam_attn_scores: bad argument");
    const size_t lds = (size_t)(K + 1) * ((A + 3) & ~3) * sizeof(float);
    SCN_ARG(lds <= 64 * 1024, "beam_attn_scores: attention_dim too large for the LDS staging");
    dim3 grid(cdiv(P, PC), N), block(256);
    const bool vec = vec_ok(att1, A);
#define L(KT)                                                                                                        \
    if (vec) hipLaunchKernelGGL((beam_attn_scores_kernel<KT, true>), grid, block, lds, st, P, A, att1, att2, bd, w, b0, nsrc, e);  \
    else     hipLaunchKernelGGL((beam_attn_scores_kernel<KT, false>), grid, block, lds, st, P, A, att1, att2, bd, w, b0, nsrc, e);
    SCN_BEAM_K_SWITCH(L)
#undef L
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_attn_context(hipStream_t st, int N, int K, int P, int E, const float* enc, const float* e, Slabs gpre,
                      const float* bbeta, const int* nsrc, float* alpha_out, float* awe, float* z) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM, "beam_attn_context: beam size out of range");
    SCN_ARG(enc && e && nsrc && z && P > 0 && E > 0, "beam_attn_context: bad argument");
    const size_t lds = (size_t)(8 * 256 + (long)K * P) * sizeof(float);
    SCN_ARG(lds <= 64 * 1024, "beam_attn_context: num_pixels too large for the LDS staging");
    dim3 grid(cdiv(E, 256), N), block(512);
    const bool vec = vec_ok(enc, E);
#define L(KT)                                                                                                                    \
    if (vec) hipLaunchKernelGGL((beam_attn_context_kernel<KT, true>), grid, block, lds, st, P, E, enc, e, gpre, bbeta, nsrc, alpha_out, awe, z);  \
    else     hipLaunchKernelGGL((beam_attn_context_kernel<KT, false>), grid, block, lds, st, P, E, enc, e, gpre, bbeta, nsrc, alpha_out, awe, z);
    SCN_BEAM_K_SWITCH(L)
#undef L
    SCN_LAUNCH_CHECK();
    return 0;
}

// The one launcher of the selection; x: what the step excludes, null: nothing.
int beam_row_topk_ens(hipStream_t st, int N, int K, int V, int M, const EnsRows& e, int mode, const float* scores,
                      const int* nsrc, const BeamExcl* x, float* outv, int* outi, int force_passes, int Kg,
                      const BeamCon* cn) {
    if (N <= 0) return 0;
    SCN_ARG(M >= 1 && M <= SCN_MAX_ENSEMBLE, "beam_row_topk_ens: need 1 <= members <= 4");
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K, "beam_row_topk_ens: need 1 <= beam size <= 8 and vocab_size >= beam size");
    if (Kg == 0) Kg = K;
    SCN_ARG(Kg >= 1 && K % Kg == 0, "beam_row_topk_ens: the slots per group must divide the beam size");
    SCN_ARG(mode == 0 || mode == 1, "beam_row_topk_ens: mode must be 0 (logprob) or 1 (prob)");
    SCN_ARG(scores && nsrc && outv && outi, "beam_row_topk_ens: null argument");
    if (x) {
        SCN_ARG(x->T >= 1 && x->T <= 4096 && x->t >= 0 && x->t <= x->T, "beam_row_topk_ens: need 0 <= t <= max_steps <= 4096");
        SCN_ARG(x->g >= 0 && x->g <= SCN_MAX_NGRAM, "beam_row_topk_ens: no_repeat_ngram must be in [0, 8]");
        SCN_ARG(x->n_banned >= 0 && x->n_banned <= SCN_MAX_BANNED, "beam_row_topk_ens: at most 64 banned tokens");
        for (int i = 0; i < x->n_banned; ++i)
            SCN_ARG(x->banned[i] >= 0 && x->banned[i] < V, "beam_row_topk_ens: a banned token lies outside the vocabulary");
        SCN_ARG(x->end_excl >= -1 && x->end_excl < V, "beam_row_topk_ens: the end token lies outside the vocabulary");
        SCN_ARG(x->g == 0 || x->hist, "beam_row_topk_ens: no_repeat_ngram needs the history");
        SCN_ARG((long)V - x->n_banned - 1 - (x->g >= 1 ? x->T : 0) >= K,
                "beam_row_topk_ens: the options may leave a row fewer than beam_size candidates "
                "(need vocab_size - banned - 1 - (no_repeat_ngram ? max_steps : 0) >= beam_size)");
    }
    if (cn) {
        SCN_ARG(x, "beam_row_topk_ens: the constraints need the exclusions (which may exclude nothing)");
        SCN_ARG(Kg == K, "beam_row_topk_ens: constraints and groups do not compose");
        SCN_ARG(cn->req && cn->met && cn->reqv && cn->reqi, "beam_row_topk_ens: null constraint operand");
        SCN_ARG(cn->end_tok >= 0 && cn->end_tok < V, "beam_row_topk_ens: the end token lies outside the vocabulary");
        SCN_ARG((long)V - x->n_banned - 1 - (x->g >= 1 ? x->T : 0) - SCN_MAX_REQUIRED >= K,
                "beam_row_topk_ens: options and required words may leave a row fewer than beam_size candidates "
                "(need vocab_size - banned - 1 - (no_repeat_ngram ? max_steps : 0) - 4 >= beam_size)");
    }
    unsigned vecmask = 0;
    for (int m = 0; m < M; ++m) {
        SCN_ARG(e.p[m] && e.ld[m] >= V, "beam_row_topk_ens: a member's logits are null or its leading dimension < vocab_size");
        SCN_ARG(e.w[m] > 0.f && e.w[m] < INFINITY, "beam_row_topk_ens: member weights must be positive and finite");
        if (aligned16(e.p[m]) && e.ld[m] % 4 == 0) vecmask |= 1u << m;
    }
    // LDS: the reductions, with exclusions the bitmap and the history, and the row itself when that still fits (STAGED)
    const size_t fixed = (size_t)(16 + (x ? excl_bitmap_words(V) + excl_hist_words(x->T) : 0)) * sizeof(float);
    const size_t staged = fixed + (size_t)V * sizeof(float);
    SCN_ARG(fixed <= 64 * 1024, "beam_row_topk_ens: vocab_size too large for the exclusion bitmap in LDS");
    const bool stage = staged <= 64 * 1024 && !force_passes;
    const size_t lds = stage ? staged : fixed;
    dim3 grid(N * K), block(256);
#define L(STAGED)                                                                                                             \
    if (cn) {                                                                                                                 \
        BeamExclCon xc;                                                                                                       \
        static_cast<BeamExcl&>(xc) = *x;                                                                                      \
        xc.c = *cn;                                                                                                           \
        hipLaunchKernelGGL((beam_row_topk_ens_kernel<STAGED, true, true>), grid, block, lds, st, K, Kg, V, M, mode, e,        \
                           vecmask, xc, scores, nsrc, outv, outi);                                                            \
    } else                                                                                                                    \
    if (x) hipLaunchKernelGGL((beam_row_topk_ens_kernel<STAGED, true>), grid, block, lds, st, K, Kg, V, M, mode, e, vecmask,   \
                              *x, scores, nsrc, outv, outi);                                                                  \
    else   hipLaunchKernelGGL((beam_row_topk_ens_kernel<STAGED, false>), grid, block, lds, st, K, Kg, V, M, mode, e, vecmask,  \
                              NoExcl{}, scores, nsrc, outv, outi);
    if (stage) { L(true) } else { L(false) }
#undef L
    SCN_LAUNCH_CHECK();
    return 0;
}

// The single decoder's selection: one member of weight 1 in mode 0, whose c_v is logits[row][v] - lse(row) to the bit.
int beam_row_topk(hipStream_t st, int N, int K, int V, const float* logits, long ld, const float* scores, const int* nsrc,
                  float* outv, int* outi, int force_passes) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K, "beam_row_topk: need 1 <= beam size <= 8 and vocab_size >= beam size");
    SCN_ARG(logits && scores && nsrc && outv && outi && ld >= V, "beam_row_topk: bad argument");
    return beam_row_topk_ens(st, N, K, V, 1, EnsRows{{logits}, {ld}, {1.f}}, 0, scores, nsrc, nullptr, outv, outi, force_passes);
}

int beam_merge(hipStream_t st, int N, int K, int V, int end_tok, int t, const float* candv, const int* candi,
               const BeamState& s) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K && t >= 0, "beam_merge: bad beam size / step");
    SCN_ARG((long)K * V < INT_MAX, "beam_merge: beam size x vocab_size overflows the flat index");
    SCN_ARG(candv && candi && s.R == N * K && s.scores && s.nsrc && s.kk && s.ncomp && s.best_idx && s.best_score &&
                s.open_images && s.comp_score && s.comp_step && s.comp_parent && s.token && s.parent,
            "beam_merge: bad argument");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(N), dim3(64), 0, st, K, V, end_tok, t, candv, candi, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_merge_banks(hipStream_t st, int N, int K, int V, int end_tok, int t, const float* candv, const int* candi,
                     const float* reqv, const int* reqi, const int* req, const BeamState& s) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K && t >= 0, "beam_merge_banks: bad beam size / step");
    SCN_ARG((long)K * V < INT_MAX, "beam_merge_banks: beam size x vocab_size overflows the flat index");
    SCN_ARG(candv && candi && reqv && reqi && req && s.R == N * K && s.scores && s.nsrc && s.kk && s.ncomp && s.best_idx &&
                s.best_score && s.open_images && s.comp_score && s.comp_step && s.comp_parent && s.token && s.parent && s.met,
            "beam_merge_banks: bad argument");
    hipLaunchKernelGGL(beam_merge_banks_kernel, dim3(N), dim3(128), 0, st, K, V, end_tok, t, candv, candi, reqv, reqi, req, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_merge_groups(hipStream_t st, int N, int K, int Kg, float penalty, int V, int end_tok, int t, const float* candv,
                      const int* candi, const BeamState& s) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K && t >= 0, "beam_merge_groups: bad beam size / step");
    SCN_ARG(Kg >= 1 && K % Kg == 0, "beam_merge_groups: the slots per group must divide the beam size");
    SCN_ARG(penalty >= 0.f && penalty < INFINITY, "beam_merge_groups: the penalty must be finite and not negative");
    SCN_ARG((long)K * V < INT_MAX, "beam_merge_groups: beam size x vocab_size overflows the flat index");
    SCN_ARG(candv && candi && s.R == N * K && s.scores && s.nsrc && s.kk && s.ncomp && s.best_idx && s.best_score &&
                s.open_images && s.comp_score && s.comp_step && s.comp_parent && s.token && s.parent,
            "beam_merge_groups: bad argument");
    hipLaunchKernelGGL(beam_merge_groups_kernel, dim3(N), dim3(64), 0, st, K, Kg, penalty, V, end_tok, t, candv, candi, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_advance(hipStream_t st, int N, int K, int D, int M, int V, const float* hs, const float* cs, const int* parent_t,
                 const int* token_t, const float* table, float* hd, float* cd, float* emb) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && D > 0 && M > 0 && V > 0, "beam_advance: bad dims");
    SCN_ARG(hs && cs && parent_t && token_t && table && hd && cd && emb, "beam_advance: null operand");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(N * K), dim3(256), 0, st, K, D, M, V, 0, 0, hs, cs, parent_t, token_t, table,
                       nullptr, nullptr, hd, cd, emb);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_advance_opt(hipStream_t st, int N, int K, int D, int M, int V, int t, int T, const float* hs, const float* cs,
                     const int* parent_t, const int* token_t, const float* table, const int* hist_s, int* hist_d, float* hd,
                     float* cd, float* emb) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && D > 0 && M > 0 && V > 0, "beam_advance_opt: bad dims");
    SCN_ARG(T >= 1 && t >= 0 && t < T, "beam_advance_opt: need 0 <= t < max_steps");
    SCN_ARG(hs && cs && parent_t && token_t && table && hist_s && hist_d && hist_s != hist_d && hd && cd && emb,
            "beam_advance_opt: null operand (or the history gathered in place)");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(N * K), dim3(256), 0, st, K, D, M, V, t, T, hs, cs, parent_t, token_t, table,
                       hist_s, hist_d, hd, cd, emb);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_expand_rows(hipStream_t st, int N, int K, int W, const float* in, float* out) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && W > 0 && in && out, "beam_expand_rows: bad argument");
    const long total = (long)N * K * W;
    hipLaunchKernelGGL(beam_expand_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, total, K, W, in, out);
    SCN_LAUNCH_CHECK();
    return 0;
}

int beam_state_init(hipStream_t st, int N, int K, const BeamState& s, int G) {
    SCN_ARG(N > 0 && K >= 1 && K <= SCN_MAX_BEAM && s.R == N * K, "beam_state_init: bad argument");
    SCN_ARG(G >= 1 && K % G == 0, "beam_state_init: the groups must divide the beam size");
    hipLaunchKernelGGL(beam_state_init_kernel, dim3(cdiv(s.R > N ? s.R : N, 256)), dim3(256), 0, st, N, K, G, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace scn
