// Sampled rollouts for self-critical training: one token per row from a row of logits, on the device.
// K slots per image, rows r = n*K + j as in csrc/beam.hip, but slots are independent captions: nothing is compacted and
// the state carries over slot for slot.  fp32 only, like the search.
//   rollout_pick     one workgroup per row, ONE pass over the row's V logits.  With y_v = logits[r][v] * inv_temp:
//                      key_v  = y_v + noisy_j * g_v          noisy_j = 0 for the arg-max slot (greedy_first and j == 0), else 1
//                      g_v    = -log(-log(u_v))              Gumbel noise: arg-max of the keys is a draw from softmax(y)
//                      u_v    = ((bits_v >> 9) + 0.5) * 2^-23      exact in fp32, strictly inside (0, 1)
//                      bits_v = word (v & 3) of Philox4x32-10 with key (seed low half, seed high half) and
//                               counter (v >> 2, r, t, draw)
//                    so a token's noise depends on (seed, draw, r, t, v) alone, not on the launch geometry.
//                      token[r] = the first key in the order (value descending, index ascending): the TIE RULE of beam.hip
//                      logp[r]  = y_token - logsumexp(y): the log-probability under the distribution that was sampled,
//                                 from an online max / sum in the same pass
//                    Book-keeping by the row's first thread: the records of step t, sum_logp[r] += logp, and on <end>
//                    length[r] = t + 1, nopen[n] -= 1, open_rows -= 1 (vector atomics).  length[r] == 0 means open.
//                    A row of an image with nsrc[n] == 0 is neither read nor written; a closed row of an open image only
//                    gets the records token = 0 (<pad>), logp = 0.0.  nsrc is read-only here, so no workgroup depends on
//                    what another one does in the same launch.
//   rollout_pick_filtered  the same pick inside the top-k / nucleus set of the row (further down): the cut by
//                    bisection on the order-preserving integer image of y, counts and fp64 masses, then one keyed pass.
//   rollout_score    the pick TOLD its token (scoring given captions; further down): the token's
//                    log-probability, its rank in the row and the row's first word, the row closing after its last given token.
//   rollout_pick_mixed  scheduled sampling (further down): a coin per (row, step) decides between the gold word
//                    it is told and rollout_pick's own pick; the gold length alone closes the row.
//   rollout_advance  the next input embedding of every row (the token record clamped into the table) and, per image,
//                    nsrc[n] = nopen[n] > 0 ? K : 0 for the attention kernels of the next step.
// The arg-max slot skips the noise: key_v = y_v exactly.  Plain vector loads and stores; no kernel waits for another
// workgroup; no inline assembly.
#include <climits>
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace scn {

namespace {

__device__ __forceinline__ float gumbel(unsigned bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * 0x1p-23f;      // 24 significant bits: exact
    return -logf(-logf(u));
}

// the running state of a thread / a wave / the row: online softmax of y and the first key in the order
struct Pick {
    float m, s;         // max of y, sum of exp(y - m)
    float bk, by;       // best key and the y behind it
    int bi;
    __device__ __forceinline__ void see(float y, float key, int v) {
        if (y > m) {
            s = s * expf(m - y) + 1.f;
            m = y;
        } else {
            s += y == -INFINITY ? 0.f : expf(y - m);
        }
        if (key > bk || (key == bk && v < bi)) { bk = key; by = y; bi = v; }
    }
    __device__ __forceinline__ void merge(float m2, float s2, float bk2, float by2, int bi2) {
        const float mm = fmaxf(m, m2);
        s = (m == -INFINITY ? 0.f : s * expf(m - mm)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mm));
        m = mm;
        if (bk2 > bk || (bk2 == bk && bi2 < bi)) { bk = bk2; by = by2; bi = bi2; }
    }
};

// The pick of row r at step t, by the whole workgroup in ONE pass over x[0 .. V): the row's Pick is complete in thread 0
// alone, and only for thread 0 does this return true.  Every thread of the workgroup must call it (it synchronises).
template <bool VEC>
__device__ __forceinline__ bool pick_row(const float* __restrict__ x, int V, float inv_temp, bool noisy, int r, int t,
                                         unsigned draw, unsigned k0, unsigned k1, Pick& p) {
    p = Pick{-INFINITY, 0.f, -INFINITY, 0.f, INT_MAX};
    const int groups = (V + 3) >> 2;
    for (int q = threadIdx.x; q < groups; q += 256) {
        const int v0 = q * 4;
        float e[4];
        if (VEC && v0 + 3 < V) {
            const f32x4 l = ld4(x + v0);
            e[0] = l[0]; e[1] = l[1]; e[2] = l[2]; e[3] = l[3];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) e[c] = v0 + c < V ? x[v0 + c] : 0.f;
        }
        u32q b = {{0u, 0u, 0u, 0u}};
        if (noisy) b = philox4x32_10((unsigned)q, (unsigned)r, (unsigned)t, draw, k0, k1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (v0 + c < V) {
                const float y = e[c] * inv_temp;
                p.see(y, noisy ? y + gumbel(b.w[c]) : y, v0 + c);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        p.merge(__shfl_xor(p.m, o, 64), __shfl_xor(p.s, o, 64), __shfl_xor(p.bk, o, 64), __shfl_xor(p.by, o, 64),
                __shfl_xor(p.bi, o, 64));
    __shared__ float sm[4], ss[4], sk[4], sy[4];
    __shared__ int si[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w] = p.m; ss[w] = p.s; sk[w] = p.bk; sy[w] = p.by; si[w] = p.bi; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    p = Pick{sm[0], ss[0], sk[0], sy[0], si[0]};
    p.merge(sm[1], ss[1], sk[1], sy[1], si[1]);
    p.merge(sm[2], ss[2], sk[2], sy[2], si[2]);
    p.merge(sm[3], ss[3], sk[3], sy[3], si[3]);
    return true;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rollout_pick_kernel(int K, int V, const float* __restrict__ logits, long ld,
                                                           float inv_temp, unsigned k0, unsigned k1, unsigned draw, int t,
                                                           int greedy_first, int end_tok, RolloutState s) {
    const int r = blockIdx.x, n = r / K, j = r - n * K;
    if (s.nsrc[n] <= 0) return;                 // a closed image: uniform over the workgroup
    int* token_t = s.token + (long)t * s.R;
    float* logp_t = s.logp + (long)t * s.R;
    if (s.length[r] != 0) {                     // a closed row of an open image
        if (threadIdx.x == 0) { token_t[r] = 0; logp_t[r] = 0.f; }
        return;
    }
    Pick p;
    if (!pick_row<VEC>(logits + (long)r * ld, V, inv_temp, !(greedy_first && j == 0), r, t, draw, k0, k1, p)) return;
    const bool found = p.bi < V;                // a row of NaN alone has no first element: <pad>, and its logp is NaN
    const int tok = found ? p.bi : 0;
    const float lp = found ? p.by - (p.m + logf(p.s)) : __builtin_nanf("");
    token_t[r] = tok;
    logp_t[r] = lp;
    s.sum_logp[r] += lp;
    if (tok == end_tok) {
        s.length[r] = t + 1;
        atomicAdd(s.nopen + n, -1);
        atomicAdd(s.open_rows, -1);
    }
}

__global__ __launch_bounds__(256) void rollout_advance_kernel(int K, int M, int V, const int* __restrict__ token_t,
                                                              const float* __restrict__ table, float* __restrict__ emb,
                                                              const int* __restrict__ nopen, int* __restrict__ nsrc) {
    const long row = blockIdx.x;
    const long tok = min(max(token_t[row], 0), V - 1);       // a record that was never written cannot leave the table
    for (int m = threadIdx.x; m < M; m += 256) emb[row * M + m] = table[tok * M + m];
    const long n = row / K;
    if (row == n * K && threadIdx.x == 0) nsrc[n] = nopen[n] > 0 ? K : 0;
}

__global__ __launch_bounds__(256) void rollout_state_init_kernel(int N, int K, RolloutState s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < s.R) {
        s.length[i] = 0;
        s.sum_logp[i] = 0.f;
    }
    if (i < N) {
        s.nsrc[i] = K;
        s.nopen[i] = K;
    }
    if (i == 0) s.open_rows[0] = s.R;
}

// ---- the filtered pick (top-k / nucleus; the contract: include/scnattn.h) ---------------------------------
// The kept set is a prefix of the ORDER (y descending, index ascending), so it is described by two numbers: the image T of
// the value at the cut and the index I of the last kept word among those equal to it.  With img() the order-preserving
// unsigned image of y (-0 taken as +0), C(T) = #{v: img_v >= T} and A(T) = sum of e_v over the same words (fp64),
//      enough(T) = C(T) >= L_k  or  A(T) >= top_p * A(0)
// is monotone in T (an fp64 sum in a fixed order only grows when non-negative terms are inserted), so the largest T that
// is enough is found bit by bit, 32 workgroup reductions, without sorting the row.  The words above T are then too few and
// too light; those equal to T all carry the same e_T, and are taken in index order: j, the smallest count with
// A_gt + j * e_T >= top_p * A(0), and the index of the (nkeep - C_gt)-th of them by bisection on the index.
// EVERY sum is the same reduction: thread i adds its words (the groups of four q = i, i + 256, ..., words 4q .. 4q + 3) in
// that order, a wave adds its lanes as a butterfly (all lanes end with the same bits), and the four waves are added
// 0, 1, 2, 3.  No atomics on floating point.  A row of up to 10240 words stays in registers between the passes (as images
// and terms: 80 registers per thread at V = 10000, where a copy in LDS cost a latency-bound loop per pass and four times
// the time); LDS holds the reductions only.  Longer rows are re-read from global memory in every pass.
__device__ __forceinline__ unsigned img_of(float y) {
    const unsigned u = __float_as_uint(y == 0.f ? 0.f : y);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float y_of(unsigned img) {
    return __uint_as_float((img & 0x80000000u) ? (img ^ 0x80000000u) : ~img);
}

struct Tally {
    int a, b;           // two counts
    double s;           // one mass
};
// red: 4 Tally of LDS.  Every thread returns the workgroup's total (the same bits in all of them).
__device__ __forceinline__ Tally tally_all(Tally x, Tally* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x.a += __shfl_xor(x.a, o, 64);
        x.b += __shfl_xor(x.b, o, 64);
        x.s += __shfl_xor(x.s, o, 64);
    }
    __syncthreads();                            // the previous round's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    Tally r = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { r.a += red[w].a; r.b += red[w].b; r.s += red[w].s; }
    return r;
}

// NPT4 > 0: the row is HELD IN REGISTERS for all passes, NPT4 groups of four words per thread (thread i owns the groups
// q = i, i + 256, ...: the words 4q .. 4q + 3, the group that shares one Philox call), as the image of y and the term e.
// NPT4 == 0: every pass re-reads the logits from global memory and forms y and e again (one fp32 product, one expf: the same
// bits every time), in the same ownership, so both forms add the same numbers in the same order.
template <int NPT4, bool VEC>
__global__ __launch_bounds__(256) void rollout_pick_filtered_kernel(int K, int V, const float* __restrict__ logits, long ld,
                                                                    float inv_temp, unsigned k0, unsigned k1, unsigned draw,
                                                                    int t, int greedy_first, int end_tok, int Lk, float top_p,
                                                                    int* __restrict__ nkeep_t, RolloutState s) {
    const int r = blockIdx.x, n = r / K, j = r - n * K;
    if (s.nsrc[n] <= 0) return;                 // a closed image: uniform over the workgroup
    int* token_t = s.token + (long)t * s.R;
    float* logp_t = s.logp + (long)t * s.R;
    if (s.length[r] != 0) {                     // a closed row of an open image
        if (threadIdx.x == 0) { token_t[r] = 0; logp_t[r] = 0.f; nkeep_t[r] = 0; }
        return;
    }
    __shared__ Tally red[4];
    __shared__ unsigned redu[4];
    __shared__ float sy[4];
    const float* x = logits + (long)r * ld;
    const int tid = threadIdx.x;
    const bool use_p = top_p < 1.f;
    const int groups = (V + 3) >> 2;
    constexpr int NR = NPT4 > 0 ? NPT4 * 4 : 1;
    unsigned ir[NR];                            // images; 0 for a slot beyond V (below every real number's image)
    float er[NR];

    // the maximum (as an image: exact, any order), and the row into registers
    unsigned mx = 0u;
    if constexpr (NPT4 > 0) {
#pragma unroll
        for (int g = 0; g < NPT4; ++g) {
            const int v0 = (tid + 256 * g) * 4;
            float y4[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC && v0 + 3 < V) {
                const f32x4 l = ld4(x + v0);
                y4[0] = l[0]; y4[1] = l[1]; y4[2] = l[2]; y4[3] = l[3];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (v0 + c < V) y4[c] = x[v0 + c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ir[4 * g + c] = v0 + c < V ? img_of(y4[c] * inv_temp) : 0u;
                mx = max(mx, ir[4 * g + c]);
            }
        }
    } else {
        for (int q = tid; q < groups; q += 256)
            for (int v = 4 * q; v < min(4 * q + 4, V); ++v) mx = max(mx, img_of(x[v] * inv_temp));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    if ((tid & 63) == 0) redu[tid >> 6] = mx;
    __syncthreads();
    mx = max(max(redu[0], redu[1]), max(redu[2], redu[3]));
    const float m = y_of(mx);

    // e_v = expf(fl(y_v - m)), 0 for y_v = -inf
    auto e_of = [&](float y) { return y == -INFINITY ? 0.f : expf(y - m); };
    if constexpr (NPT4 > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) er[i] = use_p && ir[i] != 0u ? e_of(y_of(ir[i])) : 0.f;
    }
    // f(v, image, e) for every word of this thread, in its fixed order
    auto each = [&](auto f) {
        if constexpr (NPT4 > 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) f((tid + 256 * (i >> 2)) * 4 + (i & 3), ir[i], er[i]);
        } else {
            for (int q = tid; q < groups; q += 256)
                for (int v = 4 * q; v < min(4 * q + 4, V); ++v) {
                    const float y = x[v] * inv_temp;
                    f(v, img_of(y), use_p ? e_of(y) : 0.f);
                }
        }
    };
    // the tally of the words whose image is >= T
    auto tally_ge = [&](unsigned T) {
        Tally a = {0, 0, 0.0};
        each([&](int v, unsigned im, float e) {
            if (im >= T && v < V) {
                a.a += 1;
                a.s += (double)e;
            }
        });
        return tally_all(a, red);
    };
    double need = 0.0;                          // top_p * the whole mass, in fp64
    if (use_p) need = (double)top_p * tally_ge(0u).s;
    unsigned T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = T | (1u << bit);
        if (cand > mx) continue;                // nothing up there: not enough (uniform)
        const Tally c = tally_ge(cand);
        if (c.a >= Lk || (use_p && c.s >= need)) T = cand;
    }
    // above the cut value (too few, too light) and equal to it
    Tally g = {0, 0, 0.0};
    each([&](int v, unsigned im, float e) {
        if (v < V) {
            if (im > T) {
                g.a += 1;
                g.s += (double)e;
            } else if (im == T) {
                g.b += 1;
            }
        }
    });
    g = tally_all(g, red);
    const int c_gt = g.a, n_tie = g.b;
    int jp = n_tie;
    if (use_p) {
        const double eT = (double)e_of(y_of(T));
        const double q = (need - g.s) / eT;
        jp = q >= (double)n_tie ? n_tie : (q >= 1.0 ? (int)ceil(q) : 1);      // NaN: 1
        for (int i = 0; i < 4 && jp > 1 && g.s + (double)(jp - 1) * eT >= need; ++i) --jp;
        for (int i = 0; i < 4 && jp < n_tie && g.s + (double)jp * eT < need; ++i) ++jp;
    }
    int nkeep = min(Lk, c_gt + jp);
    nkeep = max(nkeep, min(c_gt + 1, V));       // never empty (a row with a NaN can confuse the counts; it stays in bounds)
    const int c = nkeep - c_gt;                 // how many of the words equal to the cut value are kept: the first c
    int last = V - 1;                           // the index of the c-th of them
    if (c < n_tie) {
        int lo = 0, hi = V - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            Tally a = {0, 0, 0.0};
            each([&](int v, unsigned im, float) { a.a += im == T && v <= mid; });
            a = tally_all(a, red);
            if (a.a >= c) hi = mid; else lo = mid + 1;
        }
        last = lo;
    }

    // one pass over the kept words: the first key in the order and the kept mass
    const bool noisy = !(greedy_first && j == 0);
    float bk = -INFINITY, by = 0.f;
    int bi = INT_MAX;
    double sk = 0.0;
    auto group = [&](int q, const unsigned* im4) {
        const int v0 = q * 4;
        bool keep[4], any = false;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int v = v0 + cc;
            keep[cc] = v < V && (im4[cc] > T || (im4[cc] == T && v <= last));
            any |= keep[cc];
        }
        if (!any) return;
        u32q b = {{0u, 0u, 0u, 0u}};
        if (noisy) b = philox4x32_10((unsigned)q, (unsigned)r, (unsigned)t, draw, k0, k1);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (keep[cc]) {
                const float y = y_of(im4[cc]);
                const float key = noisy ? y + gumbel(b.w[cc]) : y;
                sk += (double)e_of(y);
                if (key > bk || (key == bk && v0 + cc < bi)) { bk = key; by = y; bi = v0 + cc; }
            }
        }
    };
    if constexpr (NPT4 > 0) {
#pragma unroll
        for (int gq = 0; gq < NPT4; ++gq) group(tid + 256 * gq, ir + 4 * gq);
    } else {
        for (int q = tid; q < groups; q += 256) {
            unsigned im4[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) im4[cc] = 4 * q + cc < V ? img_of(x[4 * q + cc] * inv_temp) : 0u;
            group(q, im4);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float bk2 = __shfl_xor(bk, o, 64), by2 = __shfl_xor(by, o, 64);
        const int bi2 = __shfl_xor(bi, o, 64);
        sk += __shfl_xor(sk, o, 64);
        if (bk2 > bk || (bk2 == bk && bi2 < bi)) { bk = bk2; by = by2; bi = bi2; }
    }
    __syncthreads();                            // the last tally's readers are done with red
    const int w = tid >> 6;
    if ((tid & 63) == 0) {
        red[w] = Tally{bi, __float_as_int(bk), sk};
        sy[w] = by;
    }
    __syncthreads();
    if (tid != 0) return;
    bi = red[0].a; bk = __int_as_float(red[0].b); by = sy[0]; sk = red[0].s;
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
        const float bk2 = __int_as_float(red[ww].b);
        const int bi2 = red[ww].a;
        sk += red[ww].s;
        if (bk2 > bk || (bk2 == bk && bi2 < bi)) { bk = bk2; by = sy[ww]; bi = bi2; }
    }
    const bool found = bi < V;                  // no first element (NaN): <pad>, and its logp is NaN
    const int tok = found ? bi : 0;
    // fp64 from the kept mass to the difference; ONE rounding to fp32
    const float lp = found ? (float)((double)by - ((double)m + log(sk))) : __builtin_nanf("");
    token_t[r] = tok;
    logp_t[r] = lp;
    nkeep_t[r] = nkeep;
    s.sum_logp[r] += lp;
    if (tok == end_tok) {
        s.length[r] = t + 1;
        atomicAdd(s.nopen + n, -1);
        atomicAdd(s.open_rows, -1);
    }
}

// ---- scoring given captions (teacher forcing; the contract: include/scnattn.h) ------------------------------
// The pick with the token told: s.length holds ntok, and a row is open at step t iff t < ntok[r].  Two passes over the row,
// which the fc product has just left in L2, in the ownership of the filtered pick (thread i: the groups of four q = i,
// i + 256, ...):
//   1. the first word of the ORDER as one 64-bit maximum: the image of y above the complemented index, so that among equal
//      images the lower index is the larger number.  Its upper half is the image of m = max y.
//   2. rank (the words strictly before the target in the ORDER, an exact count on images) and S = sum of e_v (fp64), in one
//      tally_all.
// y is taken back from its image in both passes, so -0 counts as +0 everywhere.  There is one form for every V: no row is
// held in registers, hence no second set of bits to keep equal.
template <bool VEC>
__device__ __forceinline__ void load_group(const float* x, int v0, int V, float* e) {
    if (VEC && v0 + 3 < V) {
        const f32x4 l = ld4(x + v0);
        e[0] = l[0]; e[1] = l[1]; e[2] = l[2]; e[3] = l[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = v0 + c < V ? x[v0 + c] : 0.f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void rollout_score_kernel(int K, int V, const float* __restrict__ logits, long ld,
                                                            float inv_temp, int t, const int* __restrict__ target_t,
                                                            int* __restrict__ rank_t, int* __restrict__ best_t,
                                                            RolloutState s) {
    const int r = blockIdx.x, n = r / K;
    if (s.nsrc[n] <= 0) return;                 // a closed image: uniform over the workgroup
    int* token_t = s.token + (long)t * s.R;
    float* logp_t = s.logp + (long)t * s.R;
    const int ntok = s.length[r];
    if (t >= ntok) {                            // a closed row of an open image
        if (threadIdx.x == 0) { token_t[r] = 0; logp_t[r] = 0.f; rank_t[r] = 0; best_t[r] = 0; }
        return;
    }
    __shared__ Tally red[4];
    __shared__ unsigned long long redk[4];
    const float* x = logits + (long)r * ld;
    const int tid = threadIdx.x;
    const int groups = (V + 3) >> 2;
    const int tgt = target_t[r];
    const bool inside = tgt >= 0 && tgt < V;
    const unsigned it = inside ? img_of(x[tgt] * inv_temp) : 0u;

    unsigned long long top = 0ull;              // below every real word: an index is < 2^31, so ~index is not 0
    for (int q = tid; q < groups; q += 256) {
        const int v0 = q * 4;
        float e[4];
        load_group<VEC>(x, v0, V, e);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (v0 + c < V) {
                const unsigned long long k = ((unsigned long long)img_of(e[c] * inv_temp) << 32) | (unsigned)~(v0 + c);
                top = k > top ? k : top;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(top >> 32), o, 64), lo = (unsigned)__shfl_xor((int)top, o, 64);
        const unsigned long long k = ((unsigned long long)hi << 32) | lo;
        top = k > top ? k : top;
    }
    if ((tid & 63) == 0) redk[tid >> 6] = top;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) top = redk[w] > top ? redk[w] : top;
    const unsigned mx = (unsigned)(top >> 32);
    const int best = (int)~(unsigned)top;
    const float m = y_of(mx);

    Tally a = {0, 0, 0.0};
    for (int q = tid; q < groups; q += 256) {
        const int v0 = q * 4;
        float e[4];
        load_group<VEC>(x, v0, V, e);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int v = v0 + c;
            if (v < V) {
                const unsigned im = img_of(e[c] * inv_temp);
                const float y = y_of(im);
                a.a += im > it || (im == it && v < tgt);
                a.s += (double)(y == -INFINITY ? 0.f : expf(y - m));
            }
        }
    }
    a = tally_all(a, red);
    if (tid != 0) return;
    // fp64 from the mass to the difference; ONE rounding to fp32
    const float lp = inside ? (float)((double)y_of(it) - ((double)m + log(a.s))) : __builtin_nanf("");
    token_t[r] = tgt;
    logp_t[r] = lp;
    rank_t[r] = inside ? a.a : V;
    best_t[r] = best;
    s.sum_logp[r] += lp;
    if (t + 1 == ntok) {
        atomicAdd(s.nopen + n, -1);
        atomicAdd(s.open_rows, -1);
    }
}

// target_ws [T][R] from targets [R][ld_tok]; ntok clamped into [0, T]; the counters counted from it (every thread that
// needs a count reads the caller's ntok itself: no workgroup waits for another)
__global__ __launch_bounds__(256) void rollout_score_init_kernel(int N, int K, const int* __restrict__ targets, long ld_tok,
                                                                 const int* __restrict__ ntok, int* __restrict__ target_ws,
                                                                 RolloutState s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int R = s.R, T = s.T;
    auto len = [&](int r) { return min(max(ntok[r], 0), T); };
    if (i < (long)R * T) {
        const int r = (int)(i / T), t = (int)(i - (long)r * T);
        target_ws[(long)t * R + r] = targets[r * ld_tok + t];
    }
    if (i < R) {
        s.length[i] = len((int)i);
        s.sum_logp[i] = 0.f;
    }
    if (i < N) {
        int c = 0;
        for (int j = 0; j < K; ++j) c += len((int)i * K + j) > 0;
        s.nopen[i] = c;
        s.nsrc[i] = c > 0 ? K : 0;
    }
    if (blockIdx.x == 0) {                      // open_rows: an integer count, so any order gives the same number
        __shared__ int cnt[4];
        int c = 0;
        for (int r = threadIdx.x; r < R; r += 256) c += len(r) > 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) s.open_rows[0] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    }
}

// ---- scheduled sampling: the pick told the gold word, behind a coin (the contract: include/scnattn.h) ---------
// s.length holds nmix, and a row is open at step t iff t < nmix[r], as in rollout_score.  The coin is word 0 of the Philox
// call with the counter (0xFFFFFFFF, r, t, draw): a word's noise has v >> 2 < 2^30 there, so the two never meet.  Every
// thread computes the same coin, so the branch is uniform over the workgroup, and a row that keeps its gold word does not
// read its logits at all.  A replaced row is pick_row, the arithmetic and the noise of rollout_pick.
template <bool VEC>
__global__ __launch_bounds__(256) void rollout_pick_mixed_kernel(int K, int V, const float* __restrict__ logits, long ld,
                                                                 float inv_temp, float prob, unsigned k0, unsigned k1,
                                                                 unsigned draw, int t, int greedy,
                                                                 const int* __restrict__ gold_t, int* __restrict__ sample_t,
                                                                 int* __restrict__ replaced_t, RolloutState s) {
    const int r = blockIdx.x, n = r / K;
    if (s.nsrc[n] <= 0) return;                 // a closed image: uniform over the workgroup
    int* token_t = s.token + (long)t * s.R;
    float* logp_t = s.logp + (long)t * s.R;
    const int nmix = s.length[r];
    if (t >= nmix) {                            // a closed row of an open image
        if (threadIdx.x == 0) { token_t[r] = 0; sample_t[r] = -1; logp_t[r] = 0.f; replaced_t[r] = 0; }
        return;
    }
    const unsigned bits = philox4x32_10(0xFFFFFFFFu, (unsigned)r, (unsigned)t, draw, k0, k1).w[0];
    const float u = ((float)(bits >> 9) + 0.5f) * 0x1p-23f;      // 24 significant bits: exact
    int tok = gold_t[r], smp = -1, rep = 0;
    float lp = 0.f;
    if (u < prob) {
        Pick p;
        if (!pick_row<VEC>(logits + (long)r * ld, V, inv_temp, !greedy, r, t, draw, k0, k1, p)) return;
        const bool found = p.bi < V;            // a row of NaN alone has no first element: <pad>, and its logp is NaN
        tok = smp = found ? p.bi : 0;
        lp = found ? p.by - (p.m + logf(p.s)) : __builtin_nanf("");
        rep = 1;
        s.sum_logp[r] += lp;
    } else if (threadIdx.x != 0) {
        return;
    }
    token_t[r] = tok;
    sample_t[r] = smp;
    logp_t[r] = lp;
    replaced_t[r] = rep;
    if (t + 1 == nmix) {
        atomicAdd(s.nopen + n, -1);
        atomicAdd(s.open_rows, -1);
    }
}

bool state_ok(const RolloutState& s, int N, int K) {
    return s.R == N * K && s.T >= 1 && s.open_rows && s.nsrc && s.nopen && s.length && s.sum_logp && s.token && s.logp;
}

}  // namespace

int rollout_pick(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, unsigned long long seed,
                 unsigned draw, int t, int greedy_first, int end_tok, const RolloutState& s) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= 1 && t >= 0, "rollout_pick: bad slot count / vocab_size / step");
    SCN_ARG((long)N * K <= (1L << 20), "rollout_pick: too many rows (images x slots)");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_pick: inv_temp must be positive and finite");
    SCN_ARG(logits && ld >= V && state_ok(s, N, K), "rollout_pick: bad argument");
    SCN_ARG(t < s.T, "rollout_pick: step beyond the records");
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
    const bool vec = aligned16(logits) && ld % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(rollout_pick_kernel<true>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, k0, k1, draw, t,
                           greedy_first, end_tok, s);
    else
        hipLaunchKernelGGL(rollout_pick_kernel<false>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, k0, k1, draw, t,
                           greedy_first, end_tok, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

bool rollout_filter_ok(int top_k, float top_p) { return top_k >= 0 && top_p > 0.f && top_p <= 1.f; }      // NaN: refused

int rollout_pick_filtered(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp,
                          unsigned long long seed, unsigned draw, int t, int greedy_first, int end_tok, int top_k, float top_p,
                          int* nkeep_t, int force_passes, const RolloutState& s) {
    SCN_ARG(rollout_filter_ok(top_k, top_p), "rollout_pick_filtered: need top_k >= 0 and 0 < top_p <= 1");
    const bool k_on = top_k >= 1 && top_k < V, p_on = top_p < 1.f;
    if (!k_on && !p_on)                         // the filter is off: the plain kernel and its bits; nkeep is not written
        return rollout_pick(st, N, K, V, logits, ld, inv_temp, seed, draw, t, greedy_first, end_tok, s);
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= 1 && t >= 0, "rollout_pick_filtered: bad slot count / vocab_size / step");
    SCN_ARG((long)N * K <= (1L << 20), "rollout_pick_filtered: too many rows (images x slots)");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_pick_filtered: inv_temp must be positive and finite");
    SCN_ARG(logits && ld >= V && state_ok(s, N, K), "rollout_pick_filtered: bad argument");
    SCN_ARG(t < s.T, "rollout_pick_filtered: step beyond the records");
    SCN_ARG(nkeep_t, "rollout_pick_filtered: the nkeep record is NULL");
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
    const bool vec = aligned16(logits) && ld % 4 == 0;
    const int Lk = k_on ? top_k : V;
    // a row of up to 10240 words (40 per thread) is held in registers, in the smallest of three sizes that takes it; a
    // longer one (or force_passes) is re-read from global memory in every pass
    const int groups = (V + 3) / 4, npt4 = force_passes || groups > 10 * 256 ? 0 : (groups + 255) / 256;
    dim3 grid(N * K), block(256);
#define L(NPT4)                                                                                                               \
    do {                                                                                                                      \
        if (vec) hipLaunchKernelGGL((rollout_pick_filtered_kernel<NPT4, true>), grid, block, 0, st, K, V, logits, ld, inv_temp, \
                                    k0, k1, draw, t, greedy_first, end_tok, Lk, top_p, nkeep_t, s);                           \
        else hipLaunchKernelGGL((rollout_pick_filtered_kernel<NPT4, false>), grid, block, 0, st, K, V, logits, ld, inv_temp,   \
                                k0, k1, draw, t, greedy_first, end_tok, Lk, top_p, nkeep_t, s);                               \
    } while (0)
    if (npt4 == 0) L(0);
    else if (npt4 <= 1) L(1);
    else if (npt4 <= 3) L(3);
    else L(10);
#undef L
    SCN_LAUNCH_CHECK();
    return 0;
}

int rollout_advance(hipStream_t st, int N, int K, int M, int V, const int* token_t, const float* table, float* emb,
                    const int* nopen, int* nsrc) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && M > 0 && V > 0, "rollout_advance: bad dims");
    SCN_ARG(token_t && table && emb && nopen && nsrc, "rollout_advance: null operand");
    hipLaunchKernelGGL(rollout_advance_kernel, dim3(N * K), dim3(256), 0, st, K, M, V, token_t, table, emb, nopen, nsrc);
    SCN_LAUNCH_CHECK();
    return 0;
}

int rollout_state_init(hipStream_t st, int N, int K, const RolloutState& s) {
    SCN_ARG(N > 0 && K >= 1 && K <= SCN_MAX_BEAM && state_ok(s, N, K), "rollout_state_init: bad argument");
    hipLaunchKernelGGL(rollout_state_init_kernel, dim3(cdiv(s.R, 256)), dim3(256), 0, st, N, K, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

int rollout_score(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, int t,
                  const int* target_t, int* rank_t, int* best_t, const RolloutState& s) {
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= 1 && t >= 0, "rollout_score: bad slot count / vocab_size / step");
    SCN_ARG((long)N * K <= (1L << 20), "rollout_score: too many rows (images x slots)");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_score: inv_temp must be positive and finite");
    SCN_ARG(logits && ld >= V && state_ok(s, N, K), "rollout_score: bad argument");
    SCN_ARG(t < s.T, "rollout_score: step beyond the records");
    SCN_ARG(target_t && rank_t && best_t, "rollout_score: a target / rank / best record is NULL");
    if (aligned16(logits) && ld % 4 == 0)
        hipLaunchKernelGGL(rollout_score_kernel<true>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, t, target_t,
                           rank_t, best_t, s);
    else
        hipLaunchKernelGGL(rollout_score_kernel<false>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, t, target_t,
                           rank_t, best_t, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

bool rollout_prob_ok(float prob) { return prob >= 0.f && prob <= 1.f; }      // NaN: refused

int rollout_pick_mixed(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, float prob,
                       unsigned long long seed, unsigned draw, int t, int greedy, const int* gold_t, int* sample_t,
                       int* replaced_t, const RolloutState& s) {
    SCN_ARG(rollout_prob_ok(prob), "rollout_pick_mixed: prob must be in [0, 1]");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_pick_mixed: inv_temp must be positive and finite");
    if (N <= 0) return 0;
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= 1 && t >= 0, "rollout_pick_mixed: bad slot count / vocab_size / step");
    SCN_ARG((long)N * K <= (1L << 20), "rollout_pick_mixed: too many rows (images x slots)");
    SCN_ARG(logits && ld >= V && state_ok(s, N, K), "rollout_pick_mixed: bad argument");
    SCN_ARG(t < s.T, "rollout_pick_mixed: step beyond the records");
    SCN_ARG(gold_t && sample_t && replaced_t, "rollout_pick_mixed: a gold / sample / replaced record is NULL");
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
    if (aligned16(logits) && ld % 4 == 0)
        hipLaunchKernelGGL(rollout_pick_mixed_kernel<true>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, prob, k0,
                           k1, draw, t, greedy, gold_t, sample_t, replaced_t, s);
    else
        hipLaunchKernelGGL(rollout_pick_mixed_kernel<false>, dim3(N * K), dim3(256), 0, st, K, V, logits, ld, inv_temp, prob, k0,
                           k1, draw, t, greedy, gold_t, sample_t, replaced_t, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

int rollout_score_init(hipStream_t st, int N, int K, const int* targets, long ld_tok, const int* ntok, int* target_ws,
                       const RolloutState& s) {
    SCN_ARG(N > 0 && K >= 1 && K <= SCN_MAX_BEAM && state_ok(s, N, K), "rollout_score_init: bad argument");
    SCN_ARG(targets && ntok && target_ws && ld_tok >= s.T, "rollout_score_init: null captions, or ld_tok below max_steps");
    hipLaunchKernelGGL(rollout_score_init_kernel, dim3(cdiv((long)s.R * s.T, 256)), dim3(256), 0, st, N, K, targets, ld_tok,
                       ntok, target_ws, s);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace scn
