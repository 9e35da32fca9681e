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
//   rollout_advance  the next input embedding of every row (the token record clamped into the table) and, per image,
//                    nsrc[n] = nopen[n] > 0 ? K : 0 for the attention kernels of the next step.
// The arg-max slot skips the noise: key_v = y_v exactly.  Plain vector loads and stores; no kernel waits for another
// workgroup; no inline assembly.
#include <climits>
#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

struct u32q { unsigned w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ u32q philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32q{{c0, c1, c2, c3}};
}

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
    const bool noisy = !(greedy_first && j == 0);
    const float* x = logits + (long)r * ld;
    Pick p = {-INFINITY, 0.f, -INFINITY, 0.f, INT_MAX};
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
    if (threadIdx.x != 0) return;
    p = Pick{sm[0], ss[0], sk[0], sy[0], si[0]};
    p.merge(sm[1], ss[1], sk[1], sy[1], si[1]);
    p.merge(sm[2], ss[2], sk[2], sy[2], si[2]);
    p.merge(sm[3], ss[3], sk[3], sy[3], si[3]);
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

}  // namespace scn
