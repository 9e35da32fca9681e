// What the decoder drivers share (sequence.cpp: the teacher-forced sequence; beam_search.cpp: the batched beam search):
// workspace carving, the split-K policy of the skinny products, the dense product with its workspace, and the weight
// re-layout of the decode step.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {

extern int g_ksplit_scale;  // 0 = auto; >0 forces ksplit for every skinny launch (tuning/testing)

namespace {

struct Carver {
    float* base;
    size_t off = 0;  // in floats
    explicit Carver(float* b) : base(b) {}
    float* take(size_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 63) & ~size_t(63);  // 256-byte granules keep every buffer 16-byte aligned
        return p;
    }
};

inline size_t sz(long a, long b = 1, long c = 1, long d = 1) { return (size_t)a * b * c * d; }

inline int ncatA(const scnattn_dims& d) { return d.has_att ? d.A + d.E + 4 * d.F : 4 * d.F; }

inline int pick(int rows, int N, int K, int groups) {
    if (g_ksplit_scale > 0) {
        int ks = g_ksplit_scale;
        const int kmax = K / 8 > 0 ? K / 8 : 1;
        if (ks > kmax) ks = kmax;
        if (ks > SCN_MAX_KSPLIT) ks = SCN_MAX_KSPLIT;
        return ks;
    }
    return skinny_pick_ksplit(rows, N, K, groups);
}

// Split-K workspace of the big GEMMs: pointer and size travel together.
struct GemmWs { float* p; long floats; };

// C = op(A) . op(B) + beta * C (+ bias; rows with rowmask == 0 written as zeros): the un-batched sgemm_ws with alpha = 1
int gemm(hipStream_t st, bool tA, bool tB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
         float beta, float* C, long ldc, GemmWs ws, const float* bias = nullptr, const float* rowmask = nullptr) {
    return sgemm_ws(st, tA, tB, M, N, K, 1.f, A, lda, B, ldb, beta, C, ldc, bias, rowmask, 1, 0, 0, 0, ws.p, ws.floats);
}

// Weight re-layout of the decode step: every per-step contraction streams a row-major [K][N] matrix.
//   WcatA [D][ncatA] = [Wd^T | Wbeta^T | Ha] (Ha alone without attention);  WD [4][2F][D] = per gate [Wc_g^T ; Hc_g^T]
inline int step_weight_layout(hipStream_t st, const scnattn_dims& d, const scnattn_params* w, float* WcatA, float* WD) {
    const int E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, NA = ncatA(d), colph = d.has_att ? A + E : 0;
    if (d.has_att) {
        SCN_TRY(transpose2d(st, A, D, w->attention_decoder_att_weight, D, WcatA, NA));       // Wd^T
        SCN_TRY(transpose2d(st, E, D, w->f_beta_weight, D, WcatA + A, NA));                  // Wbeta^T
    }
    SCN_TRY(copy2d(st, D, F4, w->decode_step_weight_ha, F4, WcatA + colph, NA));             // Ha
    for (int g = 0; g < 4; ++g) {
        float* wd = WD + (long)g * 2 * F * D;
        SCN_TRY(transpose2d(st, D, F, w->decode_step_weight_ic + g * F, F4, wd, D));           // Wc_g^T
        SCN_TRY(transpose2d(st, D, F, w->decode_step_weight_hc + g * F, F4, wd + (long)F * D, D));  // Hc_g^T
    }
    return 0;
}

}  // namespace

}  // namespace scn
