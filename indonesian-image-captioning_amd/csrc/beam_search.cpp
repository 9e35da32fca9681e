// Batched beam search driver: the decode step of sequence.cpp's forward loop over a FIXED N*K rows (K slots per image),
// followed by the selection kernels of beam.hip.  scnattn_beam_init does the teacher-forced driver's set-up (weight
// re-layout, att1 once per IMAGE, qx / qh from the tags, the initial state), scnattn_beam_steps enqueues whole steps; the
// host only reads `open_images` between chunks of steps and the token / parent / alpha records at the end.
// fp32 only: option "decoder_bf16" is not looked at here.
//
// Launches per step (attention decoders): skinny h.[Wd^T|Wbeta^T|Ha], beam_attn_scores, beam_attn_context, skinny z.Wa[M:],
// skinny emb.Wa[:M], scn_mix_fwd, skinny gates, lstm_fwd, fc (sgemm_ws: one or two launches), beam_row_topk, beam_merge,
// beam_advance = 12-13; without attention 9-10.
#include <hip/hip_runtime.h>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"
#include "driver.h"

namespace scn {

namespace {

constexpr long BEAM_GEMM_WS_FLOATS = 8L << 20;     // 32 MiB of split-K partials (fc over N*K rows, the set-up products)

struct BeamWs {
    BeamState s;
    // state: zero-filled by init, so that rows of dead slots that no kernel writes are finite
    float *hA, *cA, *hB, *cB, *emb, *alpha, *z, *e, *candv, *qxr, *qhr, *pa, *phs, *xcat, *gates, *ex, *logits;
    int* candi;
    size_t state_floats;
    // set-up results and scratch
    float *att1, *qx, *qh, *mean_enc, *h0, *c0, *WcatA, *WD, *slabA, *slabC, *slabD, *gws;
};

inline int* ints(float* p) { return reinterpret_cast<int*>(p); }

size_t carve_beam(const scnattn_dims& d, int K, int T, float* base, BeamWs& b) {
    Carver c(base);
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, NA = ncatA(d);
    const long R = (long)N * K;
    b.s.R = (int)R;
    b.s.scores = c.take(R);
    b.s.nsrc = ints(c.take(N));
    b.s.kk = ints(c.take(N));
    b.s.ncomp = ints(c.take(N));
    b.s.best_idx = ints(c.take(N));
    b.s.best_score = c.take(N);
    b.s.open_images = ints(c.take(1));
    b.s.comp_score = c.take(R);
    b.s.comp_step = ints(c.take(R));
    b.s.comp_parent = ints(c.take(R));
    b.s.token = ints(c.take(sz(T, R)));
    b.s.parent = ints(c.take(sz(T, R)));
    b.alpha = d.has_att ? c.take(sz(T, R, P)) : nullptr;
    b.hA = c.take(sz(R, D));
    b.cA = c.take(sz(R, D));
    b.hB = c.take(sz(R, D));
    b.cB = c.take(sz(R, D));
    b.emb = c.take(sz(R, d.M));
    b.z = d.has_att ? c.take(sz(R, E)) : nullptr;
    b.e = d.has_att ? c.take(sz(R, P)) : nullptr;
    b.candv = c.take(sz(R, K));
    b.candi = ints(c.take(sz(R, K)));
    b.qxr = c.take(sz(R, F4));
    b.qhr = c.take(sz(R, F4));
    b.pa = c.take(sz(R, F4));
    b.phs = c.take(sz(R, F4));
    b.xcat = c.take(sz(R, 4, 2 * F));
    b.gates = c.take(sz(R, 4 * D));
    b.ex = c.take(sz(R, F4));
    b.logits = c.take(sz(R, d.V));
    b.state_floats = c.off;
    b.att1 = d.has_att ? c.take(sz(N, P, A)) : nullptr;
    b.qx = c.take(sz(N, F4));
    b.qh = c.take(sz(N, F4));
    b.mean_enc = c.take(sz(N, E));
    b.h0 = c.take(sz(N, D));
    b.c0 = c.take(sz(N, D));
    b.WcatA = c.take(sz(D, NA));
    b.WD = c.take(sz(4, 2 * F, D));
    b.slabA = c.take(sz(SCN_MAX_KSPLIT, R, NA));
    b.slabC = d.has_att ? c.take(sz(SCN_MAX_KSPLIT, R, F4)) : nullptr;
    b.slabD = c.take(sz(SCN_MAX_KSPLIT, 4, R, D));
    b.gws = c.take(BEAM_GEMM_WS_FLOATS);
    return c.off * sizeof(float);
}

int check_beam(const scnattn_dims* d, int K, int T) {
    SCN_ARG(d, "dims is NULL");
    SCN_ARG(d->B > 0 && d->P > 0 && d->E > 0 && d->D > 0 && d->F > 0 && d->M > 0 && d->S > 0 && d->V > 0,
            "dims must be positive");
    SCN_ARG(!d->has_att || d->A > 0, "attention_dim must be positive");
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM, "beam_size must be in [1, 8]");
    SCN_ARG(d->V >= K, "vocab_size must be at least beam_size");
    SCN_ARG(T >= 1 && T <= 4096, "max_steps must be in [1, 4096]");
    SCN_ARG((long)d->B * K <= (1L << 20), "too many rows (images x beam_size)");
    return 0;
}

}  // namespace

int beam_workspace(const scnattn_dims* d, int K, int max_steps, size_t* bytes) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(bytes, "beam_workspace: bytes is NULL");
    BeamWs b;
    *bytes = carve_beam(*d, K, max_steps, nullptr, b);
    return 0;
}

// off[SCNATTN_BEAM_NOFF]: where the results live in the workspace, in 4-byte elements (order: include/scnattn.h)
int beam_layout(const scnattn_dims* d, int K, int max_steps, long* off) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(off, "beam_layout: offsets is NULL");
    BeamWs b;
    float* base = reinterpret_cast<float*>(uintptr_t(1) << 40);     // never dereferenced: only differences are taken
    carve_beam(*d, K, max_steps, base, b);
    const void* p[SCNATTN_BEAM_NOFF] = {b.s.open_images, b.s.nsrc, b.s.kk, b.s.ncomp, b.s.best_idx, b.s.best_score,
                                        b.s.scores, b.s.comp_score, b.s.comp_step, b.s.comp_parent, b.s.token,
                                        b.s.parent, b.alpha};
    for (int i = 0; i < SCNATTN_BEAM_NOFF; ++i)
        off[i] = p[i] ? (long)(reinterpret_cast<const float*>(p[i]) - base) : -1;
    return 0;
}

int beam_init(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, const scnattn_params* w, const float* enc,
              const float* tags, int start_token, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && tags && ws, "beam_init: null argument");
    SCN_ARG(start_token >= 0 && start_token < d.V, "beam_init: start token outside the vocabulary");
    SCN_ARG(aligned16(ws), "beam_init: the workspace must be 16-byte aligned");
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F4 = 4 * d.F, M = d.M;
    BeamWs b;
    carve_beam(d, K, max_steps, ws, b);
    const GemmWs gws{b.gws, BEAM_GEMM_WS_FLOATS};
    SCN_HIP(hipMemsetAsync(ws, 0, b.state_floats * sizeof(float), st));
    SCN_TRY(beam_state_init(st, N, K, b.s));
    SCN_TRY(step_weight_layout(st, d, w, b.WcatA, b.WD));
    if (d.has_att)      // once per image, not per beam
        SCN_TRY(gemm(st, false, true, N * P, A, E, enc, E, w->attention_encoder_att_weight, E, 0.f, b.att1, A, gws,
                     w->attention_encoder_att_bias));
    SCN_TRY(gemm(st, false, false, N, F4, d.S, tags, d.S, w->decode_step_weight_ib, F4, 0.f, b.qx, F4, gws));
    SCN_TRY(gemm(st, false, false, N, F4, d.S, tags, d.S, w->decode_step_weight_hb, F4, 0.f, b.qh, F4, gws));
    SCN_TRY(beam_expand_rows(st, N, K, F4, b.qx, b.qxr));
    SCN_TRY(beam_expand_rows(st, N, K, F4, b.qh, b.qhr));
    SCN_TRY(mean_pixels(st, N, P, E, enc, b.mean_enc));
    SCN_TRY(gemm(st, false, true, N, D, E, b.mean_enc, E, w->init_h_weight, E, 0.f, b.h0, D, gws, w->init_h_bias));
    SCN_TRY(gemm(st, false, true, N, D, E, b.mean_enc, E, w->init_c_weight, E, 0.f, b.c0, D, gws, w->init_c_bias));
    SCN_TRY(beam_expand_rows(st, N, K, D, b.h0, b.hA));     // slot 0 is the live one; the others hold finite copies
    SCN_TRY(beam_expand_rows(st, N, K, D, b.c0, b.cA));
    SCN_TRY(beam_expand_rows(st, 1, N * K, M, w->embedding_weight + (long)start_token * M, b.emb));
    return 0;
}

// Steps t0 .. t0 + n_steps - 1 (0-based; clipped to max_steps).  A finished image's kernels are no-ops.
int beam_steps(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, const scnattn_params* w, const float* enc,
               int end_token, int t0, int n_steps, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && ws, "beam_steps: null argument");
    SCN_ARG(t0 >= 0 && n_steps >= 0, "beam_steps: negative step");
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, M = d.M, V = d.V;
    const int R = N * K, NA = ncatA(d), colph = d.has_att ? A + E : 0;
    const long RD = (long)R * D;
    BeamWs b;
    carve_beam(d, K, max_steps, ws, b);
    const GemmWs gws{b.gws, BEAM_GEMM_WS_FLOATS};
    const float* WaM = d.has_att ? w->decode_step_weight_ia + (long)M * F4 : nullptr;
    const int t1 = t0 + n_steps < max_steps ? t0 + n_steps : max_steps;
    for (int t = t0; t < t1; ++t) {
        int* token_t = b.s.token + (long)t * R;
        int* parent_t = b.s.parent + (long)t * R;
        const int ksA = pick(R, NA, D, 1);
        SCN_TRY(skinny_gemm(st, R, NA, D, 1, b.hA, D, 0, b.WcatA, NA, 0, b.slabA, NA, 0, (long)R * NA, ksA));
        const Slabs ph{b.slabA + colph, ksA, (long)R * NA, NA};
        Slabs pz{nullptr, 0, 0, 0};
        if (d.has_att) {
            const Slabs att2{b.slabA, ksA, (long)R * NA, NA}, gpre{b.slabA + A, ksA, (long)R * NA, NA};
            SCN_TRY(beam_attn_scores(st, N, K, P, A, b.att1, att2, w->attention_decoder_att_bias,
                                     w->attention_full_att_weight, w->attention_full_att_bias, b.s.nsrc, b.e));
            SCN_TRY(beam_attn_context(st, N, K, P, E, enc, b.e, gpre, w->f_beta_bias, b.s.nsrc,
                                      b.alpha + (long)t * R * P, nullptr, b.z));
            const int ksC = pick(R, F4, E, 1);
            SCN_TRY(skinny_gemm(st, R, F4, E, 1, b.z, E, 0, WaM, F4, 0, b.slabC, F4, 0, (long)R * F4, ksC));
            pz = Slabs{b.slabC, ksC, (long)R * F4, F4};
        }
        SCN_TRY(skinny_gemm(st, R, F4, M, 1, b.emb, M, 0, w->decode_step_weight_ia, F4, 0, b.ex, F4, 0, (long)R * F4, 1));
        SCN_TRY(scn_mix_fwd(st, R, F4, pz, b.ex, ph, b.qxr, b.qhr, b.pa, b.phs, b.xcat));
        const int ksD = pick(R, D, 2 * F, 4);
        SCN_TRY(skinny_gemm(st, R, D, 2 * F, 4, b.xcat, 8 * F, 2 * F, b.WD, D, (long)2 * F * D, b.slabD, D, RD, 4 * RD, ksD));
        SCN_TRY(lstm_fwd(st, R, D, Slabs{b.slabD, ksD, 4 * RD, D}, RD, w->decode_step_bias_ih, w->decode_step_bias_hh, b.cA,
                         b.gates, b.cB, b.hB, nullptr));
        SCN_TRY(gemm(st, false, true, R, V, D, b.hB, D, w->fc_weight, D, 0.f, b.logits, V, gws, w->fc_bias));
        SCN_TRY(beam_row_topk(st, N, K, V, b.logits, V, b.s.scores, b.s.nsrc, b.candv, b.candi, 0));
        SCN_TRY(beam_merge(st, N, K, V, end_token, t, b.candv, b.candi, b.s));
        SCN_TRY(beam_advance(st, N, K, D, M, V, b.hB, b.cB, parent_t, token_t, w->embedding_weight, b.hA, b.cA, b.emb));
    }
    return 0;
}

}  // namespace scn
