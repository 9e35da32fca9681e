// Whole-sequence drivers: one C call enqueues every kernel of the teacher-forced decoder forward
// (models/decoders/attention_scn.py:124-156 / pure_scn.py:114-138) or of its gradient, on the
// caller's stream.  The time loop lives here, not in Python, so the host cost per timestep is a
// handful of hipLaunchKernel calls and nothing else.
//
// Sequence-level restructuring (algebraically identical to the reference):
//   * time-invariant projections are hoisted out of the loop: att1 = encoder_att(enc),
//     qx = s.Wb, qh = s.Hb; the embedding half of u.Wa is batched over all steps (ex), and fc runs
//     once over all (b,t) rows after the loop;
//   * in the backward pass the per-step weight-gradient GEMMs collapse into one GEMM per weight over
//     the stacked (t,b) rows kept in `scratch`, and d att1 / d enc are formed once after the loop.
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"
#include "driver.h"

namespace scn {

int g_ksplit_scale = 0;  // 0 = auto; >0 forces ksplit for every skinny launch (tuning/testing)
int g_profile = 0;       // 1: bracket the recurrence loops with HIP events (scnattn_profile_collect)
int g_dec_bf16 = 0;          // 1 (2: + bf16 matrix instruction in the skinny GEMMs): BASELINE configs[4] flavour -- the operands the recurrence STREAMS every step (recurrent
                             //    weights, att1, the encoder map) are kept as bf16 copies, made once per call; products
                             //    accumulate in fp32, softmax / LSTM state / master weights / every gradient stay fp32

// ---- optional in-stream timing of the recurrence loops (bench.py's roofline figure) ------------------
struct LoopEvent { hipEvent_t a, b; int kind, steps; };
static std::mutex g_prof_mu;
static std::vector<LoopEvent> g_prof;

static hipEvent_t prof_begin(hipStream_t st) {
    if (!g_profile) return nullptr;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    (void)hipEventRecord(e, st);
    return e;
}
static void prof_end(hipStream_t st, hipEvent_t a, int kind, int steps) {
    if (!a) return;
    hipEvent_t b = nullptr;
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return; }
    (void)hipEventRecord(b, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(LoopEvent{a, b, kind, steps});
}

// out[0..5] = {fwd loop ms, fwd steps, bwd loop ms, bwd steps, attn_context ms, attn_context launches}
// summed since the last collect (the last pair only when option "profile" was 2)
int profile_collect(double* out) {
    std::vector<LoopEvent> ev;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        ev.swap(g_prof);
    }
    for (int i = 0; i < 6; ++i) out[i] = 0.0;
    for (auto& e : ev) {
        float ms = 0.f;
        SCN_HIP(hipEventSynchronize(e.b));
        SCN_HIP(hipEventElapsedTime(&ms, e.a, e.b));
        out[e.kind * 2] += ms;
        out[e.kind * 2 + 1] += e.steps;
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    return 0;
}

namespace {

struct Saved {
    float *att1, *qx, *qh, *ex, *emb_tm, *mean_enc, *Hs, *Cs, *att2_all, *alpha_tm, *awe_all, *gate_all, *z_all,
        *pa_all, *ph_all, *gates_all, *tanhc_all, *Hd_bm, *rowmask, *alphaq_tm;
    float *att1h, *ench;      // bf16 copies (raw 16-bit elements) of att1 and of the encoder map, bf16 mode only
};

constexpr long GEMM_WS_FLOATS = 24L << 20;  // 96 MiB of split-K partials for the big GEMMs (d fc.weight: 4 slabs of 10000 x 512)

struct FwdScratch {
    float *WcatA, *WD, *slabA, *e, *slabC, *xcat, *slabD, *gws, *y;
    float *WcatAh, *WDh, *WaMh;      // bf16 copies of the per-step weight operands
};

struct BwdScratch {
    float *WDb, *WaTz, *WcatT, *dHd_bm, *dhfc_tm, *dr_all, *dpx_all, *dcat_all, *dawe_all, *de_all, *dalpha, *dc,
        *dqx_acc, *dqh_acc, *sDb, *sZ, *sH, *datt1, *dwpart, *dwtmp, *demb_tm, *dmean, *dh0, *mx_all, *gws, *present,
        *dalphaq, *dy, *WDbh, *WaTzh, *WcatTh;
};

// Q > 0: pooled path (encoder_out given as its un-pooled source map x [B][Q][E])
size_t carve_saved(const scnattn_dims& d, int Q, float* base, Saved& s) {
    Carver c(base);
    const int B = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F4 = 4 * d.F, T = d.T;
    s.att1 = d.has_att ? c.take(sz(B, P, A)) : nullptr;
    s.qx = c.take(sz(B, F4));
    s.qh = c.take(sz(B, F4));
    s.ex = c.take(sz(T, B, F4));
    s.emb_tm = c.take(sz(T, B, d.M));
    s.mean_enc = c.take(sz(B, E));
    s.Hs = c.take(sz(T + 1, B, D));
    s.Cs = c.take(sz(T + 1, B, D));
    s.att2_all = d.has_att ? c.take(sz(T, B, A)) : nullptr;
    s.alpha_tm = d.has_att ? c.take(sz(T, B, P)) : nullptr;
    s.awe_all = d.has_att ? c.take(sz(T, B, E)) : nullptr;
    s.gate_all = d.has_att ? c.take(sz(T, B, E)) : nullptr;
    s.z_all = d.has_att ? c.take(sz(T, B, E)) : nullptr;
    s.pa_all = c.take(sz(T, B, F4));
    s.ph_all = c.take(sz(T, B, F4));
    s.gates_all = c.take(sz(T, B, 4 * D));
    s.tanhc_all = c.take(sz(T, B, D));
    s.Hd_bm = c.take(sz(B, T, D));
    s.rowmask = c.take(sz(B, T));
    s.alphaq_tm = (d.has_att && Q > 0) ? c.take(sz(T, B, Q)) : nullptr;
    s.att1h = d.has_att ? c.take((sz(B, P, A) + 1) / 2) : nullptr;
    s.ench = d.has_att ? c.take((sz(B, Q > 0 ? Q : P, E) + 1) / 2) : nullptr;
    return c.off * sizeof(float);
}

size_t carve_fwd(const scnattn_dims& d, int Q, float* base, FwdScratch& s) {
    Carver c(base);
    const int B = d.B, D = d.D, F = d.F, NA = ncatA(d);
    s.WcatA = c.take(sz(D, NA));
    s.WD = c.take(sz(4, 2 * F, D));
    s.slabA = c.take(sz(SCN_MAX_KSPLIT, B, NA));
    s.e = d.has_att ? c.take(sz(B, d.P)) : nullptr;
    s.slabC = d.has_att ? c.take(sz(SCN_MAX_KSPLIT, B, 4 * F)) : nullptr;
    s.xcat = c.take(sz(B, 4, 2 * F));
    s.slabD = c.take(sz(SCN_MAX_KSPLIT, 4, B, D));
    s.gws = c.take(GEMM_WS_FLOATS);
    s.y = (d.has_att && Q > 0) ? c.take(sz(B, Q, d.A)) : nullptr;
    s.WcatAh = c.take((sz(D, NA) + 1) / 2);
    s.WDh = c.take((sz(4, 2 * F, D) + 1) / 2);
    s.WaMh = d.has_att ? c.take((sz(d.E, 4 * F) + 1) / 2) : nullptr;
    return c.off * sizeof(float);
}

size_t carve_bwd(const scnattn_dims& d, int Q, float* base, BwdScratch& s) {
    Carver c(base);
    const int B = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * d.F, T = d.T, NC = ncatA(d);
    s.WDb = c.take(sz(4, D, 2 * F));
    s.WaTz = d.has_att ? c.take(sz(F4, E)) : nullptr;
    s.WcatT = c.take(sz(NC, D));
    s.dHd_bm = c.take(sz(B, T, D));
    s.dhfc_tm = c.take(sz(T, B, D));
    s.dr_all = c.take(sz(T, B, 4 * D));
    s.dpx_all = c.take(sz(T, B, F4));
    s.dcat_all = c.take(sz(T, B, NC));
    s.dawe_all = d.has_att ? c.take(sz(T, B, E)) : nullptr;
    s.de_all = d.has_att ? c.take(sz(T, B, P)) : nullptr;
    s.dalpha = d.has_att ? c.take(sz(B, P)) : nullptr;
    s.dc = c.take(sz(B, D));
    s.dqx_acc = c.take(sz(B, F4));
    s.dqh_acc = c.take(sz(B, F4));
    s.sDb = c.take(sz(SCN_MAX_KSPLIT, 4, B, 2 * F));
    s.sZ = d.has_att ? c.take(sz(SCN_MAX_KSPLIT, B, E)) : nullptr;
    s.sH = c.take(sz(SCN_MAX_KSPLIT, B, D));
    s.datt1 = d.has_att ? c.take(sz(B, P, A)) : nullptr;
    s.dwpart = d.has_att ? c.take(sz(attn_datt1_post_blocks(B, P), A + 1)) : nullptr;
    s.dwtmp = d.has_att ? c.take(sz(A + 1)) : nullptr;
    s.demb_tm = c.take(sz(T, B, d.M));
    s.dmean = c.take(sz(B, E));
    s.dh0 = c.take(sz(B, D));
    s.mx_all = c.take(sz(T, B, F4));
    s.present = c.take(sz(d.V));
    s.gws = c.take(GEMM_WS_FLOATS);
    s.dalphaq = (d.has_att && Q > 0) ? c.take(sz(B, Q)) : nullptr;
    s.dy = (d.has_att && Q > 0) ? c.take(sz(B, Q, A)) : nullptr;
    s.WDbh = c.take((sz(4, D, 2 * F) + 1) / 2);
    s.WaTzh = d.has_att ? c.take((sz(F4, E) + 1) / 2) : nullptr;
    s.WcatTh = c.take((sz(NC, D) + 1) / 2);
    return c.off * sizeof(float);
}

int check_dims(const scnattn_dims* d) {
    SCN_ARG(d, "dims is NULL");
    SCN_ARG(d->B > 0 && d->P > 0 && d->E > 0 && d->D > 0 && d->F > 0 && d->M > 0 && d->S > 0 && d->V > 0,
            "dims must be positive");
    SCN_ARG(d->T > 0 && d->L >= d->T, "need 0 < T <= L");
    SCN_ARG(!d->has_att || d->A > 0, "attention_dim must be positive");
    return 0;
}

int check_bt(const scnattn_dims* d, const int32_t* bt) {
    SCN_ARG(bt, "bt_host is NULL");
    for (int t = 0; t < d->T; ++t) {
        SCN_ARG(bt[t] >= 1 && bt[t] <= d->B, "bt_host[t] must be in [1, B]");
        SCN_ARG(t == 0 || bt[t] <= bt[t - 1], "bt_host must be non-increasing (captions sorted by length)");
    }
    SCN_ARG(bt[0] == d->B, "bt_host[0] must equal B (every caption decodes at least one step)");
    return 0;
}

int check_pool(const scnattn_dims* d, const scnattn_pool* p, PoolDesc& out) {
    out = PoolDesc{0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!p) return 0;
    // (without attention only the initial state reads encoder_out: its pixel mean becomes a weighted mean of x)
    PoolDesc pd;
    SCN_TRY(pool_desc(p, pd));
    SCN_ARG(p->Q <= d->P, "scnattn_pool: bad Q / qtap_max");
    SCN_ARG((!d->has_att || d->A % 4 == 0) && d->E % 4 == 0,
            "scnattn_pool: attention_dim and encoder_dim must be multiples of 4");
    out = pd;
    return 0;
}

// bf16 storage mode: every converted buffer must be a whole number of 4-element groups
inline bool bf16_mode(const scnattn_dims& d) {
    return g_dec_bf16 && d.D % 4 == 0 && d.F % 4 == 0 && d.E % 4 == 0 && (!d.has_att || d.A % 4 == 0);
}

// What the step kernels stream, the same selection in both drivers: the fp32 originals, or in bf16 mode the copies of
// att1 and of the map the context is summed over that the forward pass makes once per call.
struct Streamed {
    bool bf;                    // bf16 storage mode
    int bfm;                    // skinny_gemm's wbf: 0 fp32 weights, 1 bf16 weights, 2 + the bf16 matrix instruction
    const void *att1, *enc;
};
Streamed streamed(const scnattn_dims& d, const Saved& s, const float* enc) {
    const bool bf = bf16_mode(d), copies = bf && d.has_att;
    return Streamed{bf, bf ? (g_dec_bf16 >= 2 ? 2 : 1) : 0, copies ? (const void*)s.att1h : s.att1,
                    copies ? (const void*)s.ench : enc};
}

}  // namespace

int seq_workspace(const scnattn_dims* d, const scnattn_pool* pool, size_t* saved_bytes, size_t* scratch_bytes) {
    SCN_TRY(check_dims(d));
    PoolDesc pd;
    SCN_TRY(check_pool(d, pool, pd));
    Saved s;
    FwdScratch f;
    BwdScratch b;
    const size_t sv = carve_saved(*d, pd.Q, nullptr, s);
    const size_t fw = carve_fwd(*d, pd.Q, nullptr, f);
    const size_t bw = carve_bwd(*d, pd.Q, nullptr, b);
    if (saved_bytes) *saved_bytes = sv;
    if (scratch_bytes) *scratch_bytes = fw > bw ? fw : bw;
    return 0;
}

int seq_fwd(hipStream_t st, const scnattn_dims* dp, const scnattn_params* w, const float* enc, const float* tags,
            const int64_t* caps, const int32_t* dl_dev, const int32_t* bt, const float* drop_mask, float* saved,
            float* scratch, float* preds, float* alphas, const scnattn_pool* pool) {
    SCN_TRY(check_dims(dp));
    SCN_TRY(check_bt(dp, bt));
    const scnattn_dims& d = *dp;
    PoolDesc pd;
    SCN_TRY(check_pool(dp, pool, pd));
    const int Q = pd.Q;             // > 0: `enc` is the un-pooled map x [B][Q][E]
    SCN_ARG(w && enc && tags && caps && dl_dev && saved && scratch && preds, "seq_fwd: null argument");
    SCN_ARG(!d.has_att || alphas, "seq_fwd: alphas is NULL");
    const int B = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, M = d.M, T = d.T;
    const int NA = ncatA(d), colph = d.has_att ? A + E : 0;
    Saved s;
    FwdScratch f;
    carve_saved(d, Q, saved, s);
    carve_fwd(d, Q, scratch, f);
    const GemmWs gws{f.gws, GEMM_WS_FLOATS};
    const Streamed sm = streamed(d, s, enc);
    const bool bf = sm.bf;
    const int bfm = sm.bfm;

    // ---- weight re-layout (driver.h) -------------------------------------------------------------
    SCN_TRY(step_weight_layout(st, d, w, f.WcatA, f.WD));

    if (bf) {
        SCN_TRY(f32_to_bf16(st, sz(D, NA), f.WcatA, f.WcatAh));
        SCN_TRY(f32_to_bf16(st, sz(4, 2 * F, D), f.WD, f.WDh));
        if (d.has_att) SCN_TRY(f32_to_bf16(st, sz(E, F4), w->decode_step_weight_ia + (long)M * F4, f.WaMh));
    }
    const void* WcatA = bf ? (const void*)f.WcatAh : f.WcatA;
    const void* WD = bf ? (const void*)f.WDh : f.WD;
    const void* WaM = bf ? (const void*)f.WaMh : (d.has_att ? w->decode_step_weight_ia + (long)M * F4 : nullptr);

    // ---- time-invariant pieces -----------------------------------------------------------------
    if (d.has_att && Q > 0) {
        // att1 = pool(x) . We^T + be = pool(x . We^T) + be: the projection runs on Q rows per image, not P
        SCN_TRY(gemm(st, false, true, B * Q, A, E, enc, E, w->attention_encoder_att_weight, E, 0.f, f.y, A, gws));
        SCN_TRY(pool_expand(st, B, P, A, pd, f.y, w->attention_encoder_att_bias, s.att1));
    } else if (d.has_att) {
        SCN_TRY(gemm(st, false, true, B * P, A, E, enc, E, w->attention_encoder_att_weight, E, 0.f, s.att1, A, gws,
                     w->attention_encoder_att_bias));
    }
    if (bf && d.has_att) {     // what the step kernels stream: bf16 copies of att1 and of the map the context is summed over
        SCN_TRY(f32_to_bf16(st, sz(B, P, A), s.att1, s.att1h));
        SCN_TRY(f32_to_bf16(st, sz(B, Q > 0 ? Q : P, E), enc, s.ench));
    }
    SCN_TRY(gemm(st, false, false, B, F4, d.S, tags, d.S, w->decode_step_weight_ib, F4, 0.f, s.qx, F4, gws));
    SCN_TRY(gemm(st, false, false, B, F4, d.S, tags, d.S, w->decode_step_weight_hb, F4, 0.f, s.qh, F4, gws));
    SCN_TRY(gather_rows_tm(st, B, T, d.L, M, (const long long*)caps, w->embedding_weight, d.V, s.emb_tm));
    SCN_TRY(gemm(st, false, false, T * B, F4, M, s.emb_tm, M, w->decode_step_weight_ia, F4, 0.f, s.ex, F4, gws));
    if (Q > 0) SCN_TRY(weighted_rows(st, B, Q, E, enc, pd.col_w, s.mean_enc));
    else SCN_TRY(mean_pixels(st, B, P, E, enc, s.mean_enc));
    SCN_TRY(gemm(st, false, true, B, D, E, s.mean_enc, E, w->init_h_weight, E, 0.f, s.Hs, D, gws, w->init_h_bias));
    SCN_TRY(gemm(st, false, true, B, D, E, s.mean_enc, E, w->init_c_weight, E, 0.f, s.Cs, D, gws, w->init_c_bias));

    // ---- the recurrence --------------------------------------------------------------------------
    const long BD = (long)B * D;
    hipEvent_t ev0 = prof_begin(st);
    for (int t = 0; t < T; ++t) {
        const int rows = bt[t];                                    // captions still decoding (check_bt: 1 <= rows <= B)
        const long rowT = (long)t * B;                             // first row of this step in [T][B][.] buffers
        const float *h = s.Hs + rowT * D, *c = s.Cs + rowT * D, *ex = s.ex + rowT * F4;
        float *h_new = s.Hs + (rowT + B) * D, *c_new = s.Cs + (rowT + B) * D;
        float *pa = s.pa_all + rowT * F4, *phs = s.ph_all + rowT * F4;
        float *gates = s.gates_all + rowT * 4 * D, *tanhc = s.tanhc_all + rowT * D;
        // h . [Wd^T | Wbeta^T | Ha]: att2, the gate's pre-activation and ph, as column ranges of one split-K result
        const int ksA = pick(rows, NA, D, 1);
        SCN_TRY(skinny_gemm(st, rows, NA, D, 1, h, D, 0, WcatA, NA, 0, f.slabA, NA, 0, (long)B * NA, ksA, bfm));
        const Slabs ph{f.slabA + colph, ksA, (long)B * NA, NA};
        Slabs pz{nullptr, 0, 0, 0};
        if (d.has_att) {
            const Slabs att2{f.slabA, ksA, (long)B * NA, NA}, gpre{f.slabA + A, ksA, (long)B * NA, NA};
            float* alpha_out = alphas + (long)t * P;
            SCN_TRY(attn_scores(st, rows, P, A, sm.att1, att2, w->attention_decoder_att_bias, w->attention_full_att_weight,
                                w->attention_full_att_bias, f.e, s.att2_all + rowT * A, bf));
            hipEvent_t evc = g_profile >= 2 ? prof_begin(st) : nullptr;   // per-launch timing of the dominant kernel
            if (Q > 0)
                SCN_TRY(attn_context_pooled(st, rows, P, E, sm.enc, pd, f.e, gpre, w->f_beta_bias, alpha_out, (long)T * P,
                                            s.alpha_tm + rowT * P, s.alphaq_tm + rowT * Q, s.awe_all + rowT * E,
                                            s.gate_all + rowT * E, s.z_all + rowT * E, bf));
            else
                SCN_TRY(attn_context(st, rows, P, E, sm.enc, f.e, gpre, w->f_beta_bias, alpha_out, (long)T * P,
                                     s.alpha_tm + rowT * P, s.awe_all + rowT * E, s.gate_all + rowT * E, s.z_all + rowT * E,
                                     bf));
            prof_end(st, evc, 2, 1);
            // z . Wa[M:], consumed by the SCN mix (scn_cell.py:73-86)
            const int ksC = pick(rows, F4, E, 1);
            SCN_TRY(skinny_gemm(st, rows, F4, E, 1, s.z_all + rowT * E, E, 0, WaM, F4, 0, f.slabC, F4, 0, (long)B * F4, ksC,
                                bfm));
            pz = Slabs{f.slabC, ksC, (long)B * F4, F4};
        }
        SCN_TRY(scn_mix_fwd(st, rows, F4, pz, ex, ph, s.qx, s.qh, pa, phs, f.xcat));
        // [mx | mh] . [Wc; Hc] for the four gates, then the LSTM update
        const int ksD = pick(rows, D, 2 * F, 4);
        SCN_TRY(skinny_gemm(st, rows, D, 2 * F, 4, f.xcat, 8 * F, 2 * F, WD, D, (long)2 * F * D, f.slabD, D, BD, 4 * BD, ksD,
                            bfm));
        SCN_TRY(lstm_fwd(st, rows, D, Slabs{f.slabD, ksD, 4 * BD, D}, BD, w->decode_step_bias_ih, w->decode_step_bias_hh, c,
                         gates, c_new, h_new, tanhc));
    }
    prof_end(st, ev0, 0, T);

    // ---- dropout + fc over all (b,t) rows at once ------------------------------------------------
    SCN_TRY(hidden_to_bm(st, B, T, D, dl_dev, s.Hs + BD, drop_mask, s.Hd_bm, s.rowmask));
    SCN_TRY(gemm(st, false, true, B * T, d.V, D, s.Hd_bm, D, w->fc_weight, D, 0.f, preds, d.V, gws, w->fc_bias,
                 s.rowmask));
    return 0;
}

int seq_bwd(hipStream_t st, const scnattn_dims* dp, const scnattn_params* w, const float* enc, const float* tags,
            const int64_t* caps, const int32_t* dl_dev, const int32_t* bt, const float* drop_mask,
            const float* saved, float* scratch, const float* dpreds, const float* dalphas, const scnattn_params* g,
            float* denc, float* dtags, const scnattn_pool* pool) {
    SCN_TRY(check_dims(dp));
    SCN_TRY(check_bt(dp, bt));
    const scnattn_dims& d = *dp;
    PoolDesc pd;
    SCN_TRY(check_pool(dp, pool, pd));
    const int Q = pd.Q;             // > 0: `enc` is x [B][Q][E] and `denc` receives d x [B][Q][E]
    SCN_ARG(w && g && enc && tags && caps && dl_dev && saved && scratch && dpreds, "seq_bwd: null argument");
    const int B = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, M = d.M, T = d.T, V = d.V;
    const int NC = ncatA(d);  // columns of the concatenated [dph | dgpre | datt2] operand
    const int TB = T * B;
    const long BD = (long)B * D;
    Saved s;
    BwdScratch k;
    carve_saved(d, Q, const_cast<float*>(saved), s);
    carve_bwd(d, Q, scratch, k);
    const GemmWs gws{k.gws, GEMM_WS_FLOATS};
    const Streamed sm = streamed(d, s, enc);    // the copies the forward pass streamed
    const bool bf = sm.bf;
    const int bfm = sm.bfm;
    const int R = Q > 0 ? Q : P;                // pixels per image of the map `enc` holds
    const float* dproj = Q > 0 ? k.dy : k.datt1;    // d (enc . We^T) on those pixels: d y (pooled) or d att1

    // ---- fc / dropout ----------------------------------------------------------------------------
    if (g->fc_weight)
        SCN_TRY(gemm(st, true, false, V, D, B * T, dpreds, V, s.Hd_bm, D, 0.f, g->fc_weight, D, gws));
    if (g->fc_bias)  // only rows that were decoded carry the bias
        SCN_TRY(colsum_masked(st, B * T, V, dpreds, V, s.rowmask, g->fc_bias, 0.f));
    SCN_TRY(gemm(st, false, false, B * T, D, V, dpreds, V, w->fc_weight, D, 0.f, k.dHd_bm, D, gws));
    SCN_TRY(hidden_from_bm(st, B, T, D, dl_dev, k.dHd_bm, drop_mask, k.dhfc_tm));

    // ---- transposed weight layouts for the backward contractions ------------------------------------
    for (int gi = 0; gi < 4; ++gi) {
        float* wd = k.WDb + (long)gi * D * 2 * F;
        SCN_TRY(copy2d(st, D, F, w->decode_step_weight_ic + gi * F, F4, wd, 2 * F));
        SCN_TRY(copy2d(st, D, F, w->decode_step_weight_hc + gi * F, F4, wd + F, 2 * F));
    }
    SCN_TRY(transpose2d(st, D, F4, w->decode_step_weight_ha, F4, k.WcatT, D));  // Ha^T : [4F][D]
    if (d.has_att) {
        SCN_TRY(transpose2d(st, E, F4, w->decode_step_weight_ia + (long)M * F4, F4, k.WaTz, E));  // Wa[M:]^T
        SCN_TRY(copy2d(st, E, D, w->f_beta_weight, D, k.WcatT + (long)F4 * D, D));
        SCN_TRY(copy2d(st, A, D, w->attention_decoder_att_weight, D, k.WcatT + (long)(F4 + E) * D, D));
    }
    if (bf) {
        SCN_TRY(f32_to_bf16(st, sz(4, D, 2 * F), k.WDb, k.WDbh));
        SCN_TRY(f32_to_bf16(st, sz(NC, D), k.WcatT, k.WcatTh));
        if (d.has_att) SCN_TRY(f32_to_bf16(st, sz(F4, E), k.WaTz, k.WaTzh));
    }
    const void* WDb = bf ? (const void*)k.WDbh : k.WDb;
    const void* WcatT = bf ? (const void*)k.WcatTh : k.WcatT;
    const void* WaTz = bf ? (const void*)k.WaTzh : k.WaTz;
    SCN_HIP(hipMemsetAsync(k.dc, 0, sizeof(float) * BD, st));
    SCN_HIP(hipMemsetAsync(k.dqx_acc, 0, sizeof(float) * B * F4, st));
    SCN_HIP(hipMemsetAsync(k.dqh_acc, 0, sizeof(float) * B * F4, st));

    // ---- reverse recurrence ----------------------------------------------------------------------
    hipEvent_t ev0 = prof_begin(st);
    int ksH = 0;
    for (int t = T - 1; t >= 0; --t) {
        const int rows = bt[t];                                    // check_bt: 1 <= rows <= B, non-increasing in t
        const int rows_next = (t + 1 < T) ? bt[t + 1] : 0;
        const long rowT = (long)t * B;
        float* dr = k.dr_all + rowT * 4 * D;
        float* dcat = k.dcat_all + rowT * NC;
        float* dpx = k.dpx_all + rowT * F4;
        const float *pa = s.pa_all + rowT * F4, *phs = s.ph_all + rowT * F4;
        // d h of step t+1 (the previous iteration's last product) is this step's dh_next
        SCN_TRY(lstm_bwd(st, rows, rows_next, D, k.dhfc_tm + rowT * D,
                         rows_next > 0 ? Slabs{k.sH, ksH, BD, D} : Slabs{nullptr, 0, 0, 0}, k.dc,
                         s.gates_all + rowT * 4 * D, s.Cs + rowT * D, s.tanhc_all + rowT * D, dr));
        const int ksDb = pick(rows, 2 * F, D, 4);
        SCN_TRY(skinny_gemm(st, rows, 2 * F, D, 4, dr, 4 * D, D, WDb, 2 * F, (long)D * 2 * F, k.sDb, 2 * F, (long)B * 2 * F,
                            (long)4 * B * 2 * F, ksDb, bfm));
        SCN_TRY(scn_mix_bwd(st, rows, F4, Slabs{k.sDb, ksDb, (long)4 * B * 2 * F, 2 * F}, (long)B * 2 * F, s.qx, s.qh, pa,
                            phs, dpx, dcat, NC, k.dqx_acc, k.dqh_acc));
        if (d.has_att) {
            const int ksZ = pick(rows, E, F4, 1);
            float* dawe = k.dawe_all + rowT * E;
            const float *awe = s.awe_all + rowT * E, *gate = s.gate_all + rowT * E;
            SCN_TRY(skinny_gemm(st, rows, E, F4, 1, dpx, F4, 0, WaTz, E, 0, k.sZ, E, 0, (long)B * E, ksZ, bfm));
            SCN_TRY(gate_bwd(st, rows, E, Slabs{k.sZ, ksZ, (long)B * E, E}, awe, gate, dawe, dcat + F4, NC));
            const float* din = dalphas ? dalphas + (long)t * P : nullptr;
            if (Q > 0) {
                // Q dot products per image against x, folded onto the P pooled pixels inside softmax_bwd
                SCN_TRY(attn_dalpha(st, rows, Q, E, sm.enc, dawe, nullptr, 0, k.dalphaq, bf));
                SCN_TRY(attn_softmax_bwd_pooled(st, rows, P, A, sm.att1, s.att2_all + rowT * A, w->attention_full_att_weight,
                                                s.alpha_tm + rowT * P, pd, k.dalphaq, din, (long)T * P, k.de_all + rowT * P,
                                                dcat + F4 + E, NC, bf));
            } else {
                SCN_TRY(attn_dalpha(st, rows, P, E, sm.enc, dawe, din, (long)T * P, k.dalpha, bf));
                SCN_TRY(attn_softmax_bwd(st, rows, P, A, sm.att1, s.att2_all + rowT * A, w->attention_full_att_weight,
                                         s.alpha_tm + rowT * P, k.dalpha, k.de_all + rowT * P, dcat + F4 + E, NC, bf));
            }
        }
        ksH = pick(rows, D, NC, 1);
        // d cat . Wcat^T = this step's d h, the missing input of the LSTM backward of step t-1 (scn_cell.py:134-152
        // transposed)
        SCN_TRY(skinny_gemm(st, rows, D, NC, 1, dcat, NC, 0, WcatT, D, 0, k.sH, D, 0, BD, ksH, bfm));
    }
    // d loss / d h0 (d/d c0 is k.dc): the last product ran at t = 0, where every row decodes
    SCN_TRY(reduce_slabs(st, B, D, Slabs{k.sH, ksH, BD, D}, k.dh0));
    prof_end(st, ev0, 1, T);

    // ---- after the loop: weight gradients, one GEMM per weight over the stacked (t,b) rows ----------------
    if (g->decode_step_weight_ia) {
        SCN_TRY(gemm(st, true, false, M, F4, TB, s.emb_tm, M, k.dpx_all, F4, 0.f, g->decode_step_weight_ia, F4, gws));
        if (d.has_att)
            SCN_TRY(gemm(st, true, false, E, F4, TB, s.z_all, E, k.dpx_all, F4, 0.f,
                         g->decode_step_weight_ia + (long)M * F4, F4, gws));
    }
    if (g->embedding_weight) {
        SCN_TRY(gemm(st, false, true, TB, M, F4, k.dpx_all, F4, w->decode_step_weight_ia, F4, 0.f, k.demb_tm, M, gws));
        SCN_TRY(scatter_add_rows_tm(st, B, T, d.L, M, (const long long*)caps, dl_dev, k.demb_tm, V,
                                    g->embedding_weight, reinterpret_cast<int*>(k.present)));
    }
    if (g->decode_step_weight_ic) {
        SCN_TRY(mul_bcast(st, T, B, F4, s.pa_all, s.qx, k.mx_all));
        SCN_TRY(sgemm_ws(st, true, false, D, F, TB, 1.f, k.dr_all, 4 * D, k.mx_all, F4, 0.f, g->decode_step_weight_ic, F4,
                         nullptr, nullptr, 4, D, F, F, gws.p, gws.floats));
    }
    if (g->decode_step_weight_hc) {
        SCN_TRY(mul_bcast(st, T, B, F4, s.ph_all, s.qh, k.mx_all));
        SCN_TRY(sgemm_ws(st, true, false, D, F, TB, 1.f, k.dr_all, 4 * D, k.mx_all, F4, 0.f, g->decode_step_weight_hc, F4,
                         nullptr, nullptr, 4, D, F, F, gws.p, gws.floats));
    }
    if (g->decode_step_weight_ha)
        SCN_TRY(gemm(st, true, false, D, F4, TB, s.Hs, D, k.dcat_all, NC, 0.f, g->decode_step_weight_ha, F4, gws));
    if (g->decode_step_weight_ib)
        SCN_TRY(gemm(st, true, false, d.S, F4, B, tags, d.S, k.dqx_acc, F4, 0.f, g->decode_step_weight_ib, F4, gws));
    if (g->decode_step_weight_hb)
        SCN_TRY(gemm(st, true, false, d.S, F4, B, tags, d.S, k.dqh_acc, F4, 0.f, g->decode_step_weight_hb, F4, gws));
    if (g->decode_step_bias_ih) SCN_TRY(colsum(st, TB, 4 * D, k.dr_all, 4 * D, g->decode_step_bias_ih, 0.f));
    if (g->decode_step_bias_hh) SCN_TRY(colsum(st, TB, 4 * D, k.dr_all, 4 * D, g->decode_step_bias_hh, 0.f));
    if (d.has_att) {
        if (g->f_beta_weight)
            SCN_TRY(gemm(st, true, false, E, D, TB, k.dcat_all + F4, NC, s.Hs, D, 0.f, g->f_beta_weight, D, gws));
        if (g->f_beta_bias) SCN_TRY(colsum(st, TB, E, k.dcat_all + F4, NC, g->f_beta_bias, 0.f));
        if (g->attention_decoder_att_weight)
            SCN_TRY(gemm(st, true, false, A, D, TB, k.dcat_all + F4 + E, NC, s.Hs, D, 0.f,
                         g->attention_decoder_att_weight, D, gws));
        if (g->attention_decoder_att_bias)
            SCN_TRY(colsum(st, TB, A, k.dcat_all + F4 + E, NC, g->attention_decoder_att_bias, 0.f));
    }
    if (g->init_h_weight)
        SCN_TRY(gemm(st, true, false, D, E, B, k.dh0, D, s.mean_enc, E, 0.f, g->init_h_weight, E, gws));
    if (g->init_h_bias) SCN_TRY(colsum(st, B, D, k.dh0, D, g->init_h_bias, 0.f));
    if (g->init_c_weight)
        SCN_TRY(gemm(st, true, false, D, E, B, k.dc, D, s.mean_enc, E, 0.f, g->init_c_weight, E, gws));
    if (g->init_c_bias) SCN_TRY(colsum(st, B, D, k.dc, D, g->init_c_bias, 0.f));
    if (dtags) {
        SCN_TRY(gemm(st, false, true, B, d.S, F4, k.dqx_acc, F4, w->decode_step_weight_ib, F4, 0.f, dtags, d.S, gws));
        SCN_TRY(gemm(st, false, true, B, d.S, F4, k.dqh_acc, F4, w->decode_step_weight_hb, F4, 1.f, dtags, d.S, gws));
    }
    if (d.has_att) {
        int nblk = 0;
        SCN_TRY(attn_datt1_post(st, B, P, A, T, dl_dev, sm.att1, s.att2_all, k.de_all, w->attention_full_att_weight,
                                k.datt1, k.dwpart, &nblk, bf));
        SCN_TRY(colsum(st, nblk, A + 1, k.dwpart, A + 1, k.dwtmp, 0.f));
        if (g->attention_full_att_weight)
            SCN_TRY(copy2d(st, 1, A, k.dwtmp, A + 1, g->attention_full_att_weight, A));
        if (g->attention_full_att_bias) SCN_TRY(copy2d(st, 1, 1, k.dwtmp + A, 1, g->attention_full_att_bias, 1));
        if (Q > 0 && (g->attention_encoder_att_weight || denc))
            SCN_TRY(pool_transpose(st, B, P, A, pd, k.datt1, k.dy));      // d y = pool^T (d att1): [B*Q][A]
        // d encoder_att: needs d att1 (/ d y)
        if (g->attention_encoder_att_weight)
            SCN_TRY(gemm(st, true, false, A, E, B * R, dproj, A, enc, E, 0.f, g->attention_encoder_att_weight, E, gws));
        if (g->attention_encoder_att_bias)
            SCN_TRY(colsum(st, B * P, A, k.datt1, A, g->attention_encoder_att_bias, 0.f));
    }

    // ---- d loss / d encoder_out (only when the encoder is fine-tuned) -------------------------------
    if (denc) {
        // pooled: d x = d y . We  +  sum_t alphaq_t (x) dawe_t  +  col_w (x) d mean      (all on the Q source pixels)
        // dense:  d enc = d att1 . We  +  sum_t alpha_t (x) dawe_t  +  d mean / P           (on the P pixels)
        if (d.has_att) {
            SCN_TRY(gemm(st, false, false, B * R, E, A, dproj, A, w->attention_encoder_att_weight, E, 0.f, denc, E, gws));
            // denc[b] += alpha_b^T (R x T) . dawe_b (T x E), batched over b
            SCN_TRY(sgemm_ws(st, true, false, R, E, T, 1.f, Q > 0 ? s.alphaq_tm : s.alpha_tm, (long)B * R, k.dawe_all,
                             (long)B * E, 1.f, denc, E, nullptr, nullptr, B, R, E, (long)R * E, gws.p, gws.floats));
        } else {
            SCN_HIP(hipMemsetAsync(denc, 0, sizeof(float) * B * R * E, st));
        }
        SCN_TRY(gemm(st, false, false, B, E, D, k.dh0, D, w->init_h_weight, E, 0.f, k.dmean, E, gws));
        SCN_TRY(gemm(st, false, false, B, E, D, k.dc, D, w->init_c_weight, E, 1.f, k.dmean, E, gws));
        if (Q > 0) SCN_TRY(add_bcast_rows_w(st, B, Q, E, pd.col_w, k.dmean, denc));
        else SCN_TRY(add_bcast_rows(st, B, P, E, k.dmean, 1.f / (float)P, denc));
    }
    return 0;
}

}  // namespace scn
