// extern "C" surface of libscnattn (declared in include/scnattn.h).
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

thread_local LaunchPlan* t_plan_out = nullptr;

extern int g_ksplit_scale;
extern int g_profile;
extern int g_attn_depth;
extern int g_dec_bf16;
extern int g_gemm_target, g_gemm_kmin, g_gemm_kmin_small, g_gemm_gate, g_use_cgemm, g_cgemm_target, g_cgemm_kmin, g_cgemm_mi, g_cgemm_combine, g_cgemm_combine_max;
int profile_collect(double* out);
int seq_workspace(const scnattn_dims* d, const scnattn_pool* pool, size_t* saved_bytes, size_t* scratch_bytes);
int seq_fwd(hipStream_t st, const scnattn_dims* d, const scnattn_params* w, const float* enc, const float* tags,
            const int64_t* caps, const int32_t* dl_dev, const int32_t* bt, const float* drop_mask, float* saved,
            float* scratch, float* preds, float* alphas, const scnattn_pool* pool);
int seq_bwd(hipStream_t st, const scnattn_dims* d, const scnattn_params* w, const float* enc, const float* tags,
            const int64_t* caps, const int32_t* dl_dev, const int32_t* bt, const float* drop_mask,
            const float* saved, float* scratch, const float* dpreds, const float* dalphas, const scnattn_params* g,
            float* denc, float* dtags, const scnattn_pool* pool);
// the one search driver (beam_search.cpp); o: the search options, null for a search without
// v: the diversity of a search in groups, null for a search without; cn: the constraints of a constrained search, likewise
int search_workspace(int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                     const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, size_t* bytes);
int search_layout(int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                  const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, long* off);
int search_init(hipStream_t st, int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, const scnattn_params* w,
                const float* enc, const float* const* tags, int start_token, float* ws);
int search_steps(hipStream_t st, int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                 const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, const scnattn_params* w,
                 const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps, float* ws);
// filtered: the _f form (f is then checked and the workspace holds the nkeep records); else f is ignored
int rollout_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                      bool filtered, size_t* bytes);
int rollout_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f, bool filtered,
                   long* off);
int rollout_init(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                 bool filtered, const scnattn_params* w, const float* enc, const float* tags, int start_token, float* ws);
int rollout_steps(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                  bool filtered, const scnattn_params* w, const float* enc, int end_token, float inv_temp,
                  unsigned long long seed, unsigned draw, int greedy_first, int t0, int n_steps, float* ws);
// scoring given captions: the _sc form of the rollout driver
int score_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes);
int score_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* off);
int score_init(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
               const float* enc, const float* tags, int start_token, const int* targets, long ld_tok, const int* ntok,
               float* ws);
int score_steps(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                const float* enc, float inv_temp, int t0, int n_steps, float* ws);
// scheduled sampling: the _ss form of the rollout driver
int mix_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes);
int mix_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* off);
int mix_init(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
             const float* enc, const float* tags, int start_token, const int* gold, long ld_tok, const int* nmix, float* ws);
int mix_steps(hipStream_t st, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
              const float* enc, float inv_temp, float prob, unsigned long long seed, unsigned draw, int greedy, int t0,
              int n_steps, float* ws);

int pool_desc(const scnattn_pool* p, PoolDesc& out) {
    out = PoolDesc{0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    SCN_ARG(p, "scnattn_pool: null descriptor");
    SCN_ARG(p->Q > 0 && p->qtap_max > 0 && p->qtap_max <= 64, "scnattn_pool: bad Q / qtap_max");
    SCN_ARG(p->tap_idx && p->tap_w && p->qtap_idx && p->qtap_w && p->col_w, "scnattn_pool: null table");
    out = PoolDesc{p->Q, p->qtap_max, p->tap_idx, p->tap_w, p->qtap_idx, p->qtap_w, p->col_w};
    return 0;
}

}  // namespace scn

using namespace scn;
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int scnattn_version(void) { return SCNATTN_VERSION; }
const char* scnattn_last_error(void) { return last_error(); }
int scnattn_plan_next(scnattn_launch_plan* out) { t_plan_out = out; return 0; }

// Process-wide knobs.  Two kinds only (the experiment switches of rounds 1-2 -- fuse_attn, chains,
// attn_handoff, cgemm_stagger, cgemm_w41, cgemm_vec, bn_gfirst, skinny_tail -- are gone with the code paths they selected):
//   * what a CALLER chooses per process: "decoder_bf16" (storage mode of the decode step, BASELINE configs[4]), "profile"
//     (HIP-event timing of the recurrence loops for bench.py);
//   * split-K / tile policy overrides that only tools/ (sweeps) and the tests of both policies set.
int scnattn_set_option(const char* name, int value) {
    struct Opt { const char* name; int* var; int lo, hi; };
    static const Opt opts[] = {
        {"decoder_bf16", &g_dec_bf16, 0, 2},   {"profile", &g_profile, 0, 2},
        {"ksplit", &g_ksplit_scale, 0, SCN_MAX_KSPLIT}, {"attn_depth", &g_attn_depth, 0, 1},
        {"use_cgemm", &g_use_cgemm, 0, 1},     {"cgemm_mi", &g_cgemm_mi, 0, 2},
        {"cgemm_combine", &g_cgemm_combine, 0, 2}, {"cgemm_combine_max", &g_cgemm_combine_max, 1, 128},
        {"cgemm_target", &g_cgemm_target, 1, 1 << 20}, {"cgemm_kmin", &g_cgemm_kmin, 16, 1 << 20},
        {"gemm_target", &g_gemm_target, 1, 1 << 20},   {"gemm_gate", &g_gemm_gate, 1, 1 << 20},
        {"gemm_kmin", &g_gemm_kmin, 16, 1 << 20},      {"gemm_kmin_small", &g_gemm_kmin_small, 16, 1 << 20},
    };
    for (const Opt& o : opts)
        if (name && std::strcmp(name, o.name) == 0) {
            if (value < o.lo || value > o.hi) { set_error("scnattn_set_option: %s out of range [%d, %d]", o.name, o.lo, o.hi); return -1; }
            *o.var = value;
            return 0;
        }
    set_error("scnattn_set_option: unknown option '%s'", name ? name : "(null)");
    return -1;
}

int scnattn_profile_collect(double* out6) {
    if (!out6) { set_error("scnattn_profile_collect: NULL"); return -1; }
    return profile_collect(out6);
}

// The search entry points over the one driver (sixteen here, the eight _div and the eight _con forms below).  The single search is the one-member ensemble of weight 1 in mode 0
// that records its attention maps when it has any; the _opt forms are the calls whose options may not be NULL.
static int alpha_of(const scnattn_dims* d) { return d && d->has_att ? 0 : -1; }
static const float k_one[1] = {1.f};
static int no_options() { SCN_ARG(false, "search options are NULL"); return -1; }

int scnattn_beam_workspace(const scnattn_dims* d, int K, int max_steps, size_t* bytes) {
    return search_workspace(1, d, alpha_of(d), nullptr, nullptr, nullptr, K, max_steps, bytes);
}
int scnattn_beam_layout(const scnattn_dims* d, int K, int max_steps, long* offsets) {
    return search_layout(1, d, alpha_of(d), nullptr, nullptr, nullptr, K, max_steps, offsets);
}
int scnattn_beam_init(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_params* w, const float* enc,
                      const float* tags, int start_token, float* ws) {
    return search_init(ST(stream), 1, d, alpha_of(d), nullptr, nullptr, nullptr, K, max_steps, w, enc, tags ? &tags : nullptr,
                       start_token, ws);
}
int scnattn_beam_steps(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_params* w, const float* enc,
                       int end_token, int t0, int n_steps, float* ws) {
    return search_steps(ST(stream), 1, d, alpha_of(d), nullptr, nullptr, nullptr, K, max_steps, w, enc, k_one, 0, end_token, t0,
                        n_steps, ws);
}
int scnattn_beam_attn_scores(void* stream, int N, int K, int P, int A, const float* att1, const float* att2, int nslab,
                             long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                             const int32_t* nsrc, float* e) {
    return beam_attn_scores(ST(stream), N, K, P, A, att1, Slabs{att2, nslab, slab_stride, att2_ld}, dec_bias, w, b0, nsrc, e);
}
int scnattn_beam_attn_context(void* stream, int N, int K, int P, int E, const float* enc, const float* e, const float* gpre,
                              int nslab, long slab_stride, long gpre_ld, const float* gate_bias, const int32_t* nsrc,
                              float* alpha_out, float* awe, float* z) {
    return beam_attn_context(ST(stream), N, K, P, E, enc, e, Slabs{gpre, nslab, slab_stride, gpre_ld}, gate_bias, nsrc,
                             alpha_out, awe, z);
}
int scnattn_beam_row_topk(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                          const int32_t* nsrc, float* outv, int32_t* outi, int force_passes) {
    return beam_row_topk(ST(stream), N, K, V, logits, ld, scores, nsrc, outv, outi, force_passes);
}
// the member arrays of the two ensemble selection calls -> EnsRows
static int rows_of(int M, const float* const* logits, const long* ld, const float* w, EnsRows& e) {
    SCN_ARG(M >= 1 && M <= SCN_MAX_ENSEMBLE, "scnattn_beam_row_topk_ens: need 1 <= members <= 4");
    SCN_ARG(logits && ld && w, "scnattn_beam_row_topk_ens: null member arrays");
    e = EnsRows{};
    for (int m = 0; m < M; ++m) { e.p[m] = logits[m]; e.ld[m] = ld[m]; e.w[m] = w[m]; }
    return 0;
}
int scnattn_beam_row_topk_ens(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                              const float* w, int mode, const float* scores, const int32_t* nsrc, float* outv, int32_t* outi,
                              int force_passes) {
    EnsRows e;
    SCN_TRY(rows_of(M, logits, ld, w, e));
    return beam_row_topk_ens(ST(stream), N, K, V, M, e, mode, scores, nsrc, nullptr, outv, outi, force_passes);
}
int scnattn_ensemble_workspace(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member, size_t* bytes) {
    return search_workspace(M, dims, alpha_member, nullptr, nullptr, nullptr, K, max_steps, bytes);
}
int scnattn_ensemble_layout(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member, long* offsets) {
    return search_layout(M, dims, alpha_member, nullptr, nullptr, nullptr, K, max_steps, offsets);
}
int scnattn_ensemble_init(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                          const scnattn_params* w, const float* enc, const float* const* tags, int start_token, float* ws) {
    return search_init(ST(stream), M, dims, alpha_member, nullptr, nullptr, nullptr, K, max_steps, w, enc, tags, start_token, ws);
}
int scnattn_ensemble_steps(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                           const scnattn_params* w, const float* enc, const float* member_w, int mode, int end_token, int t0,
                           int n_steps, float* ws) {
    return search_steps(ST(stream), M, dims, alpha_member, nullptr, nullptr, nullptr, K, max_steps, w, enc, member_w, mode, end_token, t0,
                        n_steps, ws);
}
int scnattn_beam_merge(void* stream, int N, int K, int V, int end_token, int t, const float* candv, const int32_t* candi,
                       void* const* state) {
    if (!state) { set_error("scnattn_beam_merge: state is NULL"); return -1; }
    if (N <= 0 || K < 1 || K > SCN_MAX_BEAM) { set_error("scnattn_beam_merge: bad N / beam size"); return -1; }
    const BeamState s{N * K, (float*)state[6], (int*)state[1], (int*)state[2], (int*)state[3], (int*)state[4],
                      (float*)state[5], (int*)state[0], (float*)state[7], (int*)state[8], (int*)state[9], (int*)state[10],
                      (int*)state[11]};
    return beam_merge(ST(stream), N, K, V, end_token, t, candv, candi, s);
}
int scnattn_beam_advance(void* stream, int N, int K, int D, int M, int V, const float* hs, const float* cs,
                         const int32_t* parent_t, const int32_t* token_t, const float* table, float* hd, float* cd,
                         float* emb) {
    return beam_advance(ST(stream), N, K, D, M, V, hs, cs, parent_t, token_t, table, hd, cd, emb);
}

int scnattn_beam_workspace_opt(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt, size_t* bytes) {
    return opt ? search_workspace(1, d, alpha_of(d), opt, nullptr, nullptr, K, max_steps, bytes) : no_options();
}
int scnattn_beam_layout_opt(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt, long* offsets) {
    return opt ? search_layout(1, d, alpha_of(d), opt, nullptr, nullptr, K, max_steps, offsets) : no_options();
}
int scnattn_beam_init_opt(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_params* w, const float* enc, const float* tags, int start_token, float* ws) {
    return opt ? search_init(ST(stream), 1, d, alpha_of(d), opt, nullptr, nullptr, K, max_steps, w, enc, tags ? &tags : nullptr,
                             start_token, ws)
               : no_options();
}
int scnattn_beam_steps_opt(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_params* w, const float* enc, int end_token, int t0, int n_steps, float* ws) {
    return opt ? search_steps(ST(stream), 1, d, alpha_of(d), opt, nullptr, nullptr, K, max_steps, w, enc, k_one, 0, end_token, t0,
                              n_steps, ws)
               : no_options();
}
int scnattn_ensemble_workspace_opt(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, size_t* bytes) {
    return opt ? search_workspace(M, dims, alpha_member, opt, nullptr, nullptr, K, max_steps, bytes) : no_options();
}
int scnattn_ensemble_layout_opt(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, long* offsets) {
    return opt ? search_layout(M, dims, alpha_member, opt, nullptr, nullptr, K, max_steps, offsets) : no_options();
}
int scnattn_ensemble_init_opt(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_params* w, const float* enc,
                              const float* const* tags, int start_token, float* ws) {
    return opt ? search_init(ST(stream), M, dims, alpha_member, opt, nullptr, nullptr, K, max_steps, w, enc, tags, start_token, ws)
               : no_options();
}
int scnattn_ensemble_steps_opt(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_params* w, const float* enc,
                               const float* member_w, int mode, int end_token, int t0, int n_steps, float* ws) {
    return opt ? search_steps(ST(stream), M, dims, alpha_member, opt, nullptr, nullptr, K, max_steps, w, enc, member_w, mode, end_token,
                              t0, n_steps, ws)
               : no_options();
}
// The _div forms: opt may be NULL, div may not.
static int no_diversity() { SCN_ARG(false, "the diversity is NULL"); return -1; }

int scnattn_beam_workspace_div(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                               const scnattn_diversity* div, size_t* bytes) {
    return div ? search_workspace(1, d, alpha_of(d), opt, div, nullptr, K, max_steps, bytes) : no_diversity();
}
int scnattn_beam_layout_div(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                            const scnattn_diversity* div, long* offsets) {
    return div ? search_layout(1, d, alpha_of(d), opt, div, nullptr, K, max_steps, offsets) : no_diversity();
}
int scnattn_beam_init_div(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_diversity* div, const scnattn_params* w, const float* enc, const float* tags,
                          int start_token, float* ws) {
    return div ? search_init(ST(stream), 1, d, alpha_of(d), opt, div, nullptr, K, max_steps, w, enc, tags ? &tags : nullptr,
                             start_token, ws)
               : no_diversity();
}
int scnattn_beam_steps_div(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_diversity* div, const scnattn_params* w, const float* enc, int end_token, int t0,
                           int n_steps, float* ws) {
    return div ? search_steps(ST(stream), 1, d, alpha_of(d), opt, div, nullptr, K, max_steps, w, enc, k_one, 0, end_token, t0,
                              n_steps, ws)
               : no_diversity();
}
int scnattn_ensemble_workspace_div(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, const scnattn_diversity* div, size_t* bytes) {
    return div ? search_workspace(M, dims, alpha_member, opt, div, nullptr, K, max_steps, bytes) : no_diversity();
}
int scnattn_ensemble_layout_div(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, const scnattn_diversity* div, long* offsets) {
    return div ? search_layout(M, dims, alpha_member, opt, div, nullptr, K, max_steps, offsets) : no_diversity();
}
int scnattn_ensemble_init_div(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_diversity* div, const scnattn_params* w,
                              const float* enc, const float* const* tags, int start_token, float* ws) {
    return div ? search_init(ST(stream), M, dims, alpha_member, opt, div, nullptr, K, max_steps, w, enc, tags, start_token, ws)
               : no_diversity();
}
int scnattn_ensemble_steps_div(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_diversity* div, const scnattn_params* w,
                               const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps,
                               float* ws) {
    return div ? search_steps(ST(stream), M, dims, alpha_member, opt, div, nullptr, K, max_steps, w, enc, member_w, mode, end_token,
                              t0, n_steps, ws)
               : no_diversity();
}
int scnattn_beam_merge_groups(void* stream, int N, int K, int Kg, float penalty, int V, int end_token, int t,
                              const float* candv, const int32_t* candi, void* const* state) {
    if (!state) { set_error("scnattn_beam_merge_groups: state is NULL"); return -1; }
    if (N <= 0 || K < 1 || K > SCN_MAX_BEAM) { set_error("scnattn_beam_merge_groups: bad N / beam size"); return -1; }
    const BeamState s{N * K, (float*)state[6], (int*)state[1], (int*)state[2], (int*)state[3], (int*)state[4],
                      (float*)state[5], (int*)state[0], (float*)state[7], (int*)state[8], (int*)state[9], (int*)state[10],
                      (int*)state[11]};
    return beam_merge_groups(ST(stream), N, K, Kg, penalty, V, end_token, t, candv, candi, s);
}
int scnattn_beam_row_topk_groups(void* stream, int N, int K, int Kg, int V, const float* logits, long ld, const float* scores,
                                 const int32_t* nsrc, float* outv, int32_t* outi, int force_passes) {
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM && V >= K, "scnattn_beam_row_topk_groups: need 1 <= beam size <= 8 <= vocab_size");
    SCN_ARG(Kg >= 1 && K % Kg == 0, "scnattn_beam_row_topk_groups: the slots per group must divide the beam size");
    SCN_ARG(logits && scores && nsrc && outv && outi && ld >= V, "scnattn_beam_row_topk_groups: bad argument");
    return beam_row_topk_ens(ST(stream), N, K, V, 1, EnsRows{{logits}, {ld}, {1.f}}, 0, scores, nsrc, nullptr, outv, outi,
                             force_passes, Kg);
}

// The _con forms: opt may be NULL, con may not.
static int no_constraints() { SCN_ARG(false, "the constraints are NULL"); return -1; }

int scnattn_beam_workspace_con(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                               const scnattn_constraints* con, size_t* bytes) {
    return con ? search_workspace(1, d, alpha_of(d), opt, nullptr, con, K, max_steps, bytes) : no_constraints();
}
int scnattn_beam_layout_con(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                            const scnattn_constraints* con, long* offsets) {
    return con ? search_layout(1, d, alpha_of(d), opt, nullptr, con, K, max_steps, offsets) : no_constraints();
}
int scnattn_beam_init_con(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_constraints* con, const scnattn_params* w, const float* enc, const float* tags,
                          int start_token, float* ws) {
    return con ? search_init(ST(stream), 1, d, alpha_of(d), opt, nullptr, con, K, max_steps, w, enc, tags ? &tags : nullptr,
                             start_token, ws)
               : no_constraints();
}
int scnattn_beam_steps_con(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_constraints* con, const scnattn_params* w, const float* enc, int end_token, int t0,
                           int n_steps, float* ws) {
    return con ? search_steps(ST(stream), 1, d, alpha_of(d), opt, nullptr, con, K, max_steps, w, enc, k_one, 0, end_token, t0,
                              n_steps, ws)
               : no_constraints();
}
int scnattn_ensemble_workspace_con(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, const scnattn_constraints* con, size_t* bytes) {
    return con ? search_workspace(M, dims, alpha_member, opt, nullptr, con, K, max_steps, bytes) : no_constraints();
}
int scnattn_ensemble_layout_con(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, const scnattn_constraints* con, long* offsets) {
    return con ? search_layout(M, dims, alpha_member, opt, nullptr, con, K, max_steps, offsets) : no_constraints();
}
int scnattn_ensemble_init_con(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_constraints* con, const scnattn_params* w,
                              const float* enc, const float* const* tags, int start_token, float* ws) {
    return con ? search_init(ST(stream), M, dims, alpha_member, opt, nullptr, con, K, max_steps, w, enc, tags, start_token, ws)
               : no_constraints();
}
int scnattn_ensemble_steps_con(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_constraints* con, const scnattn_params* w,
                               const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps,
                               float* ws) {
    return con ? search_steps(ST(stream), M, dims, alpha_member, opt, nullptr, con, K, max_steps, w, enc, member_w, mode,
                              end_token, t0, n_steps, ws)
               : no_constraints();
}
int scnattn_beam_merge_banks(void* stream, int N, int K, int V, int end_token, int t, const float* candv, const int32_t* candi,
                             const float* reqv, const int32_t* reqi, const int32_t* required, int32_t* met,
                             void* const* state) {
    if (!state) { set_error("scnattn_beam_merge_banks: state is NULL"); return -1; }
    if (N <= 0 || K < 1 || K > SCN_MAX_BEAM) { set_error("scnattn_beam_merge_banks: bad N / beam size"); return -1; }
    BeamState s{N * K, (float*)state[6], (int*)state[1], (int*)state[2], (int*)state[3], (int*)state[4],
                (float*)state[5], (int*)state[0], (float*)state[7], (int*)state[8], (int*)state[9], (int*)state[10],
                (int*)state[11]};
    s.met = met;
    return beam_merge_banks(ST(stream), N, K, V, end_token, t, candv, candi, reqv, reqi, required, s);
}

// what step t of a search with `opt` excludes, for the selection kernel alone; the launcher checks the ranges
static int excl_of(const scnattn_search_options* opt, int end_token, int t, const int32_t* hist, int max_steps, BeamExcl& x) {
    SCN_ARG(opt, "search options are NULL");
    SCN_ARG(opt->n_banned >= 0 && opt->n_banned <= SCN_MAX_BANNED, "at most 64 banned tokens");
    SCN_ARG(end_token >= 0, "end token outside the vocabulary");
    SCN_ARG(opt->min_length >= 0 && opt->min_length <= max_steps - 1, "min_length must be in [0, max_steps - 1]");
    x = BeamExcl{};
    x.t = t;
    x.T = max_steps;
    x.g = opt->no_repeat_ngram;
    x.end_excl = t < opt->min_length ? end_token : -1;
    x.n_banned = opt->n_banned;
    x.hist = hist;
    for (int i = 0; i < opt->n_banned; ++i) {
        SCN_ARG(opt->banned[i] != end_token, "the end token may not be banned");
        x.banned[i] = opt->banned[i];
    }
    return 0;
}
int scnattn_beam_row_topk_opt(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                              const int32_t* nsrc, const scnattn_search_options* opt, int end_token, int t,
                              const int32_t* hist, int max_steps, float* outv, int32_t* outi, int force_passes) {
    BeamExcl x;
    SCN_TRY(excl_of(opt, end_token, t, hist, max_steps, x));
    SCN_ARG(end_token < V, "end token outside the vocabulary");
    const EnsRows e{{logits}, {ld}, {1.f}};
    return beam_row_topk_ens(ST(stream), N, K, V, 1, e, 0, scores, nsrc, &x, outv, outi, force_passes);
}
int scnattn_beam_row_topk_ens_opt(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                                  const float* w, int mode, const float* scores, const int32_t* nsrc,
                                  const scnattn_search_options* opt, int end_token, int t, const int32_t* hist,
                                  int max_steps, float* outv, int32_t* outi, int force_passes) {
    EnsRows e;
    SCN_TRY(rows_of(M, logits, ld, w, e));
    BeamExcl x;
    SCN_TRY(excl_of(opt, end_token, t, hist, max_steps, x));
    SCN_ARG(end_token < V, "end token outside the vocabulary");
    return beam_row_topk_ens(ST(stream), N, K, V, M, e, mode, scores, nsrc, &x, outv, outi, force_passes);
}
// the selection of a constrained search alone: opt may be NULL (nothing excluded); required / met on the device
static int excl_con_of(const scnattn_search_options* opt, int end_token, int t, const int32_t* hist, int max_steps, BeamExcl& x) {
    if (opt) return excl_of(opt, end_token, t, hist, max_steps, x);
    x = BeamExcl{};
    x.t = t;
    x.T = max_steps;
    x.end_excl = -1;
    return 0;
}
int scnattn_beam_row_topk_con(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                              const int32_t* nsrc, const scnattn_search_options* opt, int end_token, int t,
                              const int32_t* hist, int max_steps, const int32_t* required, const int32_t* met, float* outv,
                              int32_t* outi, float* reqv, int32_t* reqi, int force_passes) {
    BeamExcl x;
    SCN_TRY(excl_con_of(opt, end_token, t, hist, max_steps, x));
    const EnsRows e{{logits}, {ld}, {1.f}};
    const BeamCon c{required, met, end_token, reqv, reqi};
    return beam_row_topk_ens(ST(stream), N, K, V, 1, e, 0, scores, nsrc, &x, outv, outi, force_passes, 0, &c);
}
int scnattn_beam_row_topk_ens_con(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                                  const float* w, int mode, const float* scores, const int32_t* nsrc,
                                  const scnattn_search_options* opt, int end_token, int t, const int32_t* hist,
                                  int max_steps, const int32_t* required, const int32_t* met, float* outv, int32_t* outi,
                                  float* reqv, int32_t* reqi, int force_passes) {
    EnsRows e;
    SCN_TRY(rows_of(M, logits, ld, w, e));
    BeamExcl x;
    SCN_TRY(excl_con_of(opt, end_token, t, hist, max_steps, x));
    const BeamCon c{required, met, end_token, reqv, reqi};
    return beam_row_topk_ens(ST(stream), N, K, V, M, e, mode, scores, nsrc, &x, outv, outi, force_passes, 0, &c);
}
int scnattn_beam_advance_opt(void* stream, int N, int K, int D, int M, int V, int t, int max_steps, const float* hs,
                             const float* cs, const int32_t* parent_t, const int32_t* token_t, const float* table,
                             const int32_t* hist_src, int32_t* hist_dst, float* hd, float* cd, float* emb) {
    return beam_advance_opt(ST(stream), N, K, D, M, V, t, max_steps, hs, cs, parent_t, token_t, table, hist_src, hist_dst, hd,
                            cd, emb);
}

int scnattn_rollout_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes) {
    return rollout_workspace(d, K, max_steps, want_alpha, nullptr, false, bytes);
}
int scnattn_rollout_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets) {
    return rollout_layout(d, K, max_steps, want_alpha, nullptr, false, offsets);
}
int scnattn_rollout_init(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                         const float* enc, const float* tags, int start_token, float* ws) {
    return rollout_init(ST(stream), d, K, max_steps, want_alpha, nullptr, false, w, enc, tags, start_token, ws);
}
int scnattn_rollout_steps(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                          const float* enc, int end_token, float inv_temp, uint64_t seed, uint32_t draw, int greedy_first,
                          int t0, int n_steps, float* ws) {
    return rollout_steps(ST(stream), d, K, max_steps, want_alpha, nullptr, false, w, enc, end_token, inv_temp, seed, draw,
                         greedy_first, t0, n_steps, ws);
}
int scnattn_rollout_workspace_f(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* filter,
                                size_t* bytes) {
    return rollout_workspace(d, K, max_steps, want_alpha, filter, true, bytes);
}
int scnattn_rollout_layout_f(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* filter,
                             long* offsets) {
    return rollout_layout(d, K, max_steps, want_alpha, filter, true, offsets);
}
int scnattn_rollout_init_f(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha,
                           const scnattn_sample_filter* filter, const scnattn_params* w, const float* enc, const float* tags,
                           int start_token, float* ws) {
    return rollout_init(ST(stream), d, K, max_steps, want_alpha, filter, true, w, enc, tags, start_token, ws);
}
int scnattn_rollout_steps_f(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha,
                            const scnattn_sample_filter* filter, const scnattn_params* w, const float* enc, int end_token,
                            float inv_temp, uint64_t seed, uint32_t draw, int greedy_first, int t0, int n_steps, float* ws) {
    return rollout_steps(ST(stream), d, K, max_steps, want_alpha, filter, true, w, enc, end_token, inv_temp, seed, draw,
                         greedy_first, t0, n_steps, ws);
}
static int rollout_state_of(const char* who, int N, int K, int max_steps, void* const* state, RolloutState& s) {
    if (!state) { set_error("%s: state is NULL", who); return -1; }
    if (N <= 0 || K < 1 || K > SCN_MAX_BEAM) { set_error("%s: bad N / slot count", who); return -1; }
    s = RolloutState{N * K, max_steps, (int*)state[0], (int*)state[1], (int*)state[2], (int*)state[3], (float*)state[4],
                     (int*)state[5], (float*)state[6]};
    return 0;
}
int scnattn_rollout_pick(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, uint64_t seed,
                         uint32_t draw, int t, int greedy_first, int end_token, int max_steps, void* const* state) {
    RolloutState s;
    SCN_TRY(rollout_state_of("scnattn_rollout_pick", N, K, max_steps, state, s));
    return rollout_pick(ST(stream), N, K, V, logits, ld, inv_temp, seed, draw, t, greedy_first, end_token, s);
}
int scnattn_rollout_pick_f(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, uint64_t seed,
                           uint32_t draw, int t, int greedy_first, int end_token, int max_steps, void* const* state,
                           const scnattn_sample_filter* filter, int32_t* nkeep_t, int force_passes) {
    SCN_ARG(filter, "scnattn_rollout_pick_f: the sample filter is NULL");
    RolloutState s;
    SCN_TRY(rollout_state_of("scnattn_rollout_pick_f", N, K, max_steps, state, s));
    return rollout_pick_filtered(ST(stream), N, K, V, logits, ld, inv_temp, seed, draw, t, greedy_first, end_token,
                                 filter->top_k, filter->top_p, nkeep_t, force_passes, s);
}
int scnattn_rollout_advance(void* stream, int N, int K, int M, int V, const int32_t* token_t, const float* table, float* emb,
                            const int32_t* nopen, int32_t* nsrc) {
    return rollout_advance(ST(stream), N, K, M, V, token_t, table, emb, nopen, nsrc);
}
int scnattn_rollout_workspace_sc(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes) {
    return score_workspace(d, K, max_steps, want_alpha, bytes);
}
int scnattn_rollout_layout_sc(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets) {
    return score_layout(d, K, max_steps, want_alpha, offsets);
}
int scnattn_rollout_init_sc(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                            const float* enc, const float* tags, int start_token, const int32_t* targets, long ld_tok,
                            const int32_t* ntok, float* ws) {
    return score_init(ST(stream), d, K, max_steps, want_alpha, w, enc, tags, start_token, targets, ld_tok, ntok, ws);
}
int scnattn_rollout_steps_sc(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                             const float* enc, float inv_temp, int t0, int n_steps, float* ws) {
    return score_steps(ST(stream), d, K, max_steps, want_alpha, w, enc, inv_temp, t0, n_steps, ws);
}
int scnattn_rollout_score(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, int t, int max_steps,
                          void* const* state, const int32_t* target_t, int32_t* rank_t, int32_t* best_t) {
    RolloutState s;
    SCN_TRY(rollout_state_of("scnattn_rollout_score", N, K, max_steps, state, s));
    return rollout_score(ST(stream), N, K, V, logits, ld, inv_temp, t, target_t, rank_t, best_t, s);
}
int scnattn_rollout_workspace_ss(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes) {
    return mix_workspace(d, K, max_steps, want_alpha, bytes);
}
int scnattn_rollout_layout_ss(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets) {
    return mix_layout(d, K, max_steps, want_alpha, offsets);
}
int scnattn_rollout_init_ss(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                            const float* enc, const float* tags, int start_token, const int32_t* gold, long ld_tok,
                            const int32_t* nmix, float* ws) {
    return mix_init(ST(stream), d, K, max_steps, want_alpha, w, enc, tags, start_token, gold, ld_tok, nmix, ws);
}
int scnattn_rollout_steps_ss(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                             const float* enc, float inv_temp, float prob, uint64_t seed, uint32_t draw, int greedy, int t0,
                             int n_steps, float* ws) {
    return mix_steps(ST(stream), d, K, max_steps, want_alpha, w, enc, inv_temp, prob, seed, draw, greedy, t0, n_steps, ws);
}
int scnattn_rollout_pick_mixed(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, float prob,
                               uint64_t seed, uint32_t draw, int t, int greedy, int max_steps, void* const* state,
                               const int32_t* gold_t, int32_t* sample_t, int32_t* replaced_t) {
    RolloutState s;
    SCN_TRY(rollout_state_of("scnattn_rollout_pick_mixed", N, K, max_steps, state, s));
    return rollout_pick_mixed(ST(stream), N, K, V, logits, ld, inv_temp, prob, seed, draw, t, greedy, gold_t, sample_t,
                              replaced_t, s);
}

int scnattn_seq_workspace(const scnattn_dims* d, const scnattn_pool* pool, size_t* saved_bytes, size_t* scratch_bytes) {
    return seq_workspace(d, pool, saved_bytes, scratch_bytes);
}

int scnattn_seq_fwd(void* stream, const scnattn_dims* d, const scnattn_params* w, const float* enc,
                    const float* tags, const int64_t* caps, const int32_t* dl_dev, const int32_t* bt_host,
                    const float* drop_mask, float* saved, float* scratch, float* preds, float* alphas,
                    const scnattn_pool* pool) {
    return seq_fwd(ST(stream), d, w, enc, tags, caps, dl_dev, bt_host, drop_mask, saved, scratch, preds, alphas, pool);
}

int scnattn_seq_bwd(void* stream, const scnattn_dims* d, const scnattn_params* w, const float* enc,
                    const float* tags, const int64_t* caps, const int32_t* dl_dev, const int32_t* bt_host,
                    const float* drop_mask, const float* saved, float* scratch, const float* dpreds,
                    const float* dalphas, const scnattn_params* g, float* denc, float* dtags,
                    const scnattn_pool* pool) {
    return seq_bwd(ST(stream), d, w, enc, tags, caps, dl_dev, bt_host, drop_mask, saved, scratch, dpreds, dalphas, g,
                   denc, dtags, pool);
}

int scnattn_sgemm(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A,
                  long lda, const float* B, long ldb, float beta, float* C, long ldc, const float* bias,
                  const float* rowmask, int batch, long strideA, long strideB, long strideC) {
    return sgemm(ST(stream), transA != 0, transB != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, rowmask,
                 batch < 1 ? 1 : batch, strideA, strideB, strideC);
}

int scnattn_sgemm_ws(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A,
                     long lda, const float* B, long ldb, float beta, float* C, long ldc, const float* bias,
                     const float* rowmask, int batch, long strideA, long strideB, long strideC, float* ws,
                     long ws_floats) {
    return sgemm_ws(ST(stream), transA != 0, transB != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, rowmask,
                    batch < 1 ? 1 : batch, strideA, strideB, strideC, ws, ws ? ws_floats : 0);
}

static ConvExtra to_extra(const scnattn_conv_extra* e) {
    ConvExtra x;
    if (!e) return x;
    x.pro = e->pro; x.epi = e->epi; x.pro_ss = e->pro_ss;
    x.stat_partial = e->stat_partial; x.stat_shift = e->stat_shift;
    x.ez = e->ez; x.emean = e->emean; x.einvstd = e->einvstd; x.egamma = e->egamma; x.ebeta = e->ebeta; x.ldz = e->ldz;
    x.stride = e->stride < 1 ? 1 : e->stride; x.Hi = e->Hi; x.Wi = e->Wi; x.Ho = e->Ho; x.Wo = e->Wo;
    x.force_split = e->force_split; x.force_mi = e->force_mi;
    return x;
}

int scnattn_cgemm(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, long lda,
                  const float* B, long ldb, float beta, float* C, long ldc, const float* bias, const float* rowmask,
                  int batch, long strideA, long strideB, long strideC, float* ws, long ws_floats,
                  const scnattn_conv_extra* ex) {
    const ConvExtra x = to_extra(ex);
    return cgemm(ST(stream), transA != 0, transB != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, rowmask,
                 batch < 1 ? 1 : batch, strideA, strideB, strideC, ws, ws ? ws_floats : 0, ex ? &x : nullptr);
}

int scnattn_cgemm_row_tiles(int M) { return cgemm_row_tiles(M); }

int scnattn_conv1x1_fwd(void* stream, int R, int Cin, int Cout, const float* x, const float* w, float* y,
                        const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    const ConvExtra e = to_extra(ex);
    SCN_ARG(!ex || ex->pro != 2, "conv1x1_fwd: prologue must be on the input (pro = 1)");
    return cgemm(ST(stream), false, true, R, Cout, Cin, 1.f, x, Cin, w, Cin, 0.f, y, Cout, nullptr, nullptr, 1, 0, 0, 0,
                 ws, ws ? ws_floats : 0, ex ? &e : nullptr);
}

int scnattn_conv1x1_dgrad(void* stream, int R, int Cin, int Cout, const float* dy, const float* w, int w_transposed,
                          float beta, float* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    const ConvExtra e = to_extra(ex);
    SCN_ARG(!ex || (ex->pro == 0 && ex->stride <= 1), "conv1x1_dgrad: no prologue / stride here");
    if (w_transposed)   // w is [Cin][Cout]: dx = dy . (w^T)^T, both operands k-contiguous
        return cgemm(ST(stream), false, true, R, Cin, Cout, 1.f, dy, Cout, w, Cout, beta, dx, Cin, nullptr, nullptr, 1, 0,
                     0, 0, ws, ws ? ws_floats : 0, ex ? &e : nullptr);
    return cgemm(ST(stream), false, false, R, Cin, Cout, 1.f, dy, Cout, w, Cin, beta, dx, Cin, nullptr, nullptr, 1, 0, 0,
                 0, ws, ws ? ws_floats : 0, ex ? &e : nullptr);
}

int scnattn_conv1x1_wgrad(void* stream, int R, int Cin, int Cout, const float* dy, const float* x, float* dw,
                          const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    ConvExtra e = to_extra(ex);
    SCN_ARG(!ex || (ex->pro != 1 && ex->epi == 0), "conv1x1_wgrad: prologue must be on the input (pro = 2), no epilogue");
    return cgemm(ST(stream), true, false, Cout, Cin, R, 1.f, dy, Cout, x, Cin, 0.f, dw, Cin, nullptr, nullptr, 1, 0, 0, 0,
                 ws, ws ? ws_floats : 0, ex ? &e : nullptr);
}

// 3x3 convolution as an implicit GEMM (ConvExtra::c3): `c` channels per tap of the gathered map.  The output map is
// Ho x Wo = ceil(Hi / stride) x ceil(Wi / stride); mode 4 (d-input, stride 2) gathers from that map, every other mode from
// the Hi x Wi one.
static void set_c3(ConvExtra& e, int mode, int c, int N, int Hi, int Wi, int stride) {
    e.c3 = mode; e.c3c = c;
    e.Hi = Hi; e.Wi = Wi; e.Ho = (Hi - 1) / stride + 1; e.Wo = (Wi - 1) / stride + 1; e.stride = stride;
    e.c3_src_rows = mode == 4 ? (long)N * e.Ho * e.Wo : (long)N * Hi * Wi;
}

int scnattn_conv3x3_fwd(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* x,
                        const float* w, float* y, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && stride >= 1, "conv3x3_fwd: geometry");
    ConvExtra e = to_extra(ex);
    set_c3(e, 1, Cin, N, Hi, Wi, stride);
    return cgemm(ST(stream), false, true, N * e.Ho * e.Wo, Cout, 9 * Cin, 1.f, x, Cin, w, 9L * Cin, 0.f, y, Cout, nullptr,
                 nullptr, 1, 0, 0, 0, ws, ws ? ws_floats : 0, &e);
}

// eval BatchNorm epilogue (EPI 3): geometry and tuning from ex, the BatchNorm from bn; every check before the GPU is touched
static int bn_eval_extra(const char* who, int Cin, int Cout, const scnattn_bn_eval* bn, const scnattn_conv_extra* ex,
                         ConvExtra* e) {
    if (!bn) { set_error("%s: invalid argument: bn is NULL", who); return -1; }
    if (ex && (ex->pro != 0 || ex->epi != 0)) { set_error("%s: invalid argument: ex carries geometry only (pro = epi = 0)", who); return -1; }
    if (!(bn->gamma && bn->beta && bn->mean && bn->var)) { set_error("%s: invalid argument: null BatchNorm parameter / statistic", who); return -1; }
    if (Cin <= 0 || Cout <= 0 || Cin % 16 || Cout % 16) { set_error("%s: invalid argument: Cin and Cout must be positive multiples of 16", who); return -1; }
    if (!(aligned16(bn->gamma) && aligned16(bn->beta) && aligned16(bn->mean) && aligned16(bn->var))) {
        set_error("%s: invalid argument: BatchNorm vectors must be 16-byte aligned", who); return -1;
    }
    if (bn->res && (!aligned16(bn->res) || bn->ldres % 4 || bn->ldres < Cout)) {
        set_error("%s: invalid argument: res must be 16-byte aligned with ldres %% 4 == 0 and ldres >= Cout", who); return -1;
    }
    if (ex) {
        e->stride = ex->stride < 1 ? 1 : ex->stride; e->Hi = ex->Hi; e->Wi = ex->Wi; e->Ho = ex->Ho; e->Wo = ex->Wo;
        e->force_split = ex->force_split; e->force_mi = ex->force_mi;
    }
    e->epi = 3;
    e->egamma = bn->gamma; e->ebeta = bn->beta; e->emean = bn->mean; e->evar = bn->var; e->eeps = bn->eps;
    e->ez = bn->res; e->ldz = bn->res ? bn->ldres : 0; e->erelu = bn->relu != 0;
    return 0;
}

int scnattn_conv1x1_fwd_bn_eval(void* stream, int R, int Cin, int Cout, const float* x, const float* w, float* y,
                                const scnattn_bn_eval* bn, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    ConvExtra e;
    SCN_TRY(bn_eval_extra("conv1x1_fwd_bn_eval", Cin, Cout, bn, ex, &e));
    return cgemm(ST(stream), false, true, R, Cout, Cin, 1.f, x, Cin, w, Cin, 0.f, y, Cout, nullptr, nullptr, 1, 0, 0, 0,
                 ws, ws ? ws_floats : 0, &e);
}

int scnattn_conv3x3_fwd_bn_eval(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* x,
                                const float* w, float* y, const scnattn_bn_eval* bn, const scnattn_conv_extra* ex,
                                float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && (stride == 1 || stride == 2), "conv3x3_fwd_bn_eval: geometry");
    ConvExtra e;
    SCN_TRY(bn_eval_extra("conv3x3_fwd_bn_eval", Cin, Cout, bn, ex, &e));
    set_c3(e, 1, Cin, N, Hi, Wi, stride);
    return cgemm(ST(stream), false, true, N * e.Ho * e.Wo, Cout, 9 * Cin, 1.f, x, Cin, w, 9L * Cin, 0.f, y, Cout, nullptr,
                 nullptr, 1, 0, 0, 0, ws, ws ? ws_floats : 0, &e);
}

int scnattn_conv3x3_dgrad(void* stream, int N, int Hi, int Wi, int Cin, int Cout, const float* dy, const float* w,
                          float* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0, "conv3x3_dgrad: geometry");
    ConvExtra e = to_extra(ex);
    // stride 1: dy and dx maps have the same extent; the gathered (source) map is dy
    set_c3(e, 2, Cout, N, Hi, Wi, 1);
    return cgemm(ST(stream), false, false, N * Hi * Wi, Cin, 9 * Cout, 1.f, dy, Cout, w, 9L * Cin, 0.f, dx, Cin, nullptr,
                 nullptr, 1, 0, 0, 0, ws, ws ? ws_floats : 0, &e);
}

int scnattn_conv3x3_dgrad_strided(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* dy,
                                  const float* w, float* dx, float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && stride == 2 && Hi % 2 == 0 && Wi % 2 == 0, "conv3x3_dgrad_strided: stride 2, even map");
    ConvExtra e;
    // one launch, four parity classes of d-input pixels (grid.y), each a product over the taps that reach it
    set_c3(e, 4, Cout, N, Hi, Wi, 2);
    return cgemm(ST(stream), false, false, N * e.Ho * e.Wo, Cin, 9 * Cout, 1.f, dy, Cout, w, 9L * Cin, 0.f, dx, Cin, nullptr,
                 nullptr, 1, 0, 0, 0, ws, ws ? ws_floats : 0, &e);
}

int scnattn_conv3x3_wgrad(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* dy,
                          const float* x, float* dw, float* ws, long ws_floats, int k_slices) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && stride >= 1, "conv3x3_wgrad: geometry");
    // stride 1: the halo-staged kernel (csrc/conv3.hip); strided (layerN.0) or odd widths: the gather form of cgemm
    if (stride == 1 && k_slices >= 0 && conv3x3_wgrad_halo_ok(N, Hi, Wi, Cin, Cout, dy, x, dw))
        return conv3x3_wgrad_halo(ST(stream), N, Hi, Wi, Cin, Cout, dy, x, dw, ws, ws ? ws_floats : 0, k_slices);
    ConvExtra e;
    set_c3(e, 3, Cin, N, Hi, Wi, stride);
    return cgemm(ST(stream), true, false, Cout, 9 * Cin, N * e.Ho * e.Wo, 1.f, dy, Cout, x, Cin, 0.f, dw, 9L * Cin, nullptr,
                 nullptr, 1, 0, 0, 0, ws, ws ? ws_floats : 0, &e);
}

int scnattn_stem_tiles(int N, int H, int W) { return stem_tiles(N, H, W); }

int scnattn_stem_conv7(void* stream, int N, int H, int W, const float* x, long sn, long sc, long sh, long sw,
                       const float* w, long wn, long wc, long wh, long ww, float* z, float* stat_partial,
                       const float* stat_shift) {
    return stem_conv7(ST(stream), N, H, W, x, sn, sc, sh, sw, w, wn, wc, wh, ww, z, stat_partial, stat_shift);
}

int scnattn_stem_bn_relu_maxpool(void* stream, int N, int Hz, int Wz, int C, const float* z, const float* ss, void* out,
                                 int out_bf16) {
    return stem_bn_relu_maxpool(ST(stream), N, Hz, Wz, C, z, ss, out, out_bf16);
}

int scnattn_cgemm_stat_ld(int M) { return cgemm_stat_ld(M); }

int scnattn_bn_finalize(void* stream, long R, int C, const float* partial, int ldp, int nchunk, const float* shift,
                        float eps, float momentum, float* mean, float* invstd, float* run_mean, float* run_var,
                        const float* gamma, const float* beta, float* ss_out) {
    return bn_finalize_t(ST(stream), R, C, partial, ldp, nchunk, shift, eps, momentum, mean, invstd, run_mean, run_var, gamma,
                         beta, ss_out);
}

int scnattn_bn_apply_fin(void* stream, long R, int C, const void* z, const void* res, int bf16, const float* partial, int ldp,
                         int nchunk, const float* shift, float eps, float momentum, const float* gamma, const float* beta,
                         int relu, void* y, float* mean, float* invstd, float* run_mean, float* run_var, float* ss_out) {
    return bn_apply_fin(ST(stream), R, C, z, res, bf16, partial, ldp, nchunk, shift, eps, momentum, gamma, beta, relu, y, mean,
                        invstd, run_mean, run_var, ss_out);
}

int scnattn_bn_bwd_reduce(void* stream, int R, int C, const void* dy, const void* y, const void* z, int bf16, const float* mean,
                          const float* invstd, int relu, float* partial, int ldp_cap, void* gout, int* nchunk_out) {
    return bn_bwd_reduce_t(ST(stream), R, C, dy, y, z, bf16, mean, invstd, relu, partial, ldp_cap, gout, nchunk_out);
}

int scnattn_bn_bwd_dx_fin(void* stream, long R, int C, const void* g, const void* z, int bf16, const float* mean,
                          const float* invstd, const float* gamma, const float* partial, int ldp, int nchunk, float* dbeta,
                          float* dgamma, void* dz) {
    return bn_bwd_dx_fin(ST(stream), R, C, g, z, bf16, mean, invstd, gamma, partial, ldp, nchunk, dbeta, dgamma, dz);
}

// ---- mixed-precision (bf16) convolution path ---------------------------------------------------------------------------------
int scnattn_cgemm16(void* stream, int M, int N, int K, const void* A, long lda, const void* B, long ldb, float beta, void* C,
                    long ldc, int out_bf16, float* ws, long ws_floats, const scnattn_conv_extra* ex) {
    const ConvExtra x = to_extra(ex);
    return cgemm16(ST(stream), M, N, K, A, lda, B, ldb, beta, C, ldc, out_bf16, ws, ws ? ws_floats : 0, ex ? &x : nullptr, 0);
}

int scnattn_conv3x3_fwd16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* x, const void* w,
                          void* y, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && stride >= 1, "conv3x3_fwd16: geometry");
    ConvExtra e = to_extra(ex);
    set_c3(e, 1, Cin, N, Hi, Wi, stride);
    return cgemm16(ST(stream), N * e.Ho * e.Wo, Cout, 9 * Cin, x, Cin, w, 9L * Cin, 0.f, y, Cout, 1, ws, ws ? ws_floats : 0, &e, 0);
}

// eval BatchNorm epilogue on bf16 maps (EPI 3 of csrc/cgemm16.hip): the rules of bn_eval_extra for ex; the vectors, the
// residual and the widths are cgemm16's own checks, all before the GPU is touched
static int bn_eval16_extra(const char* who, const scnattn_bn_eval16* bn, const scnattn_conv_extra* ex, ConvExtra* e) {
    if (!bn) { set_error("%s: invalid argument: bn is NULL", who); return -1; }
    if (ex && (ex->pro != 0 || ex->epi != 0)) { set_error("%s: invalid argument: ex carries geometry only (pro = epi = 0)", who); return -1; }
    if (ex) {
        e->stride = ex->stride < 1 ? 1 : ex->stride; e->Hi = ex->Hi; e->Wi = ex->Wi; e->Ho = ex->Ho; e->Wo = ex->Wo;
        e->force_split = ex->force_split; e->force_mi = ex->force_mi;
    }
    e->epi = 3;
    e->egamma = bn->gamma; e->ebeta = bn->beta; e->emean = bn->mean; e->evar = bn->var; e->eeps = bn->eps;
    e->ez = (const float*)bn->res; e->ldz = bn->res ? bn->ldres : 0; e->erelu = bn->relu != 0;
    return 0;
}

int scnattn_conv1x1_fwd_bn_eval16(void* stream, int R, int Cin, int Cout, const void* x, const void* w, void* y,
                                  const scnattn_bn_eval16* bn, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    ConvExtra e;
    SCN_TRY(bn_eval16_extra("conv1x1_fwd_bn_eval16", bn, ex, &e));
    SCN_ARG(R > 0 && Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0, "conv1x1_fwd_bn_eval16: R > 0, Cin and Cout positive multiples of 8");
    return cgemm16(ST(stream), R, Cout, Cin, x, Cin, w, Cin, 0.f, y, Cout, 1, ws, ws ? ws_floats : 0, &e, 0);
}

int scnattn_conv3x3_fwd_bn_eval16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* x,
                                  const void* w, void* y, const scnattn_bn_eval16* bn, const scnattn_conv_extra* ex,
                                  float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && (stride == 1 || stride == 2), "conv3x3_fwd_bn_eval16: geometry");
    ConvExtra e;
    SCN_TRY(bn_eval16_extra("conv3x3_fwd_bn_eval16", bn, ex, &e));
    SCN_ARG(Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 8 == 0, "conv3x3_fwd_bn_eval16: Cin a positive multiple of 32, Cout of 8");
    set_c3(e, 1, Cin, N, Hi, Wi, stride);
    return cgemm16(ST(stream), N * e.Ho * e.Wo, Cout, 9 * Cin, x, Cin, w, 9L * Cin, 0.f, y, Cout, 1, ws, ws ? ws_floats : 0, &e, 0);
}

// wt: the TRANSPOSED bf16 weight copy [Cin][3][3][Cout] (scnattn_bf16_weights).  stride 1: a forward convolution of dy with
// flipped taps; stride 2: four parity classes in one launch.
int scnattn_conv3x3_dgrad16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* dy, const void* wt,
                            void* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats) {
    SCN_ARG(N > 0 && Hi > 0 && Wi > 0 && (stride == 1 || (stride == 2 && Hi % 2 == 0 && Wi % 2 == 0)), "conv3x3_dgrad16: geometry");
    ConvExtra e = to_extra(ex);
    SCN_ARG(stride == 1 || e.epi == 0, "conv3x3_dgrad16: the mask epilogue serves the stride-1 form only");
    if (stride == 1) {
        set_c3(e, 1, Cout, N, Hi, Wi, 1);
        return cgemm16(ST(stream), N * Hi * Wi, Cin, 9 * Cout, dy, Cout, wt, 9L * Cout, 0.f, dx, Cin, 1, ws, ws ? ws_floats : 0, &e, 1);
    }
    set_c3(e, 4, Cout, N, Hi, Wi, 2);
    return cgemm16(ST(stream), N * e.Ho * e.Wo, Cin, 9 * Cout, dy, Cout, wt, 9L * Cout, 0.f, dx, Cin, 1, ws, ws ? ws_floats : 0, &e, 0);
}

int scnattn_wgrad16_3x3(void* stream, int N, int H, int W, int Cin, int Cout, const void* dy, const void* x, float* dw,
                        float* ws, long ws_floats, int k_slices) {
    return wgrad16_3x3(ST(stream), N, H, W, Cin, Cout, dy, x, dw, ws, ws ? ws_floats : 0, k_slices);
}

int scnattn_wgrad16_rows(void* stream, int R, int Cin, int Cout, const void* dy, const void* x, long src_rows, float* dw,
                         long ldo, int gs, int gHi, int gWi, int gHo, int gWo, int goh, int gow, float* ws, long ws_floats,
                         int k_slices) {
    return wgrad16_rows(ST(stream), R, Cin, Cout, dy, x, src_rows, dw, ldo, gs, gHi, gWi, gHo, gWo, goh, gow, ws,
                        ws ? ws_floats : 0, k_slices);
}

int scnattn_bf16_weights(void* stream, int n, const scnattn_weight_desc* desc, const int* tile_prefix, int total_tiles) {
    static_assert(sizeof(scnattn_weight_desc) == sizeof(WeightDesc), "descriptor layout");
    return bf16_weights(ST(stream), n, reinterpret_cast<const WeightDesc*>(desc), tile_prefix, total_tiles);
}

int scnattn_bn_stats_fold(void* stream, int R, int C, const void* x, float eps, float momentum, float* partial,
                          float* mean, float* invstd, float* run_mean, float* run_var, const float* gamma,
                          const float* beta, float* ss_out) {
    return bn_stats(ST(stream), R, C, x, 0, eps, momentum, partial, mean, invstd, run_mean, run_var, gamma, beta, ss_out);
}

// wbf: 0 fp32 W; 1 bf16 W; 2 bf16 W and the bf16 matrix instruction (kernels.h)
static int skinny_entry(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg, const void* W,
                        long ldw, long wg, float* Y, long ldy, long yg, long yslab, int ksplit, int* ksplit_out, int wbf) {
    if (ksplit <= 0) ksplit = skinny_pick_ksplit(rows, N, K, groups);
    if (ksplit_out) *ksplit_out = ksplit;
    return skinny_gemm(ST(stream), rows, N, K, groups, X, ldx, xg, W, ldw, wg, Y, ldy, yg, yslab, ksplit, wbf);
}

int scnattn_skinny_gemm(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                        const float* W, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                        int ksplit, int* ksplit_out) {
    return skinny_entry(stream, rows, N, K, groups, X, ldx, xg, W, ldw, wg, Y, ldy, yg, yslab, ksplit, ksplit_out, 0);
}

int scnattn_skinny_gemm_bf16w(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                              const void* W_bf16, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                              int ksplit, int* ksplit_out) {
    return skinny_entry(stream, rows, N, K, groups, X, ldx, xg, W_bf16, ldw, wg, Y, ldy, yg, yslab, ksplit, ksplit_out, 1);
}

int scnattn_skinny_gemm_bf16(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                             const void* W_bf16, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                             int ksplit, int* ksplit_out) {
    return skinny_entry(stream, rows, N, K, groups, X, ldx, xg, W_bf16, ldw, wg, Y, ldy, yg, yslab, ksplit, ksplit_out, 2);
}

int scnattn_f32_to_bf16(void* stream, long n, const float* in, void* out) { return f32_to_bf16(ST(stream), n, in, out); }

int scnattn_attn_scores(void* stream, int rows, int P, int A, const float* att1, const float* att2, int nslab,
                        long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                        float* e, float* att2_out) {
    return attn_scores(ST(stream), rows, P, A, att1, Slabs{att2, nslab, slab_stride, att2_ld}, dec_bias, w, b0, e,
                       att2_out);
}

int scnattn_attn_context(void* stream, int rows, int P, int E, const float* enc, const float* e,
                         const float* gpre, int nslab, long slab_stride, long gpre_ld, const float* gate_bias,
                         float* alpha_out, long alpha_ld, float* alpha_save, float* awe, float* gate, float* z) {
    return attn_context(ST(stream), rows, P, E, enc, e, Slabs{gpre, nslab, slab_stride, gpre_ld}, gate_bias,
                        alpha_out, alpha_ld, alpha_save, awe, gate, z);
}

int scnattn_mean_pixels(void* stream, int rows, int P, int E, const float* enc, float* out) {
    return mean_pixels(ST(stream), rows, P, E, enc, out);
}

int scnattn_attn_dalpha(void* stream, int rows, int P, int E, const float* enc, const float* dawe,
                        const float* dalpha_in, long dalpha_in_ld, float* dalpha) {
    return attn_dalpha(ST(stream), rows, P, E, enc, dawe, dalpha_in, dalpha_in_ld, dalpha);
}

int scnattn_attn_softmax_bwd(void* stream, int rows, int P, int A, const float* att1, const float* att2,
                             const float* w, const float* alpha, const float* dalpha, float* de, float* datt2,
                             long datt2_ld) {
    return attn_softmax_bwd(ST(stream), rows, P, A, att1, att2, w, alpha, dalpha, de, datt2, datt2_ld);
}

int scnattn_attn_datt1_post_blocks(int B, int P) { return attn_datt1_post_blocks(B, P); }

int scnattn_attn_datt1_post(void* stream, int B, int P, int A, int T, const int32_t* dl, const float* att1,
                            const float* att2_all, const float* de_all, const float* w, float* datt1,
                            float* dwpart) {
    return attn_datt1_post(ST(stream), B, P, A, T, dl, att1, att2_all, de_all, w, datt1, dwpart, nullptr);
}

// The instances the sequence drivers launch and the entries above do not reach: the streamed operand as raw bf16, and the
// pooled forms.  Thin wrappers like the ones above; a scnattn_pool goes through the same check the drivers make.
int scnattn_attn_scores_bf16(void* stream, int rows, int P, int A, const void* att1_bf16, const float* att2, int nslab,
                             long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                             float* e, float* att2_out) {
    return attn_scores(ST(stream), rows, P, A, att1_bf16, Slabs{att2, nslab, slab_stride, att2_ld}, dec_bias, w, b0, e,
                       att2_out, true);
}

int scnattn_attn_context_bf16(void* stream, int rows, int P, int E, const void* enc_bf16, const float* e,
                              const float* gpre, int nslab, long slab_stride, long gpre_ld, const float* gate_bias,
                              float* alpha_out, long alpha_ld, float* alpha_save, float* awe, float* gate, float* z) {
    return attn_context(ST(stream), rows, P, E, enc_bf16, e, Slabs{gpre, nslab, slab_stride, gpre_ld}, gate_bias,
                        alpha_out, alpha_ld, alpha_save, awe, gate, z, true);
}

int scnattn_attn_dalpha_bf16(void* stream, int rows, int P, int E, const void* enc_bf16, const float* dawe,
                             const float* dalpha_in, long dalpha_in_ld, float* dalpha) {
    return attn_dalpha(ST(stream), rows, P, E, enc_bf16, dawe, dalpha_in, dalpha_in_ld, dalpha, true);
}

int scnattn_attn_softmax_bwd_bf16(void* stream, int rows, int P, int A, const void* att1_bf16, const float* att2,
                                  const float* w, const float* alpha, const float* dalpha, float* de, float* datt2,
                                  long datt2_ld) {
    return attn_softmax_bwd(ST(stream), rows, P, A, att1_bf16, att2, w, alpha, dalpha, de, datt2, datt2_ld, true);
}

int scnattn_attn_datt1_post_bf16(void* stream, int B, int P, int A, int T, const int32_t* dl, const void* att1_bf16,
                                 const float* att2_all, const float* de_all, const float* w, float* datt1,
                                 float* dwpart) {
    return attn_datt1_post(ST(stream), B, P, A, T, dl, att1_bf16, att2_all, de_all, w, datt1, dwpart, nullptr, true);
}

int scnattn_attn_context_pooled(void* stream, int rows, int P, int E, const void* x, int bf16, const scnattn_pool* pool,
                                const float* e, const float* gpre, int nslab, long slab_stride, long gpre_ld,
                                const float* gate_bias, float* alpha_out, long alpha_ld, float* alpha_save,
                                float* alphaq_save, float* awe, float* gate, float* z) {
    PoolDesc pd;
    SCN_TRY(pool_desc(pool, pd));
    return attn_context_pooled(ST(stream), rows, P, E, x, pd, e, Slabs{gpre, nslab, slab_stride, gpre_ld}, gate_bias,
                               alpha_out, alpha_ld, alpha_save, alphaq_save, awe, gate, z, bf16 != 0);
}

int scnattn_attn_softmax_bwd_pooled(void* stream, int rows, int P, int A, const void* att1, int bf16, const float* att2,
                                    const float* w, const float* alpha, const scnattn_pool* pool, const float* dalphaq,
                                    const float* dalpha_in, long dalpha_in_ld, float* de, float* datt2, long datt2_ld) {
    PoolDesc pd;
    SCN_TRY(pool_desc(pool, pd));
    return attn_softmax_bwd_pooled(ST(stream), rows, P, A, att1, att2, w, alpha, pd, dalphaq, dalpha_in, dalpha_in_ld, de,
                                   datt2, datt2_ld, bf16 != 0);
}

int scnattn_weighted_rows(void* stream, int rows, int Q, int E, const float* x, const float* wts, float* out) {
    return weighted_rows(ST(stream), rows, Q, E, x, wts, out);
}

int scnattn_pool_expand(void* stream, int B, int P, int A, const scnattn_pool* pool, const float* y, const float* bias,
                        float* out) {
    PoolDesc pd;
    SCN_TRY(pool_desc(pool, pd));
    return pool_expand(ST(stream), B, P, A, pd, y, bias, out);
}

int scnattn_pool_transpose(void* stream, int B, int P, int A, const scnattn_pool* pool, const float* in, float* out) {
    PoolDesc pd;
    SCN_TRY(pool_desc(pool, pd));
    return pool_transpose(ST(stream), B, P, A, pd, in, out);
}

int scnattn_add_bcast_rows_w(void* stream, int B, int Q, int E, const float* wts, const float* v, float* out) {
    return add_bcast_rows_w(ST(stream), B, Q, E, wts, v, out);
}

int scnattn_scn_mix_fwd(void* stream, int rows, int F4, const float* pz, int pz_nslab, long pz_stride, long pz_ld,
                        const float* ex, const float* ph, int ph_nslab, long ph_stride, long ph_ld,
                        const float* qx, const float* qh, float* pa, float* phs, float* xcat) {
    return scn_mix_fwd(ST(stream), rows, F4, Slabs{pz, pz_nslab, pz_stride, pz_ld}, ex,
                       Slabs{ph, ph_nslab, ph_stride, ph_ld}, qx, qh, pa, phs, xcat);
}

int scnattn_lstm_fwd(void* stream, int rows, int H, const float* r, int nslab, long slab_stride, long r_ld,
                     long r_gate_stride, const float* bih, const float* bhh, const float* c_prev, float* gates,
                     float* c_new, float* h_new, float* tanhc) {
    return lstm_fwd(ST(stream), rows, H, Slabs{r, nslab, slab_stride, r_ld}, r_gate_stride, bih, bhh, c_prev, gates,
                    c_new, h_new, tanhc);
}

int scnattn_lstm_bwd(void* stream, int rows, int rows_next, int H, const float* dh_fc, const float* dh_next,
                     int nslab, long slab_stride, long dh_ld, float* dc, const float* gates, const float* c_prev,
                     const float* tanhc, float* dr) {
    return lstm_bwd(ST(stream), rows, rows_next, H, dh_fc, Slabs{dh_next, nslab, slab_stride, dh_ld}, dc, gates,
                    c_prev, tanhc, dr);
}

int scnattn_scn_mix_bwd(void* stream, int rows, int F4, const float* dxcat, int nslab, long slab_stride, long dx_ld,
                        long dx_gate_stride, const float* qx, const float* qh, const float* pa, const float* phs,
                        float* dpx, float* dph, long dph_ld, float* dqx_acc, float* dqh_acc) {
    return scn_mix_bwd(ST(stream), rows, F4, Slabs{dxcat, nslab, slab_stride, dx_ld}, dx_gate_stride, qx, qh, pa, phs,
                       dpx, dph, dph_ld, dqx_acc, dqh_acc);
}

int scnattn_gate_bwd(void* stream, int rows, int E, const float* dz, int nslab, long slab_stride, long dz_ld,
                     const float* awe, const float* gate, float* dawe, float* dgpre, long dgpre_ld) {
    return gate_bwd(ST(stream), rows, E, Slabs{dz, nslab, slab_stride, dz_ld}, awe, gate, dawe, dgpre, dgpre_ld);
}

int scnattn_transpose2d(void* stream, int R, int C, const float* in, long ldi, float* out, long ldo) {
    return transpose2d(ST(stream), R, C, in, ldi, out, ldo);
}

int scnattn_colsum(void* stream, int R, int N, const float* X, long ld, float* out, float beta) {
    return colsum(ST(stream), R, N, X, ld, out, beta);
}

int scnattn_mul_bcast(void* stream, int T, int B, int N, const float* x, const float* q, float* out) {
    return mul_bcast(ST(stream), T, B, N, x, q, out);
}

// The sequence glue of scnattn_seq_fwd / scnattn_seq_bwd, each launcher alone (csrc/misc.hip).  The launchers return 0 for an
// empty problem before they look at anything else; these entries refuse null operands and bad shapes first, so that a
// caller's mistake is an error whatever the sizes.
int scnattn_gather_rows_tm(void* stream, int B, int T, int L, int M, const int64_t* caps, const float* table, int V,
                           float* out_tm) {
    SCN_ARG(B >= 0 && T >= 0 && M >= 0 && V > 0 && T <= L, "gather_rows_tm: bad shape");
    SCN_ARG(caps && table && out_tm, "gather_rows_tm: null operand");
    return gather_rows_tm(ST(stream), B, T, L, M, (const long long*)caps, table, V, out_tm);
}

int scnattn_scatter_add_rows_tm(void* stream, int B, int T, int L, int M, const int64_t* caps, const int32_t* decode_lengths,
                                const float* demb_tm, int V, float* dtable, int32_t* present) {
    SCN_ARG(B >= 0 && T >= 0 && M >= 0 && V > 0 && T <= L, "scatter_add_rows_tm: bad shape");
    SCN_ARG(caps && decode_lengths && demb_tm && dtable && present, "scatter_add_rows_tm: null operand");
    return scatter_add_rows_tm(ST(stream), B, T, L, M, (const long long*)caps, decode_lengths, demb_tm, V, dtable, present);
}

int scnattn_hidden_to_bm(void* stream, int B, int T, int D, const int32_t* decode_lengths, const float* hs_tm,
                         const float* mask_bm, float* out_bm, float* rowmask) {
    SCN_ARG(B >= 0 && T >= 0 && D >= 0, "hidden_to_bm: bad shape");
    SCN_ARG(decode_lengths && hs_tm && out_bm, "hidden_to_bm: null operand");
    return hidden_to_bm(ST(stream), B, T, D, decode_lengths, hs_tm, mask_bm, out_bm, rowmask);
}

int scnattn_hidden_from_bm(void* stream, int B, int T, int D, const int32_t* decode_lengths, const float* dbm,
                           const float* mask_bm, float* out_tm) {
    SCN_ARG(B >= 0 && T >= 0 && D >= 0, "hidden_from_bm: bad shape");
    SCN_ARG(decode_lengths && dbm && out_tm, "hidden_from_bm: null operand");
    return hidden_from_bm(ST(stream), B, T, D, decode_lengths, dbm, mask_bm, out_tm);
}

int scnattn_colsum_masked(void* stream, int R, int N, const float* X, long ld, const float* rowmask, float* out, float beta) {
    SCN_ARG(R >= 0 && N >= 0 && ld >= N, "colsum_masked: bad shape");
    SCN_ARG(X && rowmask && out, "colsum_masked: null operand");
    return colsum_masked(ST(stream), R, N, X, ld, rowmask, out, beta);
}

int scnattn_reduce_slabs(void* stream, int rows, int N, const float* slabs, int nslab, long slab_stride, long slab_ld,
                         float* out) {
    SCN_ARG(rows >= 0 && N >= 0 && nslab >= 1 && nslab <= 16 && slab_ld >= N, "reduce_slabs: bad shape (1 to 16 slabs)");
    SCN_ARG(slabs && out, "reduce_slabs: null operand");
    return reduce_slabs(ST(stream), rows, N, Slabs{slabs, nslab, slab_stride, slab_ld}, out);
}

int scnattn_copy2d(void* stream, int R, int C, const float* in, long ldi, float* out, long ldo) {
    SCN_ARG(R >= 0 && C >= 0 && ldi >= C && ldo >= C, "copy2d: bad shape");
    SCN_ARG(in && out, "copy2d: null operand");
    return copy2d(ST(stream), R, C, in, ldi, out, ldo);
}

int scnattn_add_bcast_rows(void* stream, int B, int P, int E, const float* v, float scale, float* x) {
    SCN_ARG(B >= 0 && P > 0 && E > 0, "add_bcast_rows: bad shape");
    SCN_ARG(v && x, "add_bcast_rows: null operand");
    return add_bcast_rows(ST(stream), B, P, E, v, scale, x);
}

int scnattn_pool_permute_fwd(void* stream, int B, int C, int Hin, int Win, int Ho, int Wo, const float* x,
                             long sxb, long sxc, long sxh, long sxw, float* y) {
    return pool_permute_fwd(ST(stream), B, C, Hin, Win, Ho, Wo, x, sxb, sxc, sxh, sxw, y);
}

int scnattn_pool_permute_bwd(void* stream, int B, int C, int Hin, int Win, int Ho, int Wo, const float* dy,
                             float* dx, long sxb, long sxc, long sxh, long sxw) {
    return pool_permute_bwd(ST(stream), B, C, Hin, Win, Ho, Wo, dy, dx, sxb, sxc, sxh, sxw);
}

int scnattn_caption_loss_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                             long ldt, const int32_t* decode_lengths, long n_tokens, const float* alphas, float alpha_c,
                             float* row_lse, float* row_loss, float* sm1, float* reg_part, float* loss) {
    return caption_loss_fwd(ST(stream), B, T, V, P, scores, (const long long*)targets, ldt, decode_lengths, n_tokens,
                            alphas, alpha_c, row_lse, row_loss, sm1, reg_part, loss);
}

int scnattn_caption_loss_metrics_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                     long ldt, const int32_t* decode_lengths, long n_tokens, const float* alphas,
                                     float alpha_c, float* row_lse, float* row_loss, float* sm1, float* reg_part,
                                     float* loss, int k, int32_t* row_rank, int32_t* preds, long ldp, int32_t* hits) {
    return caption_loss_metrics_fwd(ST(stream), B, T, V, P, scores, (const long long*)targets, ldt, decode_lengths,
                                    n_tokens, alphas, alpha_c, row_lse, row_loss, sm1, reg_part, loss, k, row_rank, preds,
                                    ldp, hits);
}

int scnattn_caption_loss_bwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                             long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_lse,
                             const float* sm1, float alpha_c, const float* grad_loss, float* dscores, float* dalphas) {
    return caption_loss_bwd(ST(stream), B, T, V, P, scores, (const long long*)targets, ldt, decode_lengths, n_tokens,
                            row_lse, sm1, alpha_c, grad_loss, dscores, dalphas);
}

int scnattn_caption_loss_weighted_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                      long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_weight,
                                      const float* alphas, float alpha_c, float* row_lse, float* row_loss, float* sm1,
                                      float* reg_part, float* loss) {
    return caption_loss_weighted_fwd(ST(stream), B, T, V, P, scores, (const long long*)targets, ldt, decode_lengths,
                                     n_tokens, row_weight, alphas, alpha_c, row_lse, row_loss, sm1, reg_part, loss);
}

int scnattn_caption_loss_weighted_bwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                      long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_weight,
                                      const float* row_lse, const float* sm1, float alpha_c, const float* grad_loss,
                                      float* dscores, float* dalphas) {
    return caption_loss_weighted_bwd(ST(stream), B, T, V, P, scores, (const long long*)targets, ldt, decode_lengths,
                                     n_tokens, row_weight, row_lse, sm1, alpha_c, grad_loss, dscores, dalphas);
}

int scnattn_tag_pool_fwd(void* stream, int B, int HW, int C, const void* x, int bf16, long sb, long sp, long sc,
                         const float* ks, long ldk, float* pooled, long ldo) {
    return tag_pool_fwd(ST(stream), B, HW, C, x, bf16, sb, sp, sc, ks, ldk, pooled, ldo);
}

int scnattn_tag_pool_bwd(void* stream, int B, int HW, int C, const float* dpooled, long ldd, const float* ks, long ldk,
                         void* dx, int bf16, long sb, long sp, long sc) {
    return tag_pool_bwd(ST(stream), B, HW, C, dpooled, ldd, ks, ldk, dx, bf16, sb, sp, sc);
}

int scnattn_bce_fwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt, float* probs,
                    long ldp, float* rows, float* out) {
    return bce_fwd(ST(stream), B, S, z, ldz, targets, ldt, probs, ldp, rows, out);
}

int scnattn_bce_bwd(void* stream, int B, int S, const float* probs, long ldp, const float* targets, long ldt,
                    const float* grad_loss, float* dz, long lddz) {
    return bce_bwd(ST(stream), B, S, probs, ldp, targets, ldt, grad_loss, dz, lddz);
}

int scnattn_tagloss_fwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt,
                        const float* pos_weight, const scnattn_tag_loss_options* opt, float* probs, long ldp, float* rows,
                        float* out) {
    return tagloss_fwd(ST(stream), B, S, z, ldz, targets, ldt, pos_weight, opt, probs, ldp, rows, out);
}

int scnattn_tagloss_bwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt,
                        const float* pos_weight, const scnattn_tag_loss_options* opt, const float* grad_loss, float* dz,
                        long lddz) {
    return tagloss_bwd(ST(stream), B, S, z, ldz, targets, ldt, pos_weight, opt, grad_loss, dz, lddz);
}

int scnattn_u8_gather_normalize(void* stream, const uint8_t* src, long n_src, const int64_t* idx, long n_out, int C,
                                long HW, const float* lut, void* dst, int dst_bf16, int channels_last) {
    return u8_gather_normalize(ST(stream), src, n_src, (const long long*)idx, n_out, C, HW, lut, dst, dst_bf16,
                               channels_last);
}

int scnattn_u8_mean_grey(void* stream, const uint8_t* src, long N, long HW, int64_t* sums, float* grey) {
    return u8_mean_grey(ST(stream), src, N, HW, (long long*)sums, grey);
}

int scnattn_augment_draw(void* stream, long n, const int64_t* sid, int epoch, uint64_t seed, const scnattn_augment_config* cfg,
                         int H, int W, float* params) {
    return augment_draw(ST(stream), n, (const long long*)sid, epoch, (unsigned long long)seed, cfg, H, W, params);
}

int scnattn_u8_gather_augment(void* stream, const uint8_t* src, long N, const int64_t* idx, long n, int H, int W,
                              const float* params, const float* grey, const float* mean, const float* std, void* dst,
                              int dst_bf16, int channels_last) {
    return u8_gather_augment(ST(stream), src, N, (const long long*)idx, n, H, W, params, grey, mean, std, dst, dst_bf16,
                             channels_last);
}

int scnattn_u8_resize_bilinear(void* stream, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                               const scnattn_image_desc* desc_dev, int N, const int32_t* taps, long taps_len, int OH,
                               int OW, const float* lut, void* dst, int dst_kind, int channels_last) {
    return u8_resize_bilinear(ST(stream), src, src_bytes, desc_host, desc_dev, N, taps, taps_len, OH, OW, lut, dst,
                              dst_kind, channels_last);
}

int scnattn_u8_resize_taps(void* stream, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                           const scnattn_image_desc* desc_dev, int N, const int32_t* taps_host, const int32_t* taps_dev,
                           long taps_len, int OH, int OW, const float* lut, void* dst, int dst_kind, int channels_last) {
    return u8_resize_taps(ST(stream), src, src_bytes, desc_host, desc_dev, N, taps_host, taps_dev, taps_len, OH, OW, lut,
                          dst, dst_kind, channels_last);
}

int scnattn_attn_strips(int OH) {
    const int n = attn_strips(OH);
    if (n < 0) set_error("scnattn_attn_strips: OH outside 1..SCNATTN_OVERLAY_MAX_OUT");
    return n;
}

int scnattn_attn_expand(void* stream, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh,
                        int OH, int OW, float* S, float* lohi, float* partial) {
    return attn_expand(ST(stream), alphas, n_maps, h, w, Mv, Mh, OH, OW, S, lohi, partial);
}

int scnattn_attn_overlay(void* stream, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh,
                         int OH, int OW, const float* S, const float* partial, const uint8_t* img, int n_img,
                         const int32_t* img_index_host, const int32_t* img_index_dev, const float* beta, uint8_t* out) {
    return attn_overlay(ST(stream), alphas, n_maps, h, w, Mv, Mh, OH, OW, S, partial, img, n_img, img_index_host,
                        img_index_dev, beta, out);
}

int scnattn_text_max_len(void) { return text_max_len(); }

int scnattn_text_ngram_stats(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                             int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                             int n_skip_ref, int32_t* stats) {
    return text_ngram_stats(ST(stream), N, R, hyp, Lh, hyp_len, ref, Lr, ref_len, skip_hyp, n_skip_hyp, skip_ref, n_skip_ref,
                            stats);
}

int scnattn_text_lcs(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
                     const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
                     int32_t* lcs, double* score, double* mean) {
    return text_lcs(ST(stream), N, R, hyp, Lh, hyp_len, ref, Lr, ref_len, skip_hyp, n_skip_hyp, skip_ref, n_skip_ref, lcs,
                    score, mean);
}

int scnattn_text_ref_keys(void* stream, int n, int N, int R, const int32_t* ref, int Lr, const int32_t* ref_len,
                          const int32_t* skip_ref, int n_skip_ref, int64_t* keys, int32_t* flag) {
    return text_ref_keys(ST(stream), n, N, R, ref, Lr, ref_len, skip_ref, n_skip_ref, keys, flag);
}

int scnattn_text_cider(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                       int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                       int n_skip_ref, const int64_t* table_keys, const int32_t* table_df, const long* table_off, long n_images,
                       double* score, double* mean, int32_t* flag) {
    return text_cider(ST(stream), N, R, hyp, Lh, hyp_len, ref, Lr, ref_len, skip_hyp, n_skip_hyp, skip_ref, n_skip_ref,
                      table_keys, table_df, table_off, n_images, score, mean, flag);
}

int scnattn_tag_store_size(int S, long cap, size_t* score_bytes, size_t* label_bytes) {
    return tag_store_size(S, cap, score_bytes, label_bytes);
}

int scnattn_tag_rows(void* stream, int B, int S, const float* probs, long ld_probs, const void* targets, int targets_u8,
                     long ld_targets, long row0, long cap, const int32_t* ks, int nk, float* store_scores, uint8_t* store_labels,
                     double* row_ap, int32_t* row_npos, int32_t* row_hits, int32_t* flag) {
    return tag_rows(ST(stream), B, S, probs, ld_probs, targets, targets_u8, ld_targets, row0, cap, ks, nk, store_scores,
                    store_labels, row_ap, row_npos, row_hits, flag);
}

int scnattn_tag_cols(void* stream, int S, long n, long cap, const float* store_scores, const uint8_t* store_labels,
                     const float* thresholds, int nt, double* col_ap, int32_t* col_npos, int32_t* col_counts,
                     int32_t* col_agree) {
    return tag_cols(ST(stream), S, n, cap, store_scores, store_labels, thresholds, nt, col_ap, col_npos, col_counts, col_agree);
}

int scnattn_tag_finalize(void* stream, int S, long n, const int32_t* ks, int nk, int nt, const double* row_ap,
                         const int32_t* row_npos, const int32_t* row_hits, const double* col_ap, const int32_t* col_npos,
                         const int32_t* col_counts, const int32_t* col_agree, const int32_t* flag, double* summary) {
    return tag_finalize(ST(stream), S, n, ks, nk, nt, row_ap, row_npos, row_hits, col_ap, col_npos, col_counts, col_agree, flag,
                        summary);
}

long scnattn_resize_table_ints(int in_size, int out_size) {
    const long n = resize_table_ints(in_size, out_size);
    if (n < 0) set_error("scnattn_resize_table_ints: size outside 1..SCNATTN_RESIZE_MAX_DIM");
    return n;
}

int scnattn_bn_workspace_floats(int C) { return bn_max_chunks() * 2 * C; }

int scnattn_bn_stats(void* stream, int R, int C, const void* x, int bf16, float eps, float momentum, float* partial,
                     float* mean, float* invstd, float* run_mean, float* run_var) {
    return bn_stats(ST(stream), R, C, x, bf16, eps, momentum, partial, mean, invstd, run_mean, run_var);
}

int scnattn_bn_apply(void* stream, int R, int C, const void* z, const void* res, int bf16, const float* mean,
                     const float* invstd, const float* gamma, const float* beta, int relu, void* y) {
    return bn_apply(ST(stream), R, C, z, res, bf16, mean, invstd, gamma, beta, relu, y);
}

int scnattn_bn_bwd(void* stream, int R, int C, const void* dy, const void* y, const void* z, int bf16,
                   const float* mean, const float* invstd, const float* gamma, const float* beta, int relu, int train,
                   float* partial, float* dbeta, float* dgamma, void* dz, void* dres) {
    return bn_bwd(ST(stream), R, C, dy, y, z, bf16, mean, invstd, gamma, beta, relu, train, partial, dbeta, dgamma, dz, dres);
}

int scnattn_clamp_adam(void* stream, long n, float* p, const float* g, float* m, float* v, double lr,
                       double beta1, double beta2, double eps, int step, double clip, double gscale) {
    return clamp_adam(ST(stream), n, p, g, m, v, lr, beta1, beta2, eps, step, clip, gscale);
}

}  // extern "C"
