// Batched beam search driver: the decode step of sequence.cpp's forward loop over a FIXED N*K rows (K slots per image),
// followed by the selection kernels of beam.hip.  init does the teacher-forced driver's set-up (weight re-layout, att1 once
// per IMAGE, qx / qh from the tags, the initial state), steps enqueues whole steps; the host only reads `open_images`
// between chunks of steps and the token / parent / alpha records at the end.
// fp32 only: option "decoder_bf16" is not looked at here.
//
// ONE driver (search_workspace / search_layout / search_init / search_steps) serves the thirty-two entry points
// scnattn_beam_*, scnattn_ensemble_* and their _opt, _div and _con forms (csrc/api.cpp): M decoders step under one search
// state, the single search being M = 1 with weight 1 in mode 0; search options, the diversity
// of a search in groups and the constraints of a constrained search are pointers that are null
// without them.  With a diversity the selection takes the group size, beam_merge_groups replaces beam_merge and the
// attention kernels take att_live; with constraints the selection runs in its constrained flavour and beam_merge_banks
// replaces beam_merge: the same launches.
//
// Launches per step, all in search_steps: per member the decode part (decode_step; with attention skinny
// h.[Wd^T|Wbeta^T|Ha], beam_attn_scores, beam_attn_context, skinny z.Wa[M:], skinny emb.Wa[:M], scn_mix_fwd, skinny gates,
// lstm_fwd, fc (sgemm_ws: one or two launches) = 9-10; without attention 6-7), then ONE beam_row_topk_ens, ONE beam_merge
// and beam_advance per member: (decode launches) + 2 + M, which for the single search is 12-13 with attention and 9-10
// without.  Options add no launch: the selection takes the step's exclusions and the first member's advance also writes the
// per-beam word history, which the workspace gains.
//
// The rollout driver of self-critical training (scnattn_rollout_*, at the end of this file) shares the set-up and the decode
// part of a step (decode_setup, decode_step) and ends a step with rollout_pick + rollout_advance (csrc/rollout.hip).
#include <hip/hip_runtime.h>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"
#include "driver.h"

namespace scn {

namespace {

constexpr long BEAM_GEMM_WS_FLOATS = 8L << 20;     // 32 MiB of split-K partials (fc over N*K rows, the set-up products)

// what one decode step over R = N*K rows reads and writes (decode_step below): shared by the search and the rollout
struct StepWs {
    // state: zero-filled by init, so that rows of dead slots that no kernel writes are finite
    float *hA, *cA, *hB, *cB, *emb, *alpha, *z, *e, *qxr, *qhr, *pa, *phs, *xcat, *gates, *ex, *logits;
    size_t state_floats;
    // set-up results and scratch
    float *att1, *qx, *qh, *mean_enc, *h0, *c0, *WcatA, *WD, *slabA, *slabC, *slabD, *gws;
};

// The workspace of one search: M decoders (the single search: one) under ONE search state.  The members read the same enc
// [N,P,E] and share the vocabulary; each keeps its own StepWs (state, set-up results) and they share the split-K scratch,
// since everything runs on one stream in order.  The attention maps of one member (alpha_member) are recorded; the other
// attention members pass a null alpha_t, as the rollout does.
struct SearchWs {
    BeamState s;
    float* candv;
    int* candi;
    float* alpha;       // [T][R][P] of alpha_member, or null
    int* hist;          // [2][R][T] with search options, else null
    int G;              // groups of a diverse search; 1 without: the per-group state arrays hold N*G entries
    // a constrained search, else null: the required candidates [R][4] of the step, the table int [N][4]
    // (s.met [R] is the per-slot mask)
    float* reqv;
    int *reqi, *req;
    size_t state_floats;
    StepWs m[SCN_MAX_ENSEMBLE];
};

struct RolloutWs : StepWs {
    RolloutState s;
    int* nkeep;             // [T][R] words kept by the sample filter (the _f form of the driver), else null
    int *rank, *best, *target;      // [T][R] each: the records and the given tokens of a scoring run (_sc), else null
    int *sample, *replaced, *gold;  // [T][R] each: the records and the gold words of a scheduled-sampling run (_ss), else null
};

inline int* ints(float* p) { return reinterpret_cast<int*>(p); }

// the two halves of a StepWs: what init zero-fills (rows of dead slots that no kernel writes stay finite), and the set-up
// results and scratch
void carve_step_state(Carver& c, const scnattn_dims& d, long R, StepWs& b) {
    const int P = d.P, E = d.E, D = d.D, F = d.F, F4 = 4 * F;
    b.hA = c.take(sz(R, D));
    b.cA = c.take(sz(R, D));
    b.hB = c.take(sz(R, D));
    b.cB = c.take(sz(R, D));
    b.emb = c.take(sz(R, d.M));
    b.z = d.has_att ? c.take(sz(R, E)) : nullptr;
    b.e = d.has_att ? c.take(sz(R, P)) : nullptr;
    b.qxr = c.take(sz(R, F4));
    b.qhr = c.take(sz(R, F4));
    b.pa = c.take(sz(R, F4));
    b.phs = c.take(sz(R, F4));
    b.xcat = c.take(sz(R, 4, 2 * F));
    b.gates = c.take(sz(R, 4 * D));
    b.ex = c.take(sz(R, F4));
    b.logits = c.take(sz(R, d.V));
}

// shared_gws: the split-K scratch of another StepWs on the same stream (an ensemble's members run one after the other)
void carve_step_setup(Carver& c, const scnattn_dims& d, long R, StepWs& b, const StepWs* shared_gws = nullptr) {
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, NA = ncatA(d);
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
    b.gws = shared_gws ? shared_gws->gws : c.take(BEAM_GEMM_WS_FLOATS);
}

// In this order: the BeamState fields, alpha, the members' step state, candv / candi, the history, att_live -- which init
// zero-fills (state_floats) -- then the members' set-up results with the shared split-K scratch.
// div: a diverse search, whose per-group arrays hold N*G entries and which also keeps att_live [N] (behind the history).
// con: a constrained search, which keeps met, the required candidates and the table behind those.
size_t carve_search(int M, const scnattn_dims* d, int K, int T, int alpha_member, bool hist, const scnattn_diversity* div,
                    bool con, float* base, SearchWs& b) {
    Carver c(base);
    const int N = d[0].B, P = d[0].P;
    const long R = (long)N * K;
    b.G = div ? div->groups : 1;
    const long NG = (long)N * b.G;
    b.s.R = (int)R;
    b.s.scores = c.take(R);
    b.s.nsrc = ints(c.take(NG));
    b.s.kk = ints(c.take(NG));
    b.s.ncomp = ints(c.take(NG));
    b.s.best_idx = ints(c.take(NG));
    b.s.best_score = c.take(NG);
    b.s.open_images = ints(c.take(1));
    b.s.comp_score = c.take(R);
    b.s.comp_step = ints(c.take(R));
    b.s.comp_parent = ints(c.take(R));
    b.s.token = ints(c.take(sz(T, R)));
    b.s.parent = ints(c.take(sz(T, R)));
    const bool alpha = alpha_member >= 0 && alpha_member < M && d[alpha_member].has_att;
    b.alpha = alpha ? c.take(sz(T, R, P)) : nullptr;
    for (int m = 0; m < M; ++m) {
        b.m[m].alpha = m == alpha_member ? b.alpha : nullptr;
        carve_step_state(c, d[m], R, b.m[m]);
    }
    b.candv = c.take(sz(R, K));
    b.candi = ints(c.take(sz(R, K)));
    b.hist = hist ? ints(c.take(sz(2, R, T))) : nullptr;
    b.s.att_live = div ? ints(c.take(N)) : nullptr;
    b.s.met = con ? ints(c.take(R)) : nullptr;
    b.reqv = con ? c.take(sz(R, SCN_MAX_REQUIRED)) : nullptr;
    b.reqi = con ? ints(c.take(sz(R, SCN_MAX_REQUIRED))) : nullptr;
    b.req = con ? ints(c.take(sz(N, SCN_MAX_REQUIRED))) : nullptr;
    b.state_floats = c.off;
    for (int m = 0; m < M; ++m) {
        b.m[m].state_floats = b.state_floats;
        carve_step_setup(c, d[m], R, b.m[m], m ? &b.m[0] : nullptr);
    }
    return c.off * sizeof(float);
}

// Where results live in a workspace: off[i] = p[i] - base in 4-byte elements, -1 for a null p[i].  A layout query carves
// from layout_base(), which is never dereferenced: only differences are taken.
inline float* layout_base() { return reinterpret_cast<float*>(uintptr_t(1) << 40); }

void offsets_from(const float* base, const void* const* p, int n, long* off) {
    for (int i = 0; i < n; ++i) off[i] = p[i] ? (long)(reinterpret_cast<const float*>(p[i]) - base) : -1;
}

// The refusals of a search with options (include/scnattn.h); end_token < 0: not known to this call.
int check_options(const scnattn_search_options* o, int V, int K, int T, int end_token) {
    SCN_ARG(o, "search options are NULL");
    SCN_ARG(o->min_length >= 0 && o->min_length <= T - 1, "min_length must be in [0, max_steps - 1]");
    SCN_ARG(o->no_repeat_ngram >= 0 && o->no_repeat_ngram <= SCN_MAX_NGRAM, "no_repeat_ngram must be in [0, 8]");
    SCN_ARG(o->n_banned >= 0 && o->n_banned <= SCN_MAX_BANNED, "at most 64 banned tokens");
    for (int i = 0; i < o->n_banned; ++i) {
        SCN_ARG(o->banned[i] >= 0 && o->banned[i] < V, "a banned token lies outside the vocabulary");
        SCN_ARG(o->banned[i] != end_token, "the end token may not be banned");
    }
    SCN_ARG(end_token < V, "end token outside the vocabulary");
    SCN_ARG((long)V - o->n_banned - 1 - (o->no_repeat_ngram >= 1 ? T : 0) >= K,
            "the options may leave a row fewer than beam_size candidates "
            "(need vocab_size - banned - 1 - (no_repeat_ngram ? max_steps : 0) >= beam_size)");
    return 0;
}

// The refusals of a constrained search (include/scnattn.h); o: the options, null without; start / end < 0: not known to this
// call.  Reads the HOST table of the constraints.
int check_constraints(const scnattn_constraints* c, const scnattn_search_options* o, const scnattn_diversity* v, int N, int V,
                      int K, int T, int start_token, int end_token) {
    SCN_ARG(c && c->required, "the constraints (or their table of required words) are NULL");
    SCN_ARG(!v, "constraints and groups do not compose: a search takes required words or a diversity, not both");
    SCN_ARG(c->n_images == N, "the constraints must hold one row of required words per image");
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM, "beam_size must be in [1, 8]");
    for (int n = 0; n < N; ++n) {
        const int32_t* r = c->required + (long)n * SCN_MAX_REQUIRED;
        bool ended = false;
        for (int i = 0; i < SCN_MAX_REQUIRED; ++i) {
            if (r[i] == -1) { ended = true; continue; }
            SCN_ARG(!ended, "a required word stands behind a -1 of its row (the words first, then the padding)");
            SCN_ARG(r[i] >= 0 && r[i] < V, "a required word lies outside the vocabulary");
            SCN_ARG(r[i] != start_token && r[i] != end_token && r[i] != c->pad_token,
                    "<start>, <end> and <pad> may not be required");
            for (int q = 0; q < i; ++q) SCN_ARG(r[q] != r[i], "a required word occurs twice in an image's list");
            if (o)
                for (int q = 0; q < o->n_banned && q < SCN_MAX_BANNED; ++q)
                    SCN_ARG(o->banned[q] != r[i], "a required word is banned by the options");
        }
    }
    const int nb = o ? o->n_banned : 0, g = o ? o->no_repeat_ngram : 0;
    SCN_ARG((long)V - nb - 1 - (g >= 1 ? T : 0) - SCN_MAX_REQUIRED >= K,
            "options and required words may leave a row fewer than beam_size candidates "
            "(need vocab_size - banned - 1 - (no_repeat_ngram ? max_steps : 0) - 4 >= beam_size)");
    return 0;
}

// The refusals of a diverse search (include/scnattn.h); K is the total G * Kg.
int check_diversity(const scnattn_diversity* v, int K) {
    SCN_ARG(v, "the diversity is NULL");
    SCN_ARG(v->groups >= 1, "groups must be at least 1");
    SCN_ARG(K >= 1 && K <= SCN_MAX_BEAM, "beam_size must be in [1, 8]");
    SCN_ARG(K % v->groups == 0, "beam_size (the total over the groups) must be a multiple of groups");
    SCN_ARG(v->penalty >= 0.f && v->penalty < INFINITY, "the diversity penalty must be finite and not negative");
    return 0;
}

// what step t excludes; hist: the [2][R][T] buffers, step t reads buffer t & 1 and its advance writes the other
// o null (a constrained search without options): nothing is excluded
BeamExcl step_excl(const scnattn_search_options* o, int t, int T, long R, int end_token, const int* hist) {
    BeamExcl x{};
    x.t = t;
    x.T = T;
    x.end_excl = -1;
    if (!o) return x;
    x.g = o->no_repeat_ngram;
    x.end_excl = t < o->min_length ? end_token : -1;
    x.n_banned = o->n_banned;
    x.hist = hist + (long)(t & 1) * R * T;
    for (int i = 0; i < o->n_banned; ++i) x.banned[i] = o->banned[i];
    return x;
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

int check_search(int M, const scnattn_dims* d, int K, int T, int alpha_member) {
    SCN_ARG(M >= 1 && M <= SCN_MAX_ENSEMBLE, "an ensemble has 1 to 4 members");
    SCN_ARG(d, "dims is NULL");
    for (int m = 0; m < M; ++m) {
        SCN_TRY(check_beam(d + m, K, T));
        SCN_ARG(d[m].B == d[0].B && d[m].P == d[0].P && d[m].E == d[0].E && d[m].V == d[0].V,
                "the members of an ensemble must agree in B, P, E and V");
    }
    SCN_ARG(alpha_member >= -1 && alpha_member < M, "alpha_member must be -1 or a member index");
    return 0;
}

// The set-up both drivers share: weight re-layout, att1 once per image, the tag factors, the initial state in every slot
// and the <start> embedding in every row.
int decode_setup(hipStream_t st, const scnattn_dims& d, int K, const scnattn_params* w, const float* enc, const float* tags,
                 int start_token, const StepWs& b) {
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F4 = 4 * d.F, M = d.M;
    const GemmWs gws{b.gws, BEAM_GEMM_WS_FLOATS};
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

// The decode part of one step over the R = N*K rows: (hin, cin, emb) -> (hout, cout, logits); the K rows of image n attend
// over att1[n] / enc[n] for nsrc[n] live slots.  Launches: skinny h.[Wd^T|Wbeta^T|Ha], beam_attn_scores, beam_attn_context,
// skinny z.Wa[M:], skinny emb.Wa[:M], scn_mix_fwd, skinny gates, lstm_fwd, fc (one or two launches).
int decode_step(hipStream_t st, const scnattn_dims& d, int K, const scnattn_params* w, const float* enc, const StepWs& b,
                const int* nsrc, float* alpha_t, const float* hin, const float* cin, float* hout, float* cout) {
    const int N = d.B, P = d.P, E = d.E, A = d.A, D = d.D, F = d.F, F4 = 4 * F, M = d.M, V = d.V;
    const int R = N * K, NA = ncatA(d), colph = d.has_att ? A + E : 0;
    const long RD = (long)R * D;
    const GemmWs gws{b.gws, BEAM_GEMM_WS_FLOATS};
    const float* WaM = d.has_att ? w->decode_step_weight_ia + (long)M * F4 : nullptr;
    const int ksA = pick(R, NA, D, 1);
    SCN_TRY(skinny_gemm(st, R, NA, D, 1, hin, D, 0, b.WcatA, NA, 0, b.slabA, NA, 0, (long)R * NA, ksA));
    const Slabs ph{b.slabA + colph, ksA, (long)R * NA, NA};
    Slabs pz{nullptr, 0, 0, 0};
    if (d.has_att) {
        const Slabs att2{b.slabA, ksA, (long)R * NA, NA}, gpre{b.slabA + A, ksA, (long)R * NA, NA};
        SCN_TRY(beam_attn_scores(st, N, K, P, A, b.att1, att2, w->attention_decoder_att_bias,
                                 w->attention_full_att_weight, w->attention_full_att_bias, nsrc, b.e));
        SCN_TRY(beam_attn_context(st, N, K, P, E, enc, b.e, gpre, w->f_beta_bias, nsrc,
                                  alpha_t, nullptr, b.z));
        const int ksC = pick(R, F4, E, 1);
        SCN_TRY(skinny_gemm(st, R, F4, E, 1, b.z, E, 0, WaM, F4, 0, b.slabC, F4, 0, (long)R * F4, ksC));
        pz = Slabs{b.slabC, ksC, (long)R * F4, F4};
    }
    SCN_TRY(skinny_gemm(st, R, F4, M, 1, b.emb, M, 0, w->decode_step_weight_ia, F4, 0, b.ex, F4, 0, (long)R * F4, 1));
    SCN_TRY(scn_mix_fwd(st, R, F4, pz, b.ex, ph, b.qxr, b.qhr, b.pa, b.phs, b.xcat));
    const int ksD = pick(R, D, 2 * F, 4);
    SCN_TRY(skinny_gemm(st, R, D, 2 * F, 4, b.xcat, 8 * F, 2 * F, b.WD, D, (long)2 * F * D, b.slabD, D, RD, 4 * RD, ksD));
    SCN_TRY(lstm_fwd(st, R, D, Slabs{b.slabD, ksD, 4 * RD, D}, RD, w->decode_step_bias_ih, w->decode_step_bias_hh, cin,
                     b.gates, cout, hout, nullptr));
    SCN_TRY(gemm(st, false, true, R, V, D, hout, D, w->fc_weight, D, 0.f, b.logits, V, gws, w->fc_bias));
    return 0;
}

}  // namespace

// ---- the search: M decoders under ONE search state; o: the search options, null without ------------
int search_workspace(int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                     const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, size_t* bytes) {
    if (v) SCN_TRY(check_diversity(v, K));
    SCN_TRY(check_search(M, d, K, max_steps, alpha_member));
    if (o) SCN_TRY(check_options(o, d[0].V, K, max_steps, -1));
    if (cn) SCN_TRY(check_constraints(cn, o, v, d[0].B, d[0].V, K, max_steps, -1, -1));
    SCN_ARG(bytes, "search_workspace: bytes is NULL");
    SearchWs b;
    *bytes = carve_search(M, d, K, max_steps, alpha_member, o != nullptr, v, cn != nullptr, nullptr, b);
    return 0;
}

// off[SCNATTN_BEAM_NOFF]: where the results live in the workspace, in 4-byte elements (order: include/scnattn.h); with
// options or a diversity off[SCNATTN_BEAM_NOFF_OPT], the history's offset (-1 without options) behind them; with
// constraints off[SCNATTN_BEAM_NOFF_CON], met and the required table behind that
int search_layout(int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                  const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, long* off) {
    if (v) SCN_TRY(check_diversity(v, K));
    SCN_TRY(check_search(M, d, K, max_steps, alpha_member));
    if (o) SCN_TRY(check_options(o, d[0].V, K, max_steps, -1));
    if (cn) SCN_TRY(check_constraints(cn, o, v, d[0].B, d[0].V, K, max_steps, -1, -1));
    SCN_ARG(off, "search_layout: offsets is NULL");
    SearchWs b;
    carve_search(M, d, K, max_steps, alpha_member, o != nullptr, v, cn != nullptr, layout_base(), b);
    const void* p[SCNATTN_BEAM_NOFF_CON] = {b.s.open_images, b.s.nsrc, b.s.kk, b.s.ncomp, b.s.best_idx, b.s.best_score,
                                            b.s.scores, b.s.comp_score, b.s.comp_step, b.s.comp_parent, b.s.token,
                                            b.s.parent, b.alpha, b.hist, b.s.met, b.req};
    offsets_from(layout_base(), p, cn ? SCNATTN_BEAM_NOFF_CON : (o || v) ? SCNATTN_BEAM_NOFF_OPT : SCNATTN_BEAM_NOFF, off);
    return 0;
}

// The history int32 [2][R][max_steps] of a search with options is zero-filled with the rest of the state.
// The required table of a constrained search is copied from the host behind that fill, and the call waits for the copy: the
// device never reads the caller's array (the four calls do, for their checks).
int search_init(hipStream_t st, int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, const scnattn_params* w,
                const float* enc, const float* const* tags, int start_token, float* ws) {
    if (v) SCN_TRY(check_diversity(v, K));
    SCN_TRY(check_search(M, d, K, max_steps, alpha_member));
    if (o) SCN_TRY(check_options(o, d[0].V, K, max_steps, -1));
    if (cn) {
        SCN_ARG(start_token >= 0, "search_init: start token outside the vocabulary");
        SCN_TRY(check_constraints(cn, o, v, d[0].B, d[0].V, K, max_steps, start_token, -1));
    }
    SCN_ARG(w && enc && tags && ws, "search_init: null argument");
    for (int m = 0; m < M; ++m) SCN_ARG(tags[m], "search_init: a member's tags are NULL");
    SCN_ARG(start_token >= 0 && start_token < d[0].V, "search_init: start token outside the vocabulary");
    SCN_ARG(aligned16(ws), "search_init: the workspace must be 16-byte aligned");
    SearchWs b;
    carve_search(M, d, K, max_steps, alpha_member, o != nullptr, v, cn != nullptr, ws, b);
    SCN_HIP(hipMemsetAsync(ws, 0, b.state_floats * sizeof(float), st));
    if (cn) {
        SCN_HIP(hipMemcpyAsync(b.req, cn->required, sz(d[0].B, SCN_MAX_REQUIRED) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        SCN_HIP(hipStreamSynchronize(st));
    }
    SCN_TRY(beam_state_init(st, d[0].B, K, b.s, b.G));
    for (int m = 0; m < M; ++m) SCN_TRY(decode_setup(st, d[m], K, w + m, enc, tags[m], start_token, b.m[m]));
    return 0;
}

// Steps t0 .. t0 + n_steps - 1 (0-based; clipped to max_steps).  A finished image's kernels are no-ops.  A step is, per
// member, decode_step with that member's hA/cA -> hB/cB, then ONE selection over the M logits buffers, ONE beam_merge, and
// per member beam_advance with its own table and state.  With options the selection takes what step t excludes, and one
// history serves all members: step t reads buffer t & 1, the first member's advance writes buffer (t + 1) & 1.
// With constraints the selection also takes them (and exclusions that may be empty) and beam_merge_banks replaces beam_merge.
int search_steps(hipStream_t st, int M, const scnattn_dims* d, int alpha_member, const scnattn_search_options* o,
                 const scnattn_diversity* v, const scnattn_constraints* cn, int K, int max_steps, const scnattn_params* w,
                 const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps, float* ws) {
    if (v) SCN_TRY(check_diversity(v, K));
    SCN_TRY(check_search(M, d, K, max_steps, alpha_member));
    if (o) {    // only a search with options needs to know <end>: min_length keeps it out, and it may not be banned
        SCN_ARG(end_token >= 0, "search_steps: end token outside the vocabulary");
        SCN_TRY(check_options(o, d[0].V, K, max_steps, end_token));
    }
    if (cn) {   // a caption may not end with a requirement open, and <end> may not be required
        SCN_ARG(end_token >= 0 && end_token < d[0].V, "search_steps: end token outside the vocabulary");
        SCN_TRY(check_constraints(cn, o, v, d[0].B, d[0].V, K, max_steps, -1, end_token));
    }
    SCN_ARG(w && enc && member_w && ws, "search_steps: null argument");
    SCN_ARG(t0 >= 0 && n_steps >= 0, "search_steps: negative step");
    const int N = d[0].B, P = d[0].P, V = d[0].V, R = N * K, T = max_steps;
    SearchWs b;
    carve_search(M, d, K, T, alpha_member, o != nullptr, v, cn != nullptr, ws, b);
    const int Kg = K / b.G;
    const BeamCon bc{b.req, b.s.met, end_token, b.reqv, b.reqi};
    // what the attention kernels take as the image's live slots: in groups the live rows are no prefix of the image's slots,
    // so K while any group is open; one group is the search without groups, its nsrc [N] the prefix length
    const int* att_live = b.G > 1 ? b.s.att_live : b.s.nsrc;
    EnsRows rows{};
    for (int m = 0; m < M; ++m) {
        rows.p[m] = b.m[m].logits;
        rows.ld[m] = V;
        rows.w[m] = member_w[m];
    }
    const int t1 = t0 + n_steps < T ? t0 + n_steps : T;
    for (int t = t0; t < t1; ++t) {
        int* token_t = b.s.token + (long)t * R;
        int* parent_t = b.s.parent + (long)t * R;
        for (int m = 0; m < M; ++m) {
            const StepWs& s = b.m[m];
            SCN_TRY(decode_step(st, d[m], K, w + m, enc, s, att_live, s.alpha ? s.alpha + (long)t * R * P : nullptr, s.hA, s.cA,
                                s.hB, s.cB));
        }
        BeamExcl x{};
        if (o || cn) x = step_excl(o, t, T, R, end_token, b.hist);
        SCN_TRY(beam_row_topk_ens(st, N, K, V, M, rows, mode, b.s.scores, b.s.nsrc, (o || cn) ? &x : nullptr, b.candv, b.candi, 0,
                                  Kg, cn ? &bc : nullptr));
        if (cn)
            SCN_TRY(beam_merge_banks(st, N, K, V, end_token, t, b.candv, b.candi, b.reqv, b.reqi, b.req, b.s));
        else if (v)
            SCN_TRY(beam_merge_groups(st, N, K, Kg, v->penalty, V, end_token, t, b.candv, b.candi, b.s));
        else
            SCN_TRY(beam_merge(st, N, K, V, end_token, t, b.candv, b.candi, b.s));
        for (int m = 0; m < M; ++m) {
            const StepWs& s = b.m[m];
            if (o && m == 0)
                SCN_TRY(beam_advance_opt(st, N, K, d[m].D, d[m].M, V, t, T, s.hB, s.cB, parent_t, token_t,
                                         w[m].embedding_weight, x.hist, b.hist + (long)((t + 1) & 1) * R * T, s.hA, s.cA,
                                         s.emb));
            else
                SCN_TRY(beam_advance(st, N, K, d[m].D, d[m].M, V, s.hB, s.cB, parent_t, token_t, w[m].embedding_weight, s.hA,
                                     s.cA, s.emb));
        }
    }
    return 0;
}

// ---- sampled rollouts (csrc/rollout.hip): the same set-up and decode step, K INDEPENDENT slots per image ------------------
// After fc, rollout_pick replaces beam_row_topk + beam_merge and rollout_advance replaces beam_advance: the state carries
// over slot for slot, so h / c are not gathered but alternate between the A and B buffers with the parity of the step, and
// the advance only gathers the next embedding and refreshes nsrc.  One launch fewer per step than the search (11-12 with
// attention, 8-9 without).  fp32 only.
namespace {

// filtered: the _f form of the four calls, whose workspace also holds the nkeep records (behind alpha, zero-filled by init)
// scored: the _sc form, which keeps rank, best and the given tokens there instead; mixed: the _ss form, with sample,
// replaced and the gold words
size_t carve_rollout(const scnattn_dims& d, int K, int T, int want_alpha, bool filtered, float* base, RolloutWs& b,
                     bool scored = false, bool mixed = false) {
    Carver c(base);
    const int N = d.B, P = d.P;
    const long R = (long)N * K;
    b.s.R = (int)R;
    b.s.T = T;
    b.s.open_rows = ints(c.take(1));
    b.s.nsrc = ints(c.take(N));
    b.s.nopen = ints(c.take(N));
    b.s.length = ints(c.take(R));
    b.s.sum_logp = c.take(R);
    b.s.token = ints(c.take(sz(T, R)));
    b.s.logp = c.take(sz(T, R));
    b.alpha = (d.has_att && want_alpha) ? c.take(sz(T, R, P)) : nullptr;
    b.nkeep = filtered ? ints(c.take(sz(T, R))) : nullptr;
    b.rank = scored ? ints(c.take(sz(T, R))) : nullptr;
    b.best = scored ? ints(c.take(sz(T, R))) : nullptr;
    b.target = scored ? ints(c.take(sz(T, R))) : nullptr;
    b.sample = mixed ? ints(c.take(sz(T, R))) : nullptr;
    b.replaced = mixed ? ints(c.take(sz(T, R))) : nullptr;
    b.gold = mixed ? ints(c.take(sz(T, R))) : nullptr;
    carve_step_state(c, d, R, b);
    b.state_floats = c.off;
    carve_step_setup(c, d, R, b);
    return c.off * sizeof(float);
}

// f: the filter of the _f form (null: the plain form), refused when out of range
int check_filter(const scnattn_sample_filter* f, bool given) {
    if (!given) return 0;
    SCN_ARG(f, "rollout: the sample filter is NULL");
    SCN_ARG(rollout_filter_ok(f->top_k, f->top_p), "rollout: the sample filter needs top_k >= 0 and 0 < top_p <= 1");
    return 0;
}

}  // namespace

int rollout_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                      bool filtered, size_t* bytes) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_TRY(check_filter(f, filtered));
    SCN_ARG(bytes, "rollout_workspace: bytes is NULL");
    RolloutWs b;
    *bytes = carve_rollout(*d, K, max_steps, want_alpha, filtered, nullptr, b);
    return 0;
}

// off[SCNATTN_ROLLOUT_NOFF]: where the results live in the workspace, in 4-byte elements (order: include/scnattn.h); the _f
// form off[SCNATTN_ROLLOUT_NOFF_F], the nkeep records' offset behind them
int rollout_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f, bool filtered,
                   long* off) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_TRY(check_filter(f, filtered));
    SCN_ARG(off, "rollout_layout: offsets is NULL");
    RolloutWs b;
    carve_rollout(*d, K, max_steps, want_alpha, filtered, layout_base(), b);
    const void* p[SCNATTN_ROLLOUT_NOFF_F] = {b.s.open_rows, b.s.nsrc, b.s.nopen, b.s.length, b.s.sum_logp, b.s.token, b.s.logp,
                                             b.alpha, b.nkeep};
    offsets_from(layout_base(), p, filtered ? SCNATTN_ROLLOUT_NOFF_F : SCNATTN_ROLLOUT_NOFF, off);
    return 0;
}

int rollout_init(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                 bool filtered, const scnattn_params* w, const float* enc, const float* tags, int start_token, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    SCN_TRY(check_filter(f, filtered));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && tags && ws, "rollout_init: null argument");
    SCN_ARG(start_token >= 0 && start_token < d.V, "rollout_init: start token outside the vocabulary");
    SCN_ARG(aligned16(ws), "rollout_init: the workspace must be 16-byte aligned");
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, filtered, ws, b);
    SCN_HIP(hipMemsetAsync(ws, 0, b.state_floats * sizeof(float), st));      // the records of closed rows: <pad> / 0.0
    SCN_TRY(rollout_state_init(st, d.B, K, b.s));
    SCN_TRY(decode_setup(st, d, K, w, enc, tags, start_token, b));
    return 0;
}

// Steps t0 .. t0 + n_steps - 1 (0-based; clipped to max_steps).  A finished image's kernels are no-ops.  The _f form swaps
// the pick for the filtered one: the same launches per step.
int rollout_steps(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_sample_filter* f,
                  bool filtered, const scnattn_params* w, const float* enc, int end_token, float inv_temp,
                  unsigned long long seed, unsigned draw, int greedy_first, int t0, int n_steps, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    SCN_TRY(check_filter(f, filtered));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && ws, "rollout_steps: null argument");
    SCN_ARG(t0 >= 0 && n_steps >= 0, "rollout_steps: negative step");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_steps: inv_temp must be positive and finite");
    SCN_ARG(end_token >= 0 && end_token < d.V, "rollout_steps: end token outside the vocabulary");
    const int N = d.B, P = d.P, M = d.M, V = d.V, R = N * K;
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, filtered, ws, b);
    const int t1 = t0 + n_steps < max_steps ? t0 + n_steps : max_steps;
    for (int t = t0; t < t1; ++t) {
        const bool even = (t & 1) == 0;         // the state of step t sits in A for even t, in B for odd t
        SCN_TRY(decode_step(st, d, K, w, enc, b, b.s.nsrc, b.alpha ? b.alpha + (long)t * R * P : nullptr, even ? b.hA : b.hB,
                            even ? b.cA : b.cB, even ? b.hB : b.hA, even ? b.cB : b.cA));
        if (filtered)
            SCN_TRY(rollout_pick_filtered(st, N, K, V, b.logits, V, inv_temp, seed, draw, t, greedy_first, end_token, f->top_k,
                                          f->top_p, b.nkeep + (long)t * R, 0, b.s));
        else
            SCN_TRY(rollout_pick(st, N, K, V, b.logits, V, inv_temp, seed, draw, t, greedy_first, end_token, b.s));
        SCN_TRY(rollout_advance(st, N, K, M, V, b.s.token + (long)t * R, w->embedding_weight, b.emb, b.s.nopen, b.s.nsrc));
    }
    return 0;
}

// ---- scoring given captions (the _sc form; include/scnattn.h) --------------------------------------------------------------
// The rollout's chain with the pick replaced by rollout_score, which is told the token: the same launches per step.  The
// workspace is the plain rollout's with three more records behind alpha; `length` holds ntok.
int score_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(bytes, "rollout_workspace_sc: bytes is NULL");
    RolloutWs b;
    *bytes = carve_rollout(*d, K, max_steps, want_alpha, false, nullptr, b, true);
    return 0;
}

// off[SCNATTN_ROLLOUT_NOFF_SC]: the 8 of rollout_layout, then rank, best, target
int score_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* off) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(off, "rollout_layout_sc: offsets is NULL");
    RolloutWs b;
    carve_rollout(*d, K, max_steps, want_alpha, false, layout_base(), b, true);
    const void* p[SCNATTN_ROLLOUT_NOFF_SC] = {b.s.open_rows, b.s.nsrc, b.s.nopen, b.s.length, b.s.sum_logp, b.s.token, b.s.logp,
                                              b.alpha, b.rank, b.best, b.target};
    offsets_from(layout_base(), p, SCNATTN_ROLLOUT_NOFF_SC, off);
    return 0;
}

int score_init(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_params* w,
               const float* enc, const float* tags, int start_token, const int* targets, long ld_tok, const int* ntok,
               float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && tags && ws, "rollout_init_sc: null argument");
    SCN_ARG(targets && ntok, "rollout_init_sc: the captions are NULL");
    SCN_ARG(ld_tok >= max_steps, "rollout_init_sc: ld_tok must be at least max_steps");
    SCN_ARG(start_token >= 0 && start_token < d.V, "rollout_init_sc: start token outside the vocabulary");
    SCN_ARG(aligned16(ws), "rollout_init_sc: the workspace must be 16-byte aligned");
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, false, ws, b, true);
    SCN_HIP(hipMemsetAsync(ws, 0, b.state_floats * sizeof(float), st));      // the records of closed rows: zeros
    SCN_TRY(rollout_score_init(st, d.B, K, targets, ld_tok, ntok, b.target, b.s));
    SCN_TRY(decode_setup(st, d, K, w, enc, tags, start_token, b));
    return 0;
}

int score_steps(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_params* w,
                const float* enc, float inv_temp, int t0, int n_steps, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && ws, "rollout_steps_sc: null argument");
    SCN_ARG(t0 >= 0 && n_steps >= 0, "rollout_steps_sc: negative step");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_steps_sc: inv_temp must be positive and finite");
    const int N = d.B, P = d.P, M = d.M, V = d.V, R = N * K;
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, false, ws, b, true);
    const int t1 = t0 + n_steps < max_steps ? t0 + n_steps : max_steps;
    for (int t = t0; t < t1; ++t) {
        const bool even = (t & 1) == 0;         // the state of step t sits in A for even t, in B for odd t
        const long o = (long)t * R;
        SCN_TRY(decode_step(st, d, K, w, enc, b, b.s.nsrc, b.alpha ? b.alpha + o * P : nullptr, even ? b.hA : b.hB,
                            even ? b.cA : b.cB, even ? b.hB : b.hA, even ? b.cB : b.cA));
        SCN_TRY(rollout_score(st, N, K, V, b.logits, V, inv_temp, t, b.target + o, b.rank + o, b.best + o, b.s));
        SCN_TRY(rollout_advance(st, N, K, M, V, b.s.token + o, w->embedding_weight, b.emb, b.s.nopen, b.s.nsrc));
    }
    return 0;
}

// ---- scheduled sampling (the _ss form; include/scnattn.h) -------------------------------------------------------------------
// The scoring chain with the pick replaced by rollout_pick_mixed, which is told the gold word and flips a coin: the same
// launches per step.  The workspace is the plain rollout's with three more records behind alpha; `length` holds nmix.
int mix_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(bytes, "rollout_workspace_ss: bytes is NULL");
    RolloutWs b;
    *bytes = carve_rollout(*d, K, max_steps, want_alpha, false, nullptr, b, false, true);
    return 0;
}

// off[SCNATTN_ROLLOUT_NOFF_SS]: the 8 of rollout_layout, then sample, replaced, gold
int mix_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* off) {
    SCN_TRY(check_beam(d, K, max_steps));
    SCN_ARG(off, "rollout_layout_ss: offsets is NULL");
    RolloutWs b;
    carve_rollout(*d, K, max_steps, want_alpha, false, layout_base(), b, false, true);
    const void* p[SCNATTN_ROLLOUT_NOFF_SS] = {b.s.open_rows, b.s.nsrc, b.s.nopen, b.s.length, b.s.sum_logp, b.s.token, b.s.logp,
                                              b.alpha, b.sample, b.replaced, b.gold};
    offsets_from(layout_base(), p, SCNATTN_ROLLOUT_NOFF_SS, off);
    return 0;
}

int mix_init(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_params* w,
             const float* enc, const float* tags, int start_token, const int* gold, long ld_tok, const int* nmix, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && tags && ws, "rollout_init_ss: null argument");
    SCN_ARG(gold && nmix, "rollout_init_ss: the captions are NULL");
    SCN_ARG(ld_tok >= max_steps, "rollout_init_ss: ld_tok must be at least max_steps");
    SCN_ARG(start_token >= 0 && start_token < d.V, "rollout_init_ss: start token outside the vocabulary");
    SCN_ARG(aligned16(ws), "rollout_init_ss: the workspace must be 16-byte aligned");
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, false, ws, b, false, true);
    SCN_HIP(hipMemsetAsync(ws, 0, b.state_floats * sizeof(float), st));      // the records of rows no kernel visits: zeros
    SCN_TRY(rollout_score_init(st, d.B, K, gold, ld_tok, nmix, b.gold, b.s));
    SCN_TRY(decode_setup(st, d, K, w, enc, tags, start_token, b));
    return 0;
}

int mix_steps(hipStream_t st, const scnattn_dims* dp, int K, int max_steps, int want_alpha, const scnattn_params* w,
              const float* enc, float inv_temp, float prob, unsigned long long seed, unsigned draw, int greedy, int t0,
              int n_steps, float* ws) {
    SCN_TRY(check_beam(dp, K, max_steps));
    const scnattn_dims& d = *dp;
    SCN_ARG(w && enc && ws, "rollout_steps_ss: null argument");
    SCN_ARG(t0 >= 0 && n_steps >= 0, "rollout_steps_ss: negative step");
    SCN_ARG(inv_temp > 0.f && inv_temp < INFINITY, "rollout_steps_ss: inv_temp must be positive and finite");
    SCN_ARG(rollout_prob_ok(prob), "rollout_steps_ss: prob must be in [0, 1]");
    const int N = d.B, P = d.P, M = d.M, V = d.V, R = N * K;
    RolloutWs b;
    carve_rollout(d, K, max_steps, want_alpha, false, ws, b, false, true);
    const int t1 = t0 + n_steps < max_steps ? t0 + n_steps : max_steps;
    for (int t = t0; t < t1; ++t) {
        const bool even = (t & 1) == 0;         // the state of step t sits in A for even t, in B for odd t
        const long o = (long)t * R;
        SCN_TRY(decode_step(st, d, K, w, enc, b, b.s.nsrc, b.alpha ? b.alpha + o * P : nullptr, even ? b.hA : b.hB,
                            even ? b.cA : b.cB, even ? b.hB : b.hA, even ? b.cB : b.cA));
        SCN_TRY(rollout_pick_mixed(st, N, K, V, b.logits, V, inv_temp, prob, seed, draw, t, greedy, b.gold + o, b.sample + o,
                                   b.replaced + o, b.s));
        SCN_TRY(rollout_advance(st, N, K, M, V, b.s.token + o, w->embedding_weight, b.emb, b.s.nopen, b.s.nsrc));
    }
    return 0;
}

}  // namespace scn
