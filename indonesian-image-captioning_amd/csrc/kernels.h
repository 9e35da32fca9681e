// Internal launcher API of libscnattn: one function per kernel, all asynchronous on `st`,
// all returning 0 or an error code (message via scn::last_error()).  The extern "C" surface in
// api.cpp and the sequence drivers in sequence.cpp are thin layers over these.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/scnattn.h"

#define SCN_MAX_KSPLIT 16

namespace scn {

// ---- launch plans (include/scnattn.h, scnattn_plan_next) --------------------------------------------------------------
// Every dense-product launcher below is  argument checks -> a pure plan function -> a launch that reads only the plan.
typedef ::scnattn_launch_plan LaunchPlan;
extern thread_local LaunchPlan* t_plan_out;     // armed by scnattn_plan_next, null otherwise
// First statement of such a launcher: takes the armed request off the thread and clears *out (family 0), so no return path
// -- empty problem, refusal, answer -- leaves the thread armed.  One thread-local read when nothing is armed.
struct PlanQuery {
    LaunchPlan* out;
    PlanQuery() : out(t_plan_out) { if (out) { t_plan_out = nullptr; *out = LaunchPlan{}; } }
    bool answer(const LaunchPlan& p) const { if (out) *out = p; return out != nullptr; }     // true: launch nothing
    void hand_on() const { t_plan_out = out; }      // a launcher that forwards to another one (sgemm_ws -> cgemm)
};

// ---- sgemm.hip -------------------------------------------------------------------------------
int sgemm(hipStream_t st, bool tA, bool tB, int M, int N, int K, float alpha, const float* A, long lda,
          const float* B, long ldb, float beta, float* C, long ldc, const float* bias,
          const float* rowmask, int batch, long sA, long sB, long sC);

// same, with a workspace: low-parallelism shapes (few output tiles, deep K) are split along K into
// partial slabs in `ws` and reduced in slab order by a second launch (deterministic)
int sgemm_ws(hipStream_t st, bool tA, bool tB, int M, int N, int K, float alpha, const float* A, long lda,
             const float* B, long ldb, float beta, float* C, long ldc, const float* bias, const float* rowmask,
             int batch, long sA, long sB, long sC, float* ws, long ws_floats);

// ---- cgemm.hip: LDS-DMA pipelined fp32 GEMM with the 1x1-convolution prologues / epilogues -------------------
struct ConvExtra {
    int pro = 0;              // 1: A = relu(A*scale[k]+shift[k]) (k-contiguous A); 2: B = relu(B*scale[n]+shift[n]) ([K][N] B)
    int epi = 0;              // 1: column sums of (y-s), (y-s)^2 per 64 rows; 2: relu mask from z + sums of g, g*xhat
    const float* pro_ss = nullptr;    // interleaved {scale, shift} per channel
    float* stat_partial = nullptr;    // [2][N][cgemm_stat_ld(M)], channel-major
    const float* stat_shift = nullptr;
    const float* ez = nullptr; const float* emean = nullptr; const float* einvstd = nullptr;
    const float* egamma = nullptr; const float* ebeta = nullptr; long ldz = 0;
    int stride = 1, Hi = 0, Wi = 0, Ho = 0, Wo = 0;   // stride > 1: rows of the activation operand are gathered
    int force_split = 0;      // tests / tuning: > 0 forces the split-K factor
    int force_mi = 0;         // tests / tuning: 1 / 2 forces the 64- / 128-row tile
    int c3 = 0;               // 3x3 convolution as an implicit GEMM: 1 forward, 2 dgrad (stride 1), 3 wgrad, 4 dgrad (stride 2)
    int c3c = 0;              // channels per tap of the gathered operand
    long c3_src_rows = 0;     // rows of the gathered map
    // epi 3 (eval BatchNorm): y = act(acc * scale[n] + shift[n] (+ ez[m][n])), scale = egamma / sqrt(evar + eeps),
    // shift = ebeta - emean * scale; ez / ldz is the optional residual, erelu selects the ReLU
    const float* evar = nullptr; float eeps = 0.f; int erelu = 0;
};
bool cgemm_supported(bool tA, bool tB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                     long sA, long sB);
int cgemm(hipStream_t st, bool tA, bool tB, int M, int N, int K, float alpha, const float* A, long lda, const float* B,
          long ldb, float beta, float* C, long ldc, const float* bias, const float* rowmask, int batch, long sA, long sB,
          long sC, float* ws, long ws_floats, const ConvExtra* ex);
int cgemm_row_tiles(int M);
int cgemm_stat_ld(int M);      // leading dimension of the channel-major statistics partial [2][N][ld] a product of M rows writes
int cgemm_reduce(hipStream_t st, const float* ws, int S, int M, int N, float* C, long ldc);

// ---- conv3.hip: 3x3 weight gradient (stride 1) with the activation halo staged once per strip ---------------------
bool conv3x3_wgrad_halo_ok(int N, int H, int W, int C, int Co, const float* dy, const float* x, const float* dw);
int conv3x3_wgrad_halo(hipStream_t st, int N, int H, int W, int C, int Co, const float* dy, const float* x, float* dw,
                       float* ws, long ws_floats, int force_split);

// ---- stem.hip: conv 7x7 / 2 (+ statistics) and BatchNorm + ReLU + MaxPool 3x3 / 2 of the trunk's stem -----------------
int stem_tiles(int N, int H, int W);
int stem_conv7(hipStream_t st, int N, int H, int W, const float* x, long sn, long sc, long sh, long sw, const float* w,
               long wn, long wc, long wh, long ww, float* z, float* partial, const float* stat_shift);
int stem_bn_relu_maxpool(hipStream_t st, int N, int Hz, int Wz, int C, const float* z, const float* ss, void* out, int out_bf16);

// ---- skinny.hip ------------------------------------------------------------------------------
int skinny_pick_ksplit(int rows, int N, int K, int groups);
// A split-K result: `n` slabs `stride` elements apart, row leading dimension `ld`.
struct Slabs {
    const float* p; int n; long stride; long ld;
};
// wbf 1: W holds bf16 (raw 16-bit) elements, ldw / wg still count elements; 2: X is rounded to bf16 in registers too and
// the products run on the bf16 matrix instruction (fp32 accumulation)
int skinny_gemm(hipStream_t st, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                const void* W, long ldw, long wg, float* Y, long ldy, long yg, long yslab, int ksplit, int wbf = 0);

// ---- attention.hip ---------------------------------------------------------------------------
// e[b,p] = w . relu(att1[b,p,:] + att2[b,:]) + b0, att2 = sum(slabs) + bd   (attention.py:37-39)
// bf (here and below): the streamed operand (att1 / enc / x) holds bf16 elements
int attn_scores(hipStream_t st, int rows, int P, int A, const void* att1, Slabs att2, const float* bd,
                const float* w, const float* b0, float* e, float* att2_out, bool bf = false);
// alpha = softmax_p(e); awe = sum_p alpha*enc; z = sigmoid(gpre + bbeta) * awe   (attention.py:40-42,
// attention_scn.py:147-148).  gpre.p == nullptr -> no gate (z = awe, gate not written).
int attn_context(hipStream_t st, int rows, int P, int E, const void* enc, const float* e, Slabs gpre,
                 const float* bbeta, float* alpha_out, long alpha_ld, float* alpha_save, float* awe,
                 float* gate, float* z, bool bf = false);
int mean_pixels(hipStream_t st, int rows, int P, int E, const float* enc, float* out);
// Pooled path (include/scnattn.h, scnattn_pool): encoder_out = fixed linear pooling of x [B][Q][E]
struct PoolDesc {
    int Q, qtap_max;
    const int* tap_idx;     // [P][4]
    const float* tap_w;     // [P][4]
    const int* qtap_idx;    // [Q][qtap_max], -1 = unused
    const float* qtap_w;    // [Q][qtap_max]
    const float* col_w;     // [Q]: column sums of the pooling matrix / P (pixel mean of the pooled map)
};
// What every taker of a scnattn_pool checks before it reads one (api.cpp): Q > 0, 0 < qtap_max <= 64, no null table.
// The sequence drivers add what only they need (Q <= P, A % 4, E % 4: csrc/sequence.cpp check_pool).
int pool_desc(const ::scnattn_pool* p, PoolDesc& out);
int attn_context_pooled(hipStream_t st, int rows, int P, int E, const void* x, const PoolDesc& pool, const float* e,
                        Slabs gpre, const float* bbeta, float* alpha_out, long alpha_ld, float* alpha_save,
                        float* alphaq_save, float* awe, float* gate, float* z, bool bf = false);
int weighted_rows(hipStream_t st, int rows, int Q, int E, const float* x, const float* wts, float* out);
int attn_softmax_bwd_pooled(hipStream_t st, int rows, int P, int A, const void* att1, const float* att2, const float* w,
                            const float* alpha, const PoolDesc& pool, const float* dalphaq, const float* dalpha_in,
                            long dalpha_in_ld, float* de, float* datt2, long datt2_ld, bool bf = false);
int pool_expand(hipStream_t st, int B, int P, int A, const PoolDesc& pool, const float* y, const float* bias, float* out);
int pool_transpose(hipStream_t st, int B, int P, int A, const PoolDesc& pool, const float* in, float* out);
int add_bcast_rows_w(hipStream_t st, int B, int Q, int E, const float* wts, const float* v, float* out);
// dalpha[b,p] = enc[b,p,:] . dawe[b,:] + dalpha_in[b,p]
int attn_dalpha(hipStream_t st, int rows, int P, int E, const void* enc, const float* dawe,
                const float* dalpha_in, long dalpha_in_ld, float* dalpha, bool bf = false);
// de = alpha*(dalpha - sum(alpha*dalpha));  datt2[b,a] = w[a] * sum_p de[b,p]*[att1+att2 > 0]
int attn_softmax_bwd(hipStream_t st, int rows, int P, int A, const void* att1, const float* att2,
                     const float* w, const float* alpha, const float* dalpha, float* de, float* datt2,
                     long datt2_ld, bool bf = false);
// After the time loop: datt1[b,p,a] = w[a]*sum_t de_t[b,p]*[att1+att2_t>0]; per-block partials of
// dw[a] = sum de_t*relu(att1+att2_t) and db0 = sum de_t in dwpart[block][A+1].
int attn_datt1_post(hipStream_t st, int B, int P, int A, int T, const int* dl, const void* att1,
                    const float* att2_all, const float* de_all, const float* w, float* datt1,
                    float* dwpart, int* nblocks_out, bool bf = false);
int attn_datt1_post_blocks(int B, int P);

// ---- beam.hip: batched beam search, K slots per image, rows n*K + j (the semantics are at the top of that file) ------
#define SCN_MAX_BEAM 8
// The search state of N images (R = N*K rows); every array lives in the caller's workspace.
struct BeamState {
    int R;
    float* scores;          // [R]    running score of each open slot
    int* nsrc;              // [N]    live source beams
    int* kk;                // [N]    beams still to fill (0: finished)
    int* ncomp;             // [N]    completed beams so far (<= K)
    int* best_idx;          // [N]    index of the best completed beam in comp_* (-1: none), replaced on strictly greater
    float* best_score;      // [N]
    int* open_images;       // [1]    images with kk > 0
    float* comp_score;      // [R]    completed beams of image n in completion order at n*K ..
    int* comp_step;         // [R]    step (0-based) at which <end> was picked
    int* comp_parent;       // [R]    source slot that picked it
    int* token;             // [steps][R]  word of the beam that sits in this slot AFTER the step
    int* parent;            // [steps][R]  slot it came from
    // The grouped search (beam_merge_groups): nsrc .. best_score are then [N*G], one entry per (image,
    // group), and att_live [N] is what the attention kernels take for nsrc: K while any group of the image is open, else 0.
    int* att_live = nullptr;
    // The constrained search (beam_merge_banks): met [R], per slot the bitmask of the image's required words
    // that occur in the slot's history.
    int* met = nullptr;
};
// e[n*K+j][p] for j < nsrc[n]; att2 = sum(slabs) + bd over rows n*K+j; rows of dead slots are left untouched
int beam_attn_scores(hipStream_t st, int N, int K, int P, int A, const float* att1, Slabs att2, const float* bd,
                     const float* w, const float* b0, const int* nsrc, float* e);
// alpha_out [N*K][P] (may be NULL), awe [N*K][E] (may be NULL), z = sigmoid(gpre + bbeta) * awe (gpre.p == nullptr: z = awe)
int beam_attn_context(hipStream_t st, int N, int K, int P, int E, const float* enc, const float* e, Slabs gpre,
                      const float* bbeta, const int* nsrc, float* alpha_out, float* awe, float* z);
// The M logits rows the selection reads per live row r: p[m] + r * ld[m], weights w[m] > 0 that sum to 1.
#define SCN_MAX_ENSEMBLE 4
struct EnsRows {
    const float* p[SCN_MAX_ENSEMBLE];
    long ld[SCN_MAX_ENSEMBLE];
    float w[SCN_MAX_ENSEMBLE];
};
// ---- the search OPTIONS: candidates a step may not pick -------------------------------------------------
#define SCN_MAX_BANNED 64
#define SCN_MAX_NGRAM 8
// What the selection of step t excludes, per live row: the banned words, `end_excl` (<end> while t < min_length; -1: none)
// and, for g >= 1, every word that would close an n-gram of g words the row's history hist[row*T .. +t-1] already holds.
struct BeamExcl {
    int t, T, g, end_excl, n_banned;
    const int* hist;        // [N*K][T] (may be null when g == 0)
    int banned[SCN_MAX_BANNED];
};
// ---- the CONSTRAINTS: words a caption must contain ------------------------------------------------------
#define SCN_MAX_REQUIRED 4
// What the selection of a constrained search takes beside the exclusions: per live row the image's unmet required words
// leave the K rounds, as does <end> = end_tok while a requirement is open, and the row's 4 REQUIRED candidates go to
// reqv / reqi [N*K][4]: entry c is (scores[row] + c_v(req[n][c]), req[n][c]) when the word exists, is unmet in the row and is
// not excluded by the options, else (-inf, -1).  Everything on the device.
struct BeamCon {
    const int* req;         // [N][4] the required words of image n, padded with -1
    const int* met;         // [N*K]  bit c: the slot's history holds req[n][c]
    int end_tok;
    float* reqv;            // [N*K][4]
    int* reqi;              // [N*K][4]
};
struct BeamExclCon : BeamExcl {
    BeamCon c;
};
// THE selection (one kernel template, one launcher).  outv / outi [N*K][K]: per live row the top K of scores[row] + c_v,
// best first, with l_mv = logits_m[row][v] - lse_m(row) and
// mode 0: c_v = sum_m w_m l_mv;  mode 1: c_v = a_v + log(sum_m w_m exp(l_mv - a_v)), a_v = max_m l_mv.
// x: the candidates left out of the K rounds (the log-sum-exp still runs over all V logits); null: none, which writes the
// bits of an `x` that excludes nothing.  With x it refuses unless V - n_banned - 1 - (g >= 1 ? T : 0) >= K.
// force_passes != 0 (tests): read the rows from global memory in every pass even when a row fits the LDS.
// Kg: the slots per group of a grouped search (K % Kg == 0; nsrc is then [N * K/Kg] and row n*K + g*Kg + s is live when
// s < nsrc[n * K/Kg + g]); Kg = K (or 0, the default) is the search without groups.  A live row runs K rounds either way.
// cn: the constraints of a constrained search (needs x, which may exclude nothing, and no groups); null: none.  With cn the
// candidate-count refusal asks for SCN_MAX_REQUIRED more words.
int beam_row_topk_ens(hipStream_t st, int N, int K, int V, int M, const EnsRows& e, int mode, const float* scores,
                      const int* nsrc, const BeamExcl* x, float* outv, int* outi, int force_passes, int Kg = 0,
                      const BeamCon* cn = nullptr);
// The single decoder's selection, the top K of scores[row] + logits[row][v] - lse(row): beam_row_topk_ens with M = 1,
// mode 0, w = 1, nothing excluded.
int beam_row_topk(hipStream_t st, int N, int K, int V, const float* logits, long ld, const float* scores, const int* nsrc,
                  float* outv, int* outi, int force_passes);
int beam_merge(hipStream_t st, int N, int K, int V, int end_tok, int t, const float* candv, const int* candi,
               const BeamState& s);
// The merge of a search in G = K / Kg groups of Kg slots (include/scnattn.h: "diverse beam search"): per image the groups in
// order, group g ranking its nsrc_g x K candidates by fmaf(-penalty, c, value), c = the picks of groups h < g at this step
// with the candidate's word; raw values are stored.  s.nsrc .. s.best_score are [N*G], s.att_live [N] may be null.
int beam_merge_groups(hipStream_t st, int N, int K, int Kg, float penalty, int V, int end_tok, int t, const float* candv,
                      const int* candi, const BeamState& s);
// The merge of a constrained search (include/scnattn.h: "CONSTRAINED beam search"): per image the nsrc x (K + 4) ordinary
// and required candidates of the selection fall into banks by the number of required words their beam would have met, the
// kk picks go round-robin over the banks C_n .. 0, and the picked set is recorded in the search order as beam_merge does,
// with the new s.met.  req [N][4] on the device.
int beam_merge_banks(hipStream_t st, int N, int K, int V, int end_tok, int t, const float* candv, const int* candi,
                     const float* reqv, const int* reqi, const int* req, const BeamState& s);
// One kernel behind both: h / c of row n*K+s gathered from its parent slot, emb from the table; the _opt form also writes
// the row's history for step t+1, the parent slot's first t entries of hist_s, then token_t[row] (hist_s != hist_d)
int beam_advance(hipStream_t st, int N, int K, int D, int M, int V, const float* hs, const float* cs, const int* parent_t,
                 const int* token_t, const float* table, float* hd, float* cd, float* emb);
int beam_advance_opt(hipStream_t st, int N, int K, int D, int M, int V, int t, int T, const float* hs, const float* cs,
                     const int* parent_t, const int* token_t, const float* table, const int* hist_s, int* hist_d, float* hd,
                     float* cd, float* emb);
int beam_expand_rows(hipStream_t st, int N, int K, int W, const float* in, float* out);
// G groups per image (1: the search without groups): every group starts from one live source, its slot 0, with K / G to fill
int beam_state_init(hipStream_t st, int N, int K, const BeamState& s, int G = 1);

// ---- rollout.hip: sampled rollouts (K independent slots per image, rows n*K + j, nothing compacted) ------------------
struct RolloutState {
    int R, T;               // rows, steps the records hold
    int* open_rows;         // [1]    rows that have not produced <end> (the host polls it)
    int* nsrc;              // [N]    K while any slot of the image is open, 0 afterwards (what the attention kernels take)
    int* nopen;             // [N]    open slots of the image
    int* length;            // [R]    t + 1 of the step that produced <end>; 0: still open
    float* sum_logp;        // [R]    running sum of the logp records
    int* token;             // [T][R] token picked at step t (0 after the row closed)
    float* logp;            // [T][R] its log-probability under softmax(logits * inv_temp) (0.0 after the row closed)
};
// One token per live row: arg-max of logits * inv_temp + Gumbel noise (Philox4x32-10 keyed by seed, counter
// (v >> 2, row, t, draw)); slot 0 of every image takes the plain arg-max when greedy_first != 0.  Contract: rollout.hip.
int rollout_pick(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, unsigned long long seed,
                 unsigned draw, int t, int greedy_first, int end_tok, const RolloutState& s);
// The same pick inside the top-k / nucleus set of the row (include/scnattn.h: scnattn_sample_filter): the first
// nkeep = min(L_k, L_p) words of the order (y descending, index ascending), logp under the renormalised kept set, and the
// record nkeep_t[row] (0 for a closed row of an open image).  top_k 0 or >= V and top_p 1 mean off; both off launches
// rollout_pick's kernel and leaves nkeep_t alone (it may then be null).  force_passes != 0 (tests): re-read the row from
// global memory in every pass even when it fits the registers (V <= 10240).
bool rollout_filter_ok(int top_k, float top_p);
int rollout_pick_filtered(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp,
                          unsigned long long seed, unsigned draw, int t, int greedy_first, int end_tok, int top_k, float top_p,
                          int* nkeep_t, int force_passes, const RolloutState& s);
// emb[row] = table[clamp(token_t[row])]; nsrc[n] = nopen[n] > 0 ? K : 0
int rollout_advance(hipStream_t st, int N, int K, int M, int V, const int* token_t, const float* table, float* emb,
                    const int* nopen, int* nsrc);
int rollout_state_init(hipStream_t st, int N, int K, const RolloutState& s);
// SCORING given captions (include/scnattn.h: teacher-forced log-probabilities): the pick with the token told.  s.length
// holds ntok, the number of given tokens of the row; a row is open at step t iff t < ntok.  Per open row: token = the
// target, logp under softmax(logits * inv_temp) (fp32 terms, fp64 sum in tally order, one rounding), rank = words strictly
// before the target in the ORDER, best = the first word of the ORDER; the row closes at t + 1 == ntok.
int rollout_score(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, int t,
                  const int* target_t, int* rank_t, int* best_t, const RolloutState& s);
// The state of a scoring run from the captions: target_ws [T][R] = targets [R][ld_tok] transposed, s.length = ntok clamped
// into [0, T], nopen / nsrc / open_rows counted from it, sum_logp = 0.  One launch.
int rollout_score_init(hipStream_t st, int N, int K, const int* targets, long ld_tok, const int* ntok, int* target_ws,
                       const RolloutState& s);
// SCHEDULED SAMPLING (include/scnattn.h: the _ss form): the pick told the gold word, behind a coin.  s.length holds nmix; a
// row is open at step t iff t < nmix.  Per open row u = the uniform of word 0 of Philox with counter (0xFFFFFFFF, row, t,
// draw); u < prob: rollout_pick's pick (every row the arg-max when greedy != 0), token = sample = the pick, its logp,
// replaced = 1, sum_logp += logp; else token = gold, sample = -1, logp = 0.0, replaced = 0 and the logits are not read.  The
// row closes at t + 1 == nmix; <end> is not special.  The state of a run comes from rollout_score_init (gold for targets).
bool rollout_prob_ok(float prob);
int rollout_pick_mixed(hipStream_t st, int N, int K, int V, const float* logits, long ld, float inv_temp, float prob,
                       unsigned long long seed, unsigned draw, int t, int greedy, const int* gold_t, int* sample_t,
                       int* replaced_t, const RolloutState& s);

// ---- scn_cell.hip ----------------------------------------------------------------------------
int scn_mix_fwd(hipStream_t st, int rows, int F4, Slabs pz, const float* ex, Slabs ph, const float* qx,
                const float* qh, float* pa, float* phs, float* xcat);
int lstm_fwd(hipStream_t st, int rows, int H, Slabs r, long r_g, const float* bih, const float* bhh,
             const float* c_prev, float* gates, float* c_new, float* h_new, float* tanhc);
int lstm_bwd(hipStream_t st, int rows, int rows_next, int H, const float* dh_fc, Slabs dh_next,
             float* dc, const float* gates, const float* c_prev, const float* tanhc, float* dr);
int scn_mix_bwd(hipStream_t st, int rows, int F4, Slabs dxcat, long dxcat_g, const float* qx,
                const float* qh, const float* pa, const float* phs, float* dpx, float* dph, long dph_ld,
                float* dqx_acc, float* dqh_acc);
int gate_bwd(hipStream_t st, int rows, int E, Slabs dz, const float* awe, const float* gate,
             float* dawe, float* dgpre, long dgpre_ld);

// ---- misc.hip --------------------------------------------------------------------------------
int transpose2d(hipStream_t st, int R, int C, const float* in, long ldi, float* out, long ldo);
int copy2d(hipStream_t st, int R, int C, const float* in, long ldi, float* out, long ldo);
int colsum(hipStream_t st, int R, int N, const float* X, long ld, float* out, float beta);
int colsum_masked(hipStream_t st, int R, int N, const float* X, long ld, const float* rowmask, float* out, float beta);
int gather_rows_tm(hipStream_t st, int B, int T, int L, int M, const long long* caps, const float* table,
                   int V, float* out_tm);
int scatter_add_rows_tm(hipStream_t st, int B, int T, int L, int M, const long long* caps, const int* dl,
                        const float* demb_tm, int V, float* dtable, int* present);
int hidden_to_bm(hipStream_t st, int B, int T, int D, const int* dl, const float* hs_tm,
                 const float* mask_bm, float* out_bm, float* rowmask);
int hidden_from_bm(hipStream_t st, int B, int T, int D, const int* dl, const float* dbm,
                   const float* mask_bm, float* out_tm);
int add_bcast_rows(hipStream_t st, int B, int P, int E, const float* v, float scale, float* x);
// loss.hip: packed cross-entropy + doubly-stochastic attention term of the train step, in place
int caption_loss_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                     const int* dl, long n_tokens, const float* alphas, float alpha_c, float* row_lse, float* row_loss,
                     float* sm1, float* reg_part, float* loss);
// the same launches with the metrics in the row pass: the target's rank per row, the arg-max token, top-k / top-1 counts
int caption_loss_metrics_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                             long ldt, const int* dl, long n_tokens, const float* alphas, float alpha_c, float* row_lse,
                             float* row_loss, float* sm1, float* reg_part, float* loss, int k, int* row_rank, int* preds,
                             long ldp, int* hits);
int caption_loss_bwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets, long ldt,
                     const int* dl, long n_tokens, const float* row_lse, const float* sm1, float alpha_c,
                     const float* gout, float* dscores, float* dalphas);
// the reward-weighted pair (self-critical training): row_loss[b,t] and d scores[b,t,:] times row_weight[b], ONE product per
// row, so weights of 1.0 give the bits of the pair above; the attention regulariser is not weighted
int caption_loss_weighted_fwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                              long ldt, const int* dl, long n_tokens, const float* row_weight, const float* alphas,
                              float alpha_c, float* row_lse, float* row_loss, float* sm1, float* reg_part, float* loss);
int caption_loss_weighted_bwd(hipStream_t st, int B, int T, int V, int P, const float* scores, const long long* targets,
                              long ldt, const int* dl, long n_tokens, const float* row_weight, const float* row_lse,
                              const float* sm1, float alpha_c, const float* gout, float* dscores, float* dalphas);
// taghead.hip: the tagger's head around its Linear layer.  The map is x[b, q, c] (q over HW pixels) by element strides,
// fp32 or bf16; pooled = sum_q x / HW * ks (ks: pre-scaled dropout keep mask [B][ldk], may be null); bce_*: sigmoid +
// BCELoss (mean) + binary accuracy of the reference, rows: workspace [2][B], out: {loss, agreement count}
int tag_pool_fwd(hipStream_t st, int B, int HW, int C, const void* x, int bf16, long sb, long sp, long sc, const float* ks,
                 long ldk, float* out, long ldo);
int tag_pool_bwd(hipStream_t st, int B, int HW, int C, const float* dpooled, long ldd, const float* ks, long ldk, void* dx,
                 int bf16, long sb, long sp, long sc);
int bce_fwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, float* probs, long ldp,
            float* rows, float* out);
int bce_bwd(hipStream_t st, int B, int S, const float* probs, long ldp, const float* t, long ldt, const float* g, float* dz,
            long lddz);
// the weighted / focal / asymmetric family on the logits (include/scnattn.h: "Tagger losses for rare tags"), w: [S] or null
int tagloss_fwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, const float* w,
                const scnattn_tag_loss_options* opt, float* probs, long ldp, float* rows, float* out);
int tagloss_bwd(hipStream_t st, int B, int S, const float* z, long ldz, const float* t, long ldt, const float* w,
                const scnattn_tag_loss_options* opt, const float* g, float* dz, long lddz);
// data.hip: uint8 image rows (gathered by index) -> normalised fp32/bf16 batch, NCHW or channels-last
int u8_gather_normalize(hipStream_t st, const uint8_t* src, long n_src, const long long* idx, long n_out, int C,
                        long HW, const float* lut, void* dst, int dst_bf16, int channels_last);
// augment.hip: the same gather with a random resized crop, flip and colour jitter per sample (record of 8 floats from
// augment_draw or from the caller), the per-image mean grey its contrast step reads; semantics in include/scnattn.h
int u8_mean_grey(hipStream_t st, const uint8_t* src, long N, long HW, long long* sums, float* grey);
int augment_draw(hipStream_t st, long n, const long long* sid, int epoch, unsigned long long seed,
                 const scnattn_augment_config* cfg, int H, int W, float* params);
int u8_gather_augment(hipStream_t st, const uint8_t* src, long n_src, const long long* idx, long n_out, int H, int W,
                      const float* params, const float* grey, const float* mean, const float* std, void* dst, int dst_bf16,
                      int channels_last);
// resize.hip: a packed batch of decoded uint8 images -> Pillow's bilinear resize, as uint8 rows or normalised
int u8_resize_bilinear(hipStream_t st, const uint8_t* src, long src_bytes, const struct scnattn_image_desc* desc_host,
                       const struct scnattn_image_desc* desc_dev, int N, const int* taps, long taps_len, int OH, int OW,
                       const float* lut, void* dst, int dst_kind, int channels_last);
long resize_table_ints(int in, int out);
// the same kernel on tables that carry their row length in a header word (any filter; Pillow's LANCZOS), every row of
// the host copy of the tables checked before the launch
int u8_resize_taps(hipStream_t st, const uint8_t* src, long src_bytes, const struct scnattn_image_desc* desc_host,
                   const struct scnattn_image_desc* desc_dev, int N, const int* taps_host, const int* taps_dev,
                   long taps_len, int OH, int OW, const float* lut, void* dst, int dst_kind, int channels_last);
// overlay.hip: attention maps -> separable up-sampling + Gaussian (one operator per axis) -> min/max, blend over photographs
int attn_expand(hipStream_t st, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh, int OH,
                int OW, float* S, float* lohi, float* partial);
int attn_overlay(hipStream_t st, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh, int OH,
                 int OW, const float* S, const float* partial, const uint8_t* img, int n_img, const int* idx_host,
                 const int* idx_dev, const float* beta, uint8_t* out);
int attn_strips(int OH);
// textmetrics.hip: caption text metrics over token ids (n-gram statistics, LCS / ROUGE-L, CIDEr-D); layouts in include/scnattn.h
int text_max_len();
int text_ngram_stats(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                     int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                     int n_skip_ref, int32_t* stats);
int text_lcs(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
             const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
             int32_t* lcs, double* score, double* mean);
int text_ref_keys(hipStream_t st, int n, int N, int R, const int32_t* ref, int Lr, const int32_t* ref_len,
                  const int32_t* skip_ref, int n_skip_ref, int64_t* keys, int32_t* flag);
int text_cider(hipStream_t st, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
               const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
               const int64_t* table_keys, const int32_t* table_df, const long* table_off, long n_images, double* score,
               double* mean, int32_t* flag);
// tagmetrics.hip: tagger evaluation (per-image / per-tag AP in counting form, hits@k, tp/fp/fn, summary); layouts in include/scnattn.h
int tag_store_size(int S, long cap, size_t* score_bytes, size_t* label_bytes);
int tag_rows(hipStream_t st, int B, int S, const float* probs, long ld_probs, const void* targets, int targets_u8, long ld_targets,
             long row0, long cap, const int32_t* ks, int nk, float* store_scores, uint8_t* store_labels, double* row_ap,
             int32_t* row_npos, int32_t* row_hits, int32_t* flag);
int tag_cols(hipStream_t st, int S, long n, long cap, const float* store_scores, const uint8_t* store_labels,
             const float* thresholds, int nt, double* col_ap, int32_t* col_npos, int32_t* col_counts, int32_t* col_agree);
int tag_finalize(hipStream_t st, int S, long n, const int32_t* ks, int nk, int nt, const double* row_ap, const int32_t* row_npos,
                 const int32_t* row_hits, const double* col_ap, const int32_t* col_npos, const int32_t* col_counts,
                 const int32_t* col_agree, const int32_t* flag, double* summary);
int pool_permute_fwd(hipStream_t st, int B, int C, int Hin, int Win, int Ho, int Wo, const float* x,
                     long sxb, long sxc, long sxh, long sxw, float* y);
int pool_permute_bwd(hipStream_t st, int B, int C, int Hin, int Win, int Ho, int Wo, const float* dy,
                     float* dx, long sxb, long sxc, long sxh, long sxw);
int clamp_adam(hipStream_t st, long n, float* p, const float* g, float* m, float* v, double lr, double b1,
               double b2, double eps, int step, double clip, double gscale);
int mul_bcast(hipStream_t st, int T, int B, int N, const float* x, const float* q, float* out);
int reduce_slabs(hipStream_t st, int rows, int N, Slabs s, float* out);
// fp32 -> bf16 (round to nearest even), n elements (n % 4 == 0, 16-byte aligned input)
int f32_to_bf16(hipStream_t st, long n, const float* in, void* out);

// ---- batchnorm.hip (channels-last feature maps as [R = N*H*W, C] matrices) --------------------------
int bn_max_chunks();
int bn_stats(hipStream_t st, int R, int C, const void* x, int bf16, float eps, float momentum, float* partial,
             float* mean, float* invstd, float* run_mean, float* run_var, const float* gamma = nullptr,
             const float* beta = nullptr, float* ss_out = nullptr);
int bn_apply(hipStream_t st, int R, int C, const void* z, const void* res, int bf16, const float* mean,
             const float* invstd, const float* gamma, const float* beta, int relu, void* y);
int bn_bwd(hipStream_t st, int R, int C, const void* dy, const void* y, const void* z, int bf16, const float* mean,
           const float* invstd, const float* gamma, const float* beta, int relu, int train, float* partial, float* dbeta,
           float* dgamma, void* dz, void* dres);

// ---- finalize on load: channel-major partials [2][C][ldp] (cgemm statistics epilogues, cstats, bn_bwd_reduce_t, the stem) ----
int bn_finalize_t(hipStream_t st, long R, int C, const float* partial, int ldp, int nchunk, const float* shift, float eps,
                  float momentum, float* mean, float* invstd, float* run_mean, float* run_var, const float* gamma,
                  const float* beta, float* ss_out);
// bf16 != 0: the maps (z, res, y / dy, y, z, gout / g, z, dz) hold bf16; statistics, partials and parameters stay fp32
int bn_apply_fin(hipStream_t st, long R, int C, const void* z, const void* res, int bf16, const float* partial, int ldp, int nchunk,
                 const float* shift, float eps, float momentum, const float* gamma, const float* beta, int relu, void* y,
                 float* mean, float* invstd, float* run_mean, float* run_var, float* ss_out);
// Aliasing: gout may BE dy (the masked gradient replaces dy in place; csrc/block16.cpp does that); it must not overlap
// y or z, nor dy in any other way.
int bn_bwd_reduce_t(hipStream_t st, int R, int C, const void* dy, const void* y, const void* z, int bf16, const float* mean,
                    const float* invstd, int relu, float* partial, int ldp_cap, void* gout, int* nchunk_out);
// Aliasing: dz may BE g (dz replaces the masked gradient in place; scnattn/conv.py and csrc/block16.cpp do that); it must
// not overlap z, nor g in any other way.  In both entries a thread reads an element before the same thread writes it; the
// kernels rely on that order, not on their __restrict__ qualifiers, which these two pairs do not honour.
int bn_bwd_dx_fin(hipStream_t st, long R, int C, const void* g, const void* z, int bf16, const float* mean, const float* invstd,
                  const float* gamma, const float* partial, int ldp, int nchunk, float* dbeta, float* dgamma, void* dz);

// ---- bf16 convolution path (BASELINE configs[4]): cgemm16.hip, wgrad16.hip, misc.hip ----------------------------------------
int cgemm16(hipStream_t st, int M, int N, int K, const void* A, long lda, const void* B, long ldb, float beta, void* C, long ldc,
            int out_bf16, float* ws, long ws_floats, const ConvExtra* ex, int flip);
int wgrad16_3x3(hipStream_t st, int N, int H, int W, int C, int Co, const void* dy, const void* x, float* dw, float* ws,
                long ws_floats, int force_split);
int wgrad16_rows(hipStream_t st, int R, int C, int Co, const void* dy, const void* x, long src_rows, float* dw, long ldo,
                 int gs, int gHi, int gWi, int gHo, int gWo, int goh, int gow, float* ws, long ws_floats, int force_split);
// One launch converts every convolution weight of a trunk: fp32 master [Cout][taps][Cin] -> bf16 copy in the same layout
// and a TRANSPOSED bf16 copy [Cin][taps][Cout] (the B operand of the d-input products).  desc: device array of
// WeightDesc, tile_prefix[n+1]: exclusive prefix sums of each weight's 32 x 32 tile count (taps * Cout/32 * Cin/32).
struct WeightDesc { const float* src; void* dst; void* dst_t; int cout, taps, cin, pad; };
int bf16_weights(hipStream_t st, int n, const WeightDesc* desc, const int* tile_prefix, int total_tiles);

}  // namespace scn
