/* libscnattn -- C ABI of the MI355X (gfx950) SCN+Attention training path.
 *
 * The reference (rayandrew/indonesian-image-captioning) has no FFI layer: its hot path is eager
 * PyTorch.  This header is the boundary that sits UNDER the reference's nn.Module API
 * (SURVEY.md 8b); each entry point names the reference code it replaces (paths relative to the
 * reference checkout).  The Python binding a maintainer adds is in INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - plain pointers + sizes, fp32 row-major device memory, int64 token ids, no torch types;
 *   - every call is asynchronous on the hipStream_t passed as `void* stream` (0 = null stream);
 *   - the library allocates nothing: callers pass workspaces sized by scnattn_seq_workspace();
 *   - return 0 on success, <0 for invalid arguments, >0 = hipError_t; message (thread-local) from
 *     scnattn_last_error(); no exceptions or aborts cross this boundary; entry points are
 *     re-entrant (autograd calls backward from its own thread).
 */
#ifndef SCNATTN_H
#define SCNATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCNATTN_VERSION 109 /* 0.1.9: - the scnattn_seq_bwd_streams entry point: decoder weight gradients on a second stream were not faster; - option dec_tail: the cell
                               kernels inside the skinny launches were slower; DESIGN.md keeps the numbers;
                               + tagger losses for rare tags on the logits: positive weights, focal, asymmetric (scnattn_tag_loss_options,
                               scnattn_tagloss_fwd, scnattn_tagloss_bwd; new symbols only, the version stays);
                               + image augmentation in the input assembly: crop, flip, colour jitter (scnattn_augment_config,
                               scnattn_u8_mean_grey, scnattn_augment_draw, scnattn_u8_gather_augment; new symbols only, the version stays);
                               + tagger evaluation: per-image / per-tag average precision, hits@k, tp/fp/fn per threshold
                               (scnattn_tag_store_size, scnattn_tag_rows, scnattn_tag_cols, scnattn_tag_finalize; new symbols only, the
                               version stays);
                               + scoring given captions: teacher-forced log-probabilities, rank and arg-max per token (scnattn_rollout_*_sc,
                               scnattn_rollout_score; new symbols only, the version stays);
                               + scheduled sampling: gold and sampled input words mixed by a coin (scnattn_rollout_*_ss,
                               scnattn_rollout_pick_mixed; new symbols only, the version stays);
                               + the caption metrics in the loss pass (scnattn_caption_loss_metrics_fwd; new symbol only, the version stays);
                               + constrained beam search: required words, beam banks (scnattn_constraints, scnattn_beam_*_con,
                               scnattn_ensemble_*_con, scnattn_beam_row_topk_con, scnattn_beam_row_topk_ens_con, scnattn_beam_merge_banks; new
                               symbols only, the version stays);
                               + diverse beam search: groups of beams, a Hamming penalty (scnattn_diversity, scnattn_beam_*_div,
                               scnattn_ensemble_*_div, scnattn_beam_merge_groups, scnattn_beam_row_topk_groups; new symbols only, the
                               version stays);
                               + truncated sampling: top-k / nucleus rollouts (scnattn_sample_filter, scnattn_rollout_*_f; new symbols only,
                               the version stays);
                               + search options: n-gram blocking, minimum length, banned tokens (scnattn_search_options, scnattn_beam_*_opt,
                               scnattn_ensemble_*_opt; new symbols only, the version stays);
                               + ensemble beam search (scnattn_ensemble_*, scnattn_beam_row_topk_ens; new symbols only, the version stays);
                               + sampled rollouts and the reward-weighted loss for self-critical training (scnattn_rollout_*,
                               scnattn_caption_loss_weighted_fwd/_bwd; new symbols only, the version stays);
                               0.1.8: + the tagger head (scnattn_tag_pool_fwd/_bwd, scnattn_bce_fwd/_bwd; new symbols only, the version stays), + eval-mode BatchNorm epilogue on bf16 maps (scnattn_bn_eval16, scnattn_conv1x1_fwd_bn_eval16, _conv3x3_fwd_bn_eval16;
                               new symbols only, the version stays), + batched beam search (scnattn_beam_*; new symbols only, the version stays), + eval-mode BatchNorm epilogue (scnattn_bn_eval, scnattn_conv1x1_fwd_bn_eval,
                               _conv3x3_fwd_bn_eval; new symbols only, the version stays), + bf16 trunk kernels (scnattn_cgemm16, _conv3x3_fwd16/_dgrad16, _wgrad16_*, _bf16_weights), split-K
                               epilogues inside the GEMM launch (options cgemm_combine, cgemm_combine_max);
                               0.1.7: + halo-staged 3x3 weight gradient, strided 3x3 d input, the stem (scnattn_stem_*), BatchNorm
                               finalize on load; - whole-block drivers, scnattn_stream_*, the experiment options of rounds 1-2 */

int scnattn_version(void);
const char* scnattn_last_error(void);
/* Process-wide options.  Every entry point is re-entrant and takes its stream explicitly; what is left here is
 *   - what a caller chooses once per process: "decoder_bf16" (0 fp32; 1: the sequence drivers stream bf16 copies of the
 *     recurrent weights, att1 and the encoder map, fp32 accumulate / state / gradients; 2: also the bf16 matrix
 *     instruction in the per-step products -- BASELINE configs[4]; needs D, F, E, A multiples of 4) and "profile" (1: bracket
 *     the recurrence loops with HIP events on the caller's stream; 2: also every attn_context launch; see
 *     scnattn_profile_collect);
 *   - policy overrides used by tools/ sweeps and the tests that cover both sides of a policy: "ksplit" (split-K factor of the
 *     skinny GEMMs; 0 = auto), "attn_depth", "use_cgemm" (0: every dense product on the round-1 sgemm kernel), "cgemm_mi"
 *     (0 auto; 1 / 2 force the 64- / 128-row tile), "cgemm_target" (workgroups a split-K product aims for, 512),
 *     "cgemm_kmin" (smallest K per slab, 128), "gemm_target" / "gemm_gate" / "gemm_kmin" / "gemm_kmin_small" (the same for
 *     sgemm), "cgemm_combine" (1, default: a split product's epilogue is run inside the launch by the workgroup that arrives
 *     last at each tile -- write-through slabs, arrival counters per stream, bit-identical to the reduce launch; 2: plain
 *     slab stores + an agent release; 0: always the reduce launch), "cgemm_combine_max" (deepest split combined in-launch, 8).
 *     The experiment switches of rounds 1-2 (fuse_attn, chains, attn_handoff, cgemm_stagger, cgemm_w41, cgemm_vec,
 *     bn_gfirst, skinny_tail) and "dec_tail" (the decode step's element-wise cell kernels inside the skinny launches that
 *     feed them: bit-identical, measured slower) were removed together with the code paths they selected; DESIGN.md keeps
 *     their numbers.
 * Returns -1 for an unknown name or an out-of-range value. */
int scnattn_set_option(const char* name, int value);
/* Sums since the last call: out6 = {forward loop ms, forward steps, backward loop ms, backward steps,
 * attn_context ms, attn_context launches}.  Synchronises on the recorded events. */
int scnattn_profile_collect(double* out6);

/* ---- dimensions of one decoder (models/decoders/attention_scn.py:28-56, pure_scn.py:26-48) ------ */
typedef struct {
    int B;       /* batch rows                                                         */
    int P;       /* pixels per image (14*14)                                           */
    int E;       /* encoder_dim                                                        */
    int A;       /* attention_dim   (ignored when has_att == 0)                        */
    int D;       /* decoder_dim == SCNCell.hidden_size                                 */
    int F;       /* factored_dim                                                       */
    int M;       /* embed_dim                                                          */
    int S;       /* semantic_dim (tags)                                                */
    int V;       /* vocab_size                                                         */
    int T;       /* decode steps = max(decode_lengths)                                 */
    int L;       /* width of the caption tensor (>= T)                                 */
    int has_att; /* 1: AttentionSCN (SCNCell input = M+E), 0: PureSCN (input = M)      */
} scnattn_dims;

/* Parameter pointers, named after the reference's state_dict keys.  The same struct (with
 * writable memory behind it) receives the gradients in scnattn_seq_bwd. */
typedef struct {
    float* attention_encoder_att_weight; /* [A,E]   models/attention.py:18 */
    float* attention_encoder_att_bias;   /* [A]                            */
    float* attention_decoder_att_weight; /* [A,D]   models/attention.py:20 */
    float* attention_decoder_att_bias;   /* [A]                            */
    float* attention_full_att_weight;    /* [1,A]   models/attention.py:22 */
    float* attention_full_att_bias;      /* [1]                            */
    float* embedding_weight;             /* [V,M]   attention_scn.py:43    */
    float* decode_step_weight_ia;        /* [I,4F]  models/scn_cell.py:29  */
    float* decode_step_weight_ib;        /* [S,4F]                         */
    float* decode_step_weight_ic;        /* [D,4F]                         */
    float* decode_step_weight_ha;        /* [D,4F]                         */
    float* decode_step_weight_hb;        /* [S,4F]                         */
    float* decode_step_weight_hc;        /* [D,4F]                         */
    float* decode_step_bias_ih;          /* [4D]                           */
    float* decode_step_bias_hh;          /* [4D]                           */
    float* init_h_weight;                /* [D,E]   attention_scn.py:48    */
    float* init_h_bias;                  /* [D]                            */
    float* init_c_weight;                /* [D,E]                          */
    float* init_c_bias;                  /* [D]                            */
    float* f_beta_weight;                /* [E,D]   attention_scn.py:52    */
    float* f_beta_bias;                  /* [E]                            */
    float* fc_weight;                    /* [V,D]   attention_scn.py:55    */
    float* fc_bias;                      /* [V]                            */
} scnattn_params;

/* Optional: encoder_out described as a FIXED LINEAR POOLING of a smaller feature map x [B,Q,E] -- what
 * models/encoders/caption.py:41-43 produces (AdaptiveAvgPool2d(14) of the trunk's 8x8 map at 256x256 input,
 * an up-sampling 1-or-2-tap average, then permute):
 *     enc[b][p][:] = sum_{k<4} tap_w[p][k] * x[b][tap_idx[p][k]][:]        (unused taps: weight 0, index 0)
 * With it the sequence drivers take x in place of enc and never materialise the pooled map: by linearity
 * encoder_att runs on Q rows (att1 = pool(x.We^T) + be), the attention context and its gradient read Q rows
 * per image instead of P (sum_p alpha_p enc_p = sum_q alphaq_q x_q, alphaq = pool^T alpha), and d x comes out
 * directly.  SURVEY.md 8d names this shortcut.  All tables live in device memory.
 *   qtap_*: the transpose -- for source pixel q the (p, weight) pairs that read it, padded with index -1;
 *   col_w[q] = (sum_p weight(p,q)) / P, so that mean_p enc[b][p] = sum_q col_w[q] x[b][q]. */
typedef struct scnattn_pool {
    int Q;                   /* source pixels per image (Q <= P) */
    int qtap_max;            /* row length of qtap_idx / qtap_w (<= 64) */
    const int32_t* tap_idx;  /* [P][4] */
    const float* tap_w;      /* [P][4] */
    const int32_t* qtap_idx; /* [Q][qtap_max] */
    const float* qtap_w;     /* [Q][qtap_max] */
    const float* col_w;      /* [Q] */
} scnattn_pool;

/* Bytes of the two workspaces of the sequence drivers (pool may be NULL).  `saved` carries forward state to
 * the backward pass; `scratch` is free after each call and may be re-used, as may `saved` once its backward has run.
 * Zero-fill `saved` before scnattn_seq_fwd and `scratch` before scnattn_seq_bwd, unless every caption decodes at
 * every step (bt_host[T-1] == B), in which case every element is written before it is read.  The scratch of
 * scnattn_seq_fwd needs no fill in either case: the forward writes every word of it before reading it.
 * (tests/test_gpu_seq_driver.py holds the drivers to this with NaN-filled workspaces.) */
int scnattn_seq_workspace(const scnattn_dims* d, const scnattn_pool* pool, size_t* saved_bytes, size_t* scratch_bytes);

/* Teacher-forced decoder forward over all T steps: replaces the loop of
 * models/decoders/attention_scn.py:124-156 (pure_scn.py:114-138 when has_att == 0), i.e. per step
 * Attention.forward (models/attention.py:35-44), the f_beta gate, SCNCell.forward/recurrent_step
 * (models/scn_cell.py:62-154), dropout and fc.
 *   enc     [B,P,E]  encoder output, rows already permuted by sort_ind ([B,Q,E] = x when pool != NULL)
 *   tags    [B,S]    semantic input, NOT permuted (reference quirk, attention_scn.py:152)
 *   caps    [B,L]    int64 sorted captions;  dl_dev [B] int32 decode lengths (device)
 *   bt_host [T]      host array: active rows at step t (non-increasing)
 *   drop_mask [B,T,D] pre-scaled dropout mask or NULL
 *   preds   [B,T,V]  out (fully written; rows past a caption's length are 0)
 *   alphas  [B,T,P]  out, must be zero-filled by the caller (NULL when has_att == 0) */
int scnattn_seq_fwd(void* stream, const scnattn_dims* d, const scnattn_params* w, const float* enc,
                    const float* tags, const int64_t* caps, const int32_t* dl_dev, const int32_t* bt_host,
                    const float* drop_mask, float* saved, float* scratch, float* preds, float* alphas,
                    const scnattn_pool* pool);

/* Gradient of scnattn_seq_fwd (what autograd derives for the reference's loop).  `g` receives
 * d loss / d parameter (fields may be NULL to skip; embedding_weight must be zero-filled: rows
 * are accumulated -- it is the ONE accumulated output: every other one is overwritten, so a second call on the
 * same `saved` gives the same bits once embedding_weight is zeroed again).  denc [B,P,E] ([B,Q,E] = d x when
 * pool != NULL) and dtags [B,S] may be NULL; an omitted output changes no other.  dalphas may be NULL (= zeros).
 * Finite values in the dpreds / dalphas cells at t >= decode length change no result. */
int scnattn_seq_bwd(void* stream, const scnattn_dims* d, const scnattn_params* w, const float* enc,
                    const float* tags, const int64_t* caps, const int32_t* dl_dev, const int32_t* bt_host,
                    const float* drop_mask, const float* saved, float* scratch, const float* dpreds,
                    const float* dalphas, const scnattn_params* g, float* denc, float* dtags,
                    const scnattn_pool* pool);

/* ---- batched beam search: the reference's sample() (models/decoders/attention_scn.py:160-296, pure_scn.py:142-249,
 * pure_attention.py:153-281), which eval_caption.py:96-131 calls once per image, for N images at once ---------------------
 * dims: B = N images; T and L are ignored (max_steps is passed explicitly; the reference stops after 51).  K = beam_size
 * slots per image, 1 <= K <= 8 <= V; rows of every per-step buffer are n*K + j and nothing shrinks: per image `nsrc` live
 * source beams (1 at the first step: the reference selects from scores[0]) and `kk` beams still to fill.  Each step
 * takes the top kk of the nsrc x V candidates score[j] + log_softmax(fc(h_j))[v], ordered by (value descending, flat
 * index j*V + v ascending -- the TIE RULE, which the reference leaves to topk); <end> picks are recorded as completed (the
 * running best replaced only on a strictly greater score), the others compacted to slots 0.. in rank order.  Sequences
 * and attention maps are not copied per step: token[t][row] / parent[t][row] / alpha[t][row][P] are recorded and the
 * caller follows the parent chain.  The k rows of an image read att1[n] / enc[n] once (csrc/beam.hip).
 * fp32 only: option "decoder_bf16" is ignored here.  Dense encoder_out only (no scnattn_pool).
 *   enc [N,P,E], tags [N,S] (NOT expanded per beam); ws: scnattn_beam_workspace bytes, 16-byte aligned, owned by the caller
 *   scnattn_beam_init   set-up (weight re-layout, att1 once per image, tag factors, initial state, <start> embeddings)
 *   scnattn_beam_steps  enqueues steps t0 .. t0+n_steps-1 (0-based, clipped to max_steps); steps on a finished batch are
 *                       no-ops, so the host may enqueue chunks and read `open_images` (one int) in between
 *   scnattn_beam_layout offsets (in 4-byte elements from ws) of the results, in this order:
 *       0 open_images int[1]   1 nsrc int[N]   2 kk int[N]   3 ncomp int[N]   4 best_idx int[N] (-1: none completed)
 *       5 best_score f32[N]    6 scores f32[N*K] (open slots)   7 comp_score f32[N*K]   8 comp_step int[N*K] (0-based)
 *       9 comp_parent int[N*K] (source slot that picked <end>)  10 token int[max_steps][N*K]   11 parent int[max_steps][N*K]
 *       12 alpha f32[max_steps][N*K][P] (-1 without attention), alpha[t][row] belonging to SOURCE slot `row` of step t
 *     completed beams of image n sit at n*K .. n*K+ncomp[n]-1 in completion order (by step, within a step by rank). */
#define SCNATTN_BEAM_NOFF 13
int scnattn_beam_workspace(const scnattn_dims* d, int K, int max_steps, size_t* bytes);
int scnattn_beam_layout(const scnattn_dims* d, int K, int max_steps, long* offsets);
int scnattn_beam_init(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_params* w, const float* enc,
                      const float* tags, int start_token, float* ws);
int scnattn_beam_steps(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_params* w, const float* enc,
                       int end_token, int t0, int n_steps, float* ws);
/* ---- ensemble beam search: up to SCNATTN_MAX_ENSEMBLE decoders under ONE search state -----------------------------------
 * Published caption scores are reported for an ensemble of the trained models; the three decoders read the same encoder map
 * and share one vocabulary.  The search above, with the candidates of a step ranked by a COMBINED distribution.  With
 * l_mv = log_softmax(fc_m(h_mj))[v] of member m:
 *   mode 0 ("logprob", weighted geometric mean of the probabilities)   c_v = sum_m w_m l_mv, summed in member order
 *   mode 1 ("prob", weighted arithmetic mean of the probabilities)     c_v = a_v + log(sum_m w_m exp(l_mv - a_v)),
 *                                                                      a_v = max_m l_mv (finite when every exp underflows)
 * and a step takes the top kk of score[j] + c_v under the TIE RULE.  Every member keeps its own recurrent state, gathered by
 * the same parents.  M = 1, mode 0, w = 1 is, bit for bit, the search above.
 *   dims / w   arrays of M structs.  Members may differ in has_att, A, D, F, M (embed_dim) and S; they must agree in B, P, E
 *              and V (refused otherwise).
 *   enc [N,P,E] one map for all members; tags: HOST array of M device pointers, tags[m] [N,S_m]
 *   member_w   HOST array of M fp32 weights, each positive and finite, summing to 1 (normalise in double, then round)
 *   alpha_member  the member whose attention maps are recorded (-1, or a member without attention: none)
 *   scnattn_ensemble_layout  the 13 offsets of scnattn_beam_layout, in the same order (12: the maps of alpha_member or -1)
 *   ws: scnattn_ensemble_workspace bytes, 16-byte aligned: one search state, one step workspace per member, ONE split-K
 *   scratch for all of them -- everything runs on the caller's stream, in order.
 * A step launches the decode part of every member (9-10 launches with attention, 6-7 without), one _row_topk_ens, one
 * _merge and one _advance per member.  alpha_member, M, K and max_steps must be the same in the four calls.
 * fp32 only: option "decoder_bf16" is ignored here.  Dense encoder_out only (no scnattn_pool).
 *   scnattn_beam_row_topk_ens  the selection kernel alone: logits / ld / w are HOST arrays of M entries (row r of member m at
 *   logits[m] + r*ld[m], ld[m] >= V); refuses (-1) M outside [1, 4], K outside [1, 8], V < K, a null row, ld < V, a
 *   weight that is not positive and finite, mode outside {0, 1}.  Rows of dead slots are neither read nor written. */
#define SCNATTN_MAX_ENSEMBLE 4
int scnattn_ensemble_workspace(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member, size_t* bytes);
int scnattn_ensemble_layout(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member, long* offsets);
int scnattn_ensemble_init(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                          const scnattn_params* w, const float* enc, const float* const* tags, int start_token, float* ws);
int scnattn_ensemble_steps(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                           const scnattn_params* w, const float* enc, const float* member_w, int mode, int end_token, int t0,
                           int n_steps, float* ws);
int scnattn_beam_row_topk_ens(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                              const float* w, int mode, const float* scores, const int32_t* nsrc, float* outv, int32_t* outi,
                              int force_passes);
/* ---- search OPTIONS: n-gram blocking, a minimum length, banned tokens (both searches above) ----------------
 * The reference's search has none of these; the semantics are this library's.  Let w_0 .. w_{t-1} be the words the open beam
 * in slot j has emitted before 0-based step t (<start> is not among them).  At step t candidate (j, v) is EXCLUDED when
 *   1. v is one of the n_banned <= 64 tokens of `banned` (<end> may not be among them), or
 *   2. v == <end> and t < min_length                                (0 <= min_length <= max_steps - 1), or
 *   3. g = no_repeat_ngram in [1, 8], t >= g, and there is an i in [0, t - g] with w_i .. w_{i+g-2} == w_{t-g+1} .. w_{t-1}
 *      and w_{i+g-1} == v: picking v would repeat an n-gram of g words (g = 1: v occurs in the history).  <end> is never
 *      in a history, so this rule never excludes it.  g = 0: the rule is off.
 * An excluded candidate is not a candidate -- NOTHING IS RENORMALISED: the log-sum-exp runs over all V logits, scores stay
 * sums of the model's log-probabilities, and a step that excludes nothing picks what the plain kernel picks, with its fp32
 * values.  Order, tie rule, dead slots, nsrc / kk, completion records and the open-beam fallback are those of the search
 * above.  Every live row must still offer K candidates: a call is REFUSED (-1) unless
 *       V - n_banned - 1 - (no_repeat_ngram >= 1 ? max_steps : 0) >= K
 * (sufficient: at most n_banned + 1 + t words can be excluded), as are options out of range, a banned token outside the
 * vocabulary and a banned <end> (checked where the call knows <end>: _steps_opt).
 * The per-beam history lives in the workspace as int32 [2][N*K][max_steps]: the selection of step t reads buffer t & 1
 * (t entries per row), the advance gathers the parent slot's entries into the other buffer and appends the step's word;
 * dead slots get slot 0's copy.  After `steps` steps the current buffer is steps & 1.  The launches per step are those of
 * the plain search: the selection and the advance run in their _opt form.
 *   _workspace_opt / _layout_opt / _init_opt / _steps_opt   the four calls of each search with the options after max_steps
 *       (the ensemble: after alpha_member); the same options in all four.  _layout_opt writes SCNATTN_BEAM_NOFF_OPT
 *       offsets: the 13 of scnattn_beam_layout, then 13 history int[2][N*K][max_steps].
 *   scnattn_beam_row_topk_opt / _row_topk_ens_opt   the selection alone for step t: hist int32 [N*K][max_steps] holds t
 *       entries per row (may be NULL when no_repeat_ngram == 0); <end> = end_token is excluded while t < min_length.
 *       outv / outi as _row_topk; rows of dead slots are neither read nor written.  _row_topk_opt is _row_topk_ens_opt
 *       with one member of weight 1 in mode 0, which writes the bits of _row_topk when nothing is excluded.
 *   scnattn_beam_advance_opt   _advance, and hist_dst[row][0..t-1] = hist_src[n*K + parent_t[row]][0..t-1],
 *       hist_dst[row][t] = token_t[row] (0 <= t < max_steps, hist_src != hist_dst). */
#define SCNATTN_MAX_BANNED 64
#define SCNATTN_MAX_NGRAM 8
#define SCNATTN_BEAM_NOFF_OPT 14
typedef struct {
    int32_t min_length;
    int32_t no_repeat_ngram;
    int32_t n_banned;
    int32_t banned[SCNATTN_MAX_BANNED];
} scnattn_search_options;
int scnattn_beam_workspace_opt(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt, size_t* bytes);
int scnattn_beam_layout_opt(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt, long* offsets);
int scnattn_beam_init_opt(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_params* w, const float* enc, const float* tags, int start_token, float* ws);
int scnattn_beam_steps_opt(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_params* w, const float* enc, int end_token, int t0, int n_steps, float* ws);
int scnattn_ensemble_workspace_opt(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, size_t* bytes);
int scnattn_ensemble_layout_opt(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, long* offsets);
int scnattn_ensemble_init_opt(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_params* w, const float* enc,
                              const float* const* tags, int start_token, float* ws);
int scnattn_ensemble_steps_opt(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_params* w, const float* enc,
                               const float* member_w, int mode, int end_token, int t0, int n_steps, float* ws);
int scnattn_beam_row_topk_opt(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                              const int32_t* nsrc, const scnattn_search_options* opt, int end_token, int t,
                              const int32_t* hist, int max_steps, float* outv, int32_t* outi, int force_passes);
int scnattn_beam_row_topk_ens_opt(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                                  const float* w, int mode, const float* scores, const int32_t* nsrc,
                                  const scnattn_search_options* opt, int end_token, int t, const int32_t* hist,
                                  int max_steps, float* outv, int32_t* outi, int force_passes);
int scnattn_beam_advance_opt(void* stream, int N, int K, int D, int M, int V, int t, int max_steps, const float* hs,
                             const float* cs, const int32_t* parent_t, const int32_t* token_t, const float* table,
                             const int32_t* hist_src, int32_t* hist_dst, float* hd, float* cd, float* emb);
/* ---- DIVERSE beam search: groups of beams, a Hamming penalty (Vijayakumar et al. 2016; both searches above) --
 * The reference has no such search; the semantics are this library's.  "The search order" is the order above: value
 * descending, flat index ascending.  The K slots of an image are split into G = groups groups of Kg = K / G slots,
 * 1 <= G, 1 <= Kg, G * Kg = K <= 8 <= V; penalty lambda >= 0, finite.  The slots of image n are the rows n*K + g*Kg + s.
 *   Every group is the search above with beam size Kg: it starts from one live source (its slot 0, the <start> row), its kk
 *   shrinks as its beams complete, it keeps its own completions in completion order (by step, within a step by rank) at
 *   n*K + g*Kg .., its own running best (replaced only on a strictly greater score) and its own open-beam fallback, and it
 *   finishes on its own.  A finished group is a no-op and penalises nobody.
 *   At step t the groups of an image are handled in order g = 0 .. G-1.  c(g, v) is the number of picks of the groups h < g
 *   at this step whose word is v -- all of their kk picks count, <end> picks like any other word.  Candidate (j, v) of group
 *   g has the raw value r = score[j] + logp_j(v), the value of the search above with the same bits, and the selection value
 *   a = fmaf(-lambda, (float)c(g, v), r) in fp32.  The group takes its top kk by (a descending, flat index j_in_group*V + v
 *   ascending).
 *   NOTHING OF THE PENALTY IS STORED: scores, comp_score and best_score hold raw values r, so scores stay sums of the
 *   model's log-probabilities, as with the search options.  Slots are compacted in rank order of a; dead slots get a copy of
 *   the group's slot 0.  parent[t][row] is a slot of the IMAGE (g*Kg + j), as is comp_parent, so _advance and _advance_opt
 *   are used unchanged and with no_repeat_ngram the history follows the same parents.
 *   Search options compose: the exclusions act in the row selection as above, and the candidate-count refusal uses
 *   K = G * Kg.  A length penalty chooses among a group's finished beams on the host, per group.
 *   G = 1 is the search above bit for bit, for any lambda: c == 0 and fmaf(-lambda, 0, r) == r.
 * Why K candidates per row are enough: group g is penalised on at most g*Kg <= K - Kg distinct words, a penalty only moves a
 * candidate down, and exclusions happen before the ranking; so whatever group g can take from a row lies within that row's
 * unpenalised top Kg + g*Kg <= K in the search order.  The launches per step are exactly those of the search above.
 *   _workspace_div / _layout_div / _init_div / _steps_div   the four calls of each search with `opt` (may be NULL: no
 *       options) and `div` after max_steps (the ensemble: after alpha_member); K is the TOTAL G * Kg; the same opt / div
 *       in all four.  _layout_div writes SCNATTN_BEAM_NOFF_OPT offsets, those of _layout_opt (13: -1 without options),
 *       with these shapes: 1 nsrc, 2 kk, 3 ncomp, 4 best_idx, 5 best_score are [N*G], entry n*G + g; nsrc counts the live
 *       slots g*Kg .. g*Kg + nsrc - 1 of the group; 0 open_images counts the images with an open group.
 *       With G > 1 the attention kernels of a step take K live slots for an image while any of its groups is open and 0
 *       afterwards: dead slots hold finite copies, so computing them is correct, only wasted (G = 1: nsrc, as above).
 *   scnattn_beam_merge_groups   the merge alone, on the state arrays a _layout_div describes (state: the 12 pointers of
 *       scnattn_beam_merge); Kg slots per group, K % Kg == 0.
 *   scnattn_beam_row_topk_groups   _row_topk with the group liveness: nsrc int[N * K/Kg], row n*K + g*Kg + s is live when
 *       s < nsrc[n * K/Kg + g]; every live row still gets K candidates; rows of dead slots are neither read nor written.
 * Refused (-1): groups < 1, K % groups != 0, K outside [1, 8], a penalty that is negative, NaN or infinite, and whatever the
 * searches above refuse. */
typedef struct {
    int32_t groups;
    float penalty;
} scnattn_diversity;
int scnattn_beam_workspace_div(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                               const scnattn_diversity* div, size_t* bytes);
int scnattn_beam_layout_div(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                            const scnattn_diversity* div, long* offsets);
int scnattn_beam_init_div(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_diversity* div, const scnattn_params* w, const float* enc, const float* tags,
                          int start_token, float* ws);
int scnattn_beam_steps_div(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_diversity* div, const scnattn_params* w, const float* enc, int end_token, int t0,
                           int n_steps, float* ws);
int scnattn_ensemble_workspace_div(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, const scnattn_diversity* div, size_t* bytes);
int scnattn_ensemble_layout_div(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, const scnattn_diversity* div, long* offsets);
int scnattn_ensemble_init_div(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_diversity* div, const scnattn_params* w,
                              const float* enc, const float* const* tags, int start_token, float* ws);
int scnattn_ensemble_steps_div(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_diversity* div, const scnattn_params* w,
                               const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps,
                               float* ws);
int scnattn_beam_merge_groups(void* stream, int N, int K, int Kg, float penalty, int V, int end_token, int t,
                              const float* candv, const int32_t* candi, void* const* state);
int scnattn_beam_row_topk_groups(void* stream, int N, int K, int Kg, int V, const float* logits, long ld, const float* scores,
                                 const int32_t* nsrc, float* outv, int32_t* outi, int force_passes);
/* ---- CONSTRAINED beam search: required words, beam banks (Anderson et al. 2017; Post & Vilar 2018) ----------
 * The reference has no such search; the semantics are this library's.  "The search order" is the order above: value
 * descending, flat index j*V + v ascending.
 *   Per image n a list req[n] of C_n REQUIRED words, 0 <= C_n <= SCNATTN_MAX_REQUIRED = 4, distinct token ids in [0, V), C_n
 *   free per image: int32 [N][4], the C_n words first, padded with -1.
 *   STATE.  Every slot carries met, the bitmask of the image's required words that occur in its history (bit c: req[n][c]);
 *   it starts at 0.  bank(slot) = popcount(met).  A child's mask is met(parent) | bit(c) when its word is req[n][c], else
 *   met(parent).
 *   ROW SELECTION of a live row (n, j) at step t.  The row's ORDINARY candidates are all words except what the options
 *   exclude, the row's UNMET required words, and <end> unless the row has met all C_n words: a caption cannot finish with a
 *   requirement open.  The kernel emits the row's top K ordinary candidates, as above, and separately 4 REQUIRED candidates:
 *   entry c is (score[j] + c_v(req[n][c]), req[n][c]) when c < C_n, c is unmet in the row and the options do not exclude the
 *   word (the n-gram rule can), else (-inf, -1).  The value is computed by the expression the K rounds use for that word, to
 *   the bit.  NOTHING IS RENORMALISED: scores stay sums of the model's log-probabilities.
 *   MERGE of image n.  An ordinary candidate of row j lies in bank popcount(met_j), a required one in bank popcount(met_j) + 1;
 *   within a bank candidates are in the search order.  The kk picks are made ROUND-ROBIN over the banks: visit b = C_n,
 *   C_n - 1, .., 0, then again from C_n; at each visit take the bank's best candidate not yet picked, if it has one; stop at
 *   kk picks.  The picked set is then arranged in the search order, and in that order everything is as in _merge: <end> picks
 *   are recorded as completed (the running best replaced only by a strictly greater score), the others compacted to slots
 *   0 .. nopen-1 with their new met, dead slots get slot 0's copy.
 *   Why K ordinary candidates per row are enough: a bank receives at most kk <= K picks, a row's ordinary candidates all lie
 *   in ONE bank, and a bank's picks are a prefix of its order; so whatever is picked from a row lies within that row's top K
 *   ordinary candidates, and its required candidates are all emitted.
 *   STEP LIMIT.  An image with no completed beam after max_steps falls back to the open beam with the largest popcount(met),
 *   ties to the higher score, then to the lower slot (C_n = 0: the fallback above); the caller reads scores / met.  Beams that
 *   can no longer satisfy their requirements in the steps left are not pruned; the result reports what was met.
 *   C_n = 0 for every image is the search above BIT FOR BIT (one bank, nothing extra excluded, the picks are the top kk), and
 *   images are independent: an image with an empty list in a mixed batch gets exactly its plain result.
 *   Search options compose (the exclusions are the union; a length penalty chooses among finished beams, all of which satisfy
 *   the requirements), as does the ensemble (the selection kernel is shared).  Groups (_div) do NOT compose, and multi-word
 *   phrases are out of scope.  The launches per step are those of the search above: the selection runs in its constrained
 *   flavour and _merge_banks replaces _merge.
 *   _workspace_con / _layout_con / _init_con / _steps_con   the four calls of each search with `opt` (may be NULL: no options)
 *       and `con` after max_steps (the ensemble: after alpha_member); the same opt / con in all four.  con->required is a HOST
 *       array that every call checks and _init_con copies into the workspace (it returns after the copy).  _layout_con writes
 *       SCNATTN_BEAM_NOFF_CON offsets: those of _layout_opt (13: -1 without options), then 14 met int[N*K] (the masks of the
 *       slots after the last step) and 15 the required table int[N][4].
 *   scnattn_beam_row_topk_con / _row_topk_ens_con   the selection alone for step t: _row_topk_opt / _row_topk_ens_opt (opt
 *       may be NULL) with required int[N][4] and met int[N*K] ON THE DEVICE and the outputs reqv f32 / reqi int [N*K][4].
 *       Rows of dead slots are neither read nor written.
 *   scnattn_beam_merge_banks   the merge alone, on the state arrays a _layout_con describes (state: the 12 pointers of
 *       scnattn_beam_merge) with met int[N*K] and required int[N][4] on the device.
 * Refused (-1): con NULL or without a table, n_images != B, a required word equal to <start> (checked by _init_con), <end>
 * (_steps_con) or con->pad_token, a required word the options ban, a duplicate within an image, an id outside the
 * vocabulary, a word behind a -1 of its row (more than 4 words cannot be stated), K outside [1, 8], unless
 *       V - n_banned - 1 - (no_repeat_ngram >= 1 ? max_steps : 0) - 4 >= K,
 * and whatever the searches above refuse. */
#define SCNATTN_MAX_REQUIRED 4
#define SCNATTN_BEAM_NOFF_CON 16
typedef struct {
    int32_t n_images;           /* must equal dims.B */
    int32_t pad_token;          /* <pad>, refused as a required word; -1: not stated */
    const int32_t* required;    /* HOST int32 [n_images][4]: the C_n words of image n, then -1 */
} scnattn_constraints;
int scnattn_beam_workspace_con(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                               const scnattn_constraints* con, size_t* bytes);
int scnattn_beam_layout_con(const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                            const scnattn_constraints* con, long* offsets);
int scnattn_beam_init_con(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                          const scnattn_constraints* con, const scnattn_params* w, const float* enc, const float* tags,
                          int start_token, float* ws);
int scnattn_beam_steps_con(void* stream, const scnattn_dims* d, int K, int max_steps, const scnattn_search_options* opt,
                           const scnattn_constraints* con, const scnattn_params* w, const float* enc, int end_token, int t0,
                           int n_steps, float* ws);
int scnattn_ensemble_workspace_con(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                   const scnattn_search_options* opt, const scnattn_constraints* con, size_t* bytes);
int scnattn_ensemble_layout_con(int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                                const scnattn_search_options* opt, const scnattn_constraints* con, long* offsets);
int scnattn_ensemble_init_con(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                              const scnattn_search_options* opt, const scnattn_constraints* con, const scnattn_params* w,
                              const float* enc, const float* const* tags, int start_token, float* ws);
int scnattn_ensemble_steps_con(void* stream, int M, const scnattn_dims* dims, int K, int max_steps, int alpha_member,
                               const scnattn_search_options* opt, const scnattn_constraints* con, const scnattn_params* w,
                               const float* enc, const float* member_w, int mode, int end_token, int t0, int n_steps,
                               float* ws);
int scnattn_beam_row_topk_con(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                              const int32_t* nsrc, const scnattn_search_options* opt, int end_token, int t,
                              const int32_t* hist, int max_steps, const int32_t* required, const int32_t* met, float* outv,
                              int32_t* outi, float* reqv, int32_t* reqi, int force_passes);
int scnattn_beam_row_topk_ens_con(void* stream, int N, int K, int V, int M, const float* const* logits, const long* ld,
                                  const float* w, int mode, const float* scores, const int32_t* nsrc,
                                  const scnattn_search_options* opt, int end_token, int t, const int32_t* hist,
                                  int max_steps, const int32_t* required, const int32_t* met, float* outv, int32_t* outi,
                                  float* reqv, int32_t* reqi, int force_passes);
int scnattn_beam_merge_banks(void* stream, int N, int K, int V, int end_token, int t, const float* candv, const int32_t* candi,
                             const float* reqv, const int32_t* reqi, const int32_t* required, int32_t* met,
                             void* const* state);
/* ---- sampled rollouts for self-critical training (csrc/rollout.hip, the driver beside the search's) ---------------------
 * The set-up and the decode step of the search above over the same N*K rows, but the K slots of an image are INDEPENDENT
 * captions: nothing is compacted, the state carries over slot for slot, and after fc one token per open row is picked:
 *   y_v = logits[row][v] * inv_temp,   key_v = y_v + noisy_j * g_v,   token = the first key under the TIE RULE (value
 *   descending, index ascending, compared as the fp32 numbers the kernel computes)
 *   noisy_j = 0 for slot 0 of every image when greedy_first != 0 (the arg-max caption), 1 otherwise
 *   g_v = -log(-log(u_v)), u_v = ((bits_v >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1)): Gumbel noise, so the pick is
 *   a draw from softmax(y)
 * THE RNG CONTRACT: bits_v is word (v & 3) of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (v >> 2, row, t, draw): a token's noise depends on (seed, draw, row, t, v) alone -- not on N, K, the launch geometry or
 * the chunking of the steps -- and numpy can restate it exactly.  draw is the caller's sequence number: one per rollout.
 *   logp = y_token - logsumexp(y): the log-probability under the distribution that was sampled (temperature included).
 * <end> closes a row: length[row] = t + 1 (0-based t), and the row's later records are token 0 (<pad>) / logp 0.0; a closed
 * slot keeps computing on finite values and is ignored.  A row that never produced <end> within max_steps is CUT OFF there:
 * its length stays 0 and all max_steps records are its tokens.  nsrc[n] for the attention kernels is K while any slot of
 * image n is open and 0 afterwards; then no kernel reads or writes the image's rows.
 * K in [1, 8], max_steps as for the search, inv_temp > 0 and finite, start / end tokens inside the vocabulary; a refusal
 * returns -1 before anything is launched.  want_alpha != 0 keeps the attention maps (the largest buffer; training does not
 * need them) and must be the same in the four calls.  fp32 only; dense encoder_out only.
 *   scnattn_rollout_layout offsets (in 4-byte elements from ws), in this order:
 *       0 open_rows int[1]   1 nsrc int[N]   2 nopen int[N] (open slots per image)   3 length int[N*K]   4 sum_logp f32[N*K]
 *       5 token int[max_steps][N*K]   6 logp f32[max_steps][N*K]   7 alpha f32[max_steps][N*K][P] (-1 unless asked for)
 *   scnattn_rollout_steps enqueues steps t0 .. t0+n_steps-1 (clipped to max_steps); steps on a finished batch are no-ops, so
 *       the host enqueues chunks and reads `open_rows` (one int) in between.  Per step it launches the search's decode part,
 *       then _pick and _advance: one launch fewer than a search step.
 * The two kernels alone (state: the seven pointers 0..6 of the layout above, token / logp holding max_steps steps):
 *   _pick     as above for step t; rows of an image with nsrc == 0 are neither read nor written
 *   _advance  emb[row] = table[clamp(token_t[row], 0, V-1)] for every row; nsrc[n] = nopen[n] > 0 ? K : 0 */
#define SCNATTN_ROLLOUT_NOFF 8
int scnattn_rollout_workspace(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes);
int scnattn_rollout_layout(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets);
int scnattn_rollout_init(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                         const float* enc, const float* tags, int start_token, float* ws);
int scnattn_rollout_steps(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                          const float* enc, int end_token, float inv_temp, uint64_t seed, uint32_t draw, int greedy_first,
                          int t0, int n_steps, float* ws);
int scnattn_rollout_pick(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, uint64_t seed,
                         uint32_t draw, int t, int greedy_first, int end_token, int max_steps, void* const* state);
int scnattn_rollout_advance(void* stream, int N, int K, int M, int V, const int32_t* token_t, const float* table, float* emb,
                            const int32_t* nopen, int32_t* nsrc);
/* ---- TRUNCATED sampling: top-k and nucleus (top-p) rollouts (csrc/rollout.hip: rollout_pick_filtered) ------
 * The reference has none of this; the semantics are this library's.  For an open row at step t, with y_v =
 * fl(logits[row][v] * inv_temp) (the fp32 number _pick forms) and the ORDER of the project (y descending, index ascending,
 * compared as fp32 numbers, so -0 == +0):
 *   THE FILTER   top_k >= 0 (0 or >= V: off), 0 < top_p <= 1 (1: off).  Anything else, NaN included, is refused (-1) before
 *                any launch.
 *   THE KEPT SET the first nkeep = min(L_k, L_p) words of the ORDER, where
 *                  L_k = top_k when 1 <= top_k < V, else V
 *                  L_p = the smallest L >= 1 with sum_{i<L} e_(i) >= top_p * sum_all e      ((i): along the ORDER)
 *                  e_v = expf(fl(y_v - m)), m = max y; a -inf logit has e_v = 0 exactly and sorts last
 *                top_p == 1 gives L_p = V without computing anything.  Both limits are measured on the FULL distribution
 *                (top-p is not re-applied to a renormalised top-k), and ties at the cut are broken by index.
 *                WHERE fp64 BEGINS: the terms e_v are fp32 (one fp32 subtraction, one expf); every sum of them, the product
 *                top_p * sum_all (top_p widened exactly), and the comparison are fp64.  The sums are taken in one fixed order
 *                that does not follow the ORDER (thread i of 256 adds its groups of four words q = i, i + 256, ..., words
 *                4q .. 4q + 3; lanes, then waves, are added in a fixed tree); among the words EQUAL to the value at the cut, which all carry the same e, the mass of
 *                the first j is A + j * e in fp64 (A: the fp64 mass of the words above that value).  An fp64 sum of at most
 *                2^20 fp32 terms is exact to 2^-32 relative, so the choice of order is invisible next to the terms' own error.
 *   THE DRAW     token = the first key in the ORDER among the kept words, key_v = y_v + noisy_j * g_v with exactly the noise
 *                of _pick (counter (v >> 2, row, t, draw)): the noise of word v does not depend on the filter, (seed, draw)
 *                repeats a rollout, and the Gumbel arg-max over the kept set is a draw from the truncated, renormalised
 *                softmax.  The arg-max slot (greedy_first, slot 0) picks the first word of the ORDER, inside every kept set.
 *   logp         = y_token - (m + log(sum_kept e)): the log-probability under the distribution that was sampled.
 *                WHERE fp64 ENDS: sum_kept (fp64 sum of the fp32 terms), its log, m + log(.) and the difference from y_token
 *                are fp64 (y_token and m widened exactly); the difference is rounded ONCE to fp32 and is the record.
 *                sum_logp accumulates the fp32 records in fp32, as _pick does.  top_k == 1 gives logp = +0.0 exactly.
 *   nkeep        a NEW RECORD int[max_steps][N*K]: nkeep of every open row and step; 0 for the records of a closed row of an
 *                open image (as token and logp get 0).
 *   DETERMINISM  the same inputs give the same bits from run to run and for any chunking of the steps: the reductions have a
 *                fixed order and no floating-point atomics.
 * Closed images, closed rows, <end> book-keeping, cut-off rows and the read-only nsrc are exactly those of _pick.  A row that
 * holds a NaN is OUTSIDE this contract (its nkeep, token and logp are unspecified); it still writes only its own records.
 * FILTER OFF (both limits off): the bits of the plain entry points in every buffer they share -- the plain kernel is
 * launched -- and nothing writes nkeep, which keeps the zeros _init_f put there.
 *   _workspace_f / _layout_f / _init_f / _steps_f   the four calls with the filter after want_alpha; the same filter in all
 *       four.  _layout_f writes SCNATTN_ROLLOUT_NOFF_F offsets: the 8 of scnattn_rollout_layout, then 8 nkeep
 *       int[max_steps][N*K].  The launches per step are those of the plain rollout: the pick runs in its filtered form.
 *   scnattn_rollout_pick_f   _pick with the filter; nkeep_t int[N*K] is the record of step t (refused when NULL while the
 *       filter is on); force_passes != 0 re-reads the row from global memory in every pass even when it fits the
 *       registers (the path of a V beyond 10240); both paths add the same numbers in the same order: the same bits. */
#define SCNATTN_ROLLOUT_NOFF_F 9
typedef struct {
    int32_t top_k;
    float top_p;
} scnattn_sample_filter;
int scnattn_rollout_workspace_f(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* filter,
                                size_t* bytes);
int scnattn_rollout_layout_f(const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_sample_filter* filter,
                             long* offsets);
int scnattn_rollout_init_f(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha,
                           const scnattn_sample_filter* filter, const scnattn_params* w, const float* enc, const float* tags,
                           int start_token, float* ws);
int scnattn_rollout_steps_f(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha,
                            const scnattn_sample_filter* filter, const scnattn_params* w, const float* enc, int end_token,
                            float inv_temp, uint64_t seed, uint32_t draw, int greedy_first, int t0, int n_steps, float* ws);
int scnattn_rollout_pick_f(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, uint64_t seed,
                           uint32_t draw, int t, int greedy_first, int end_token, int max_steps, void* const* state,
                           const scnattn_sample_filter* filter, int32_t* nkeep_t, int force_passes);
/* ---- SCORING given captions: teacher-forced log-probabilities (csrc/rollout.hip: rollout_score) -----------
 * The reference has none of this; the semantics are this library's.  The rollout's chain with the pick TOLD its token: row
 * r = n*K + j carries ntok[r] given tokens, target[t][r] at step t, and K captions of one image share the image-side set-up.
 *   OPEN AND CLOSED   a row is open at step t iff t < ntok[r].  A row of an image with nsrc[n] == 0 is neither read nor
 *                written.  A closed row of an open image gets the records token = 0, logp = 0.0, rank = 0, best = 0.
 *   QUANTITIES   y_v = fl(logits[row][v] * inv_temp), the fp32 number _pick forms, and the ORDER of the project (y
 *                descending, index ascending, compared as fp32 numbers, so -0 == +0).  A y of -0 is TAKEN AS +0 in the
 *                arithmetic below too (the kernel works on the order-preserving image of y, as the filtered pick does), so
 *                a row whose one finite logit is -0 gives logp = +0.0 like any other.
 *                  token = target                 so _advance works unchanged
 *                  best  = the first word of the ORDER (the lowest index among the maxima)
 *                  rank  = the number of words strictly before the target in the ORDER: those with a larger y and those
 *                          with an equal y and a lower index.  rank == 0 <=> best == target.
 *   logp         the arithmetic of the filtered pick with everything kept: m = max y; e_v = expf(fl(y_v - m)) in fp32, a
 *                -inf logit has e_v = 0 exactly; S = the fp64 sum of the e_v in one fixed order (thread i of 256 adds its
 *                groups of four words q = i, i + 256, ..., words 4q .. 4q + 3; lanes are then added as a butterfly, then
 *                the waves 0..3);  logp = (double)y_target - ((double)m + log(S)), rounded ONCE to fp32.  A -inf target
 *                gives -inf, a row with one finite logit +0.0.  sum_logp accumulates the fp32 records in fp32, as _pick
 *                does.  No floating-point atomics: the same inputs give the same bits, for any chunking of the steps.
 *   CLOSING      when t + 1 == ntok[r] the row closes: nopen[n] -= 1 and open_rows -= 1, as _pick closes a row on <end>.
 *                <end> itself is NOT special here: it is a token like any other, and a caption without <end> is scored as
 *                given.
 *   ODD INPUTS   a target outside [0, V) gives logp = NaN and rank = V (best is still the row's), writes only its own
 *                records, and _advance clamps the token.  A row that holds a NaN is OUTSIDE this contract; it still
 *                writes only its own records.
 * K in [1, 8], max_steps as for the search, inv_temp > 0 and finite, the start token inside the vocabulary; a refusal
 * returns -1 before anything is launched.  want_alpha as in the rollout: the maps are the attention of the given caption.
 * fp32 only; dense encoder_out only.
 *   _workspace_sc / _layout_sc   _layout_sc writes SCNATTN_ROLLOUT_NOFF_SC offsets: the 8 of scnattn_rollout_layout (3 length
 *       now holds ntok), then 8 rank int[max_steps][N*K], 9 best int[max_steps][N*K], 10 target int[max_steps][N*K].
 *   _init_sc   the captions as device pointers: targets int32 [N*K][ld_tok] row-major with ld_tok >= max_steps (the first
 *       max_steps entries of a row are read), ntok int32 [N*K], each in [0, max_steps] (clamped into it).  One kernel copies
 *       the captions into the workspace step-major and sets nopen[n] = #{j: ntok > 0}, nsrc[n] = nopen[n] > 0 ? K : 0,
 *       open_rows = sum of nopen, sum_logp = 0; then the set-up of _init.  Ragged input is allowed: a slot with ntok == 0 is
 *       empty, and an image whose slots are all empty is closed from the start.
 *   _steps_sc  steps t0 .. t0+n_steps-1 (clipped to max_steps): the search's decode part, _score, _advance -- the launches
 *       of a rollout step; chunks and the open_rows counter as in the rollout.
 *   scnattn_rollout_score   the kernel alone for step t (state: the seven pointers 0..6 of scnattn_rollout_layout, 3 holding
 *       ntok); target_t / rank_t / best_t int[N*K] are the given tokens and the records of that step. */
#define SCNATTN_ROLLOUT_NOFF_SC 11
int scnattn_rollout_workspace_sc(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes);
int scnattn_rollout_layout_sc(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets);
int scnattn_rollout_init_sc(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                            const float* enc, const float* tags, int start_token, const int32_t* targets, long ld_tok,
                            const int32_t* ntok, float* ws);
int scnattn_rollout_steps_sc(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                             const float* enc, float inv_temp, int t0, int n_steps, float* ws);
int scnattn_rollout_score(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, int t, int max_steps,
                          void* const* state, const int32_t* target_t, int32_t* rank_t, int32_t* best_t);
/* ---- SCHEDULED SAMPLING: gold and sampled input words mixed by a coin (csrc/rollout.hip: rollout_pick_mixed)
 * The reference has none of this; the semantics are this library's.  The scoring chain above with a pick that is TOLD the
 * gold word and flips a coin (Bengio et al. 2015): row r = n*K + j carries nmix[r] gold words, gold[t][r] at step t, and
 * token[t][r] -- the gold word or the model's own sample -- is the decoder's input at step t + 1.
 *   OPEN AND CLOSED   a row is open at step t iff t < nmix[r].  A row of an image with nsrc[n] == 0 is neither read nor
 *                written.  A closed row of an open image gets the records token = 0, sample = -1, logp = 0.0, replaced = 0.
 *   THE COIN     bits = word 0 of Philox4x32-10 with the rollout's key (seed & 0xffffffff, seed >> 32) and counter
 *                (0xFFFFFFFF, row, t, draw).  The first counter word of a word's noise is v >> 2 < 2^30, so the coin never
 *                shares a counter with it.  u = ((bits >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1));
 *                replaced = u < prob, compared in fp32.  prob == 0 never replaces, prob == 1 always does.  The decision
 *                depends on (seed, draw, row, t) alone -- not on V, N, K, prob's other rows or the chunking of the steps.
 *   NOT REPLACED the row's logits are not read.  token = gold, sample = -1, logp = 0.0, replaced = 0.
 *   REPLACED     the pick is _pick's, in its arithmetic and with its noise (counter (v >> 2, row, t, draw)):
 *                y_v = fl(logits[row][v] * inv_temp), key_v = fl(y_v + g_v), the first key under the TIE RULE, and
 *                logp = y_token - logsumexp(y) from the same pass.  greedy != 0: EVERY row takes the arg-max (key_v = y_v;
 *                there is no greedy_first here).  token = sample = the pick, logp, replaced = 1, and sum_logp[row] += logp
 *                in fp32.  At prob == 1 and greedy == 0 the tokens are _pick's for the same logits, (seed, draw, t) and K,
 *                bit for bit.
 *   CLOSING      when t + 1 == nmix[r] the row closes: nopen[n] -= 1 and open_rows -= 1, as _score closes a row.  <end> is
 *                NOT special: a sampled <end> becomes an input like any other word, and the gold length alone governs
 *                the row.
 *   ODD INPUTS   a gold word outside [0, V) is recorded as given; _advance clamps it.  A replaced row that holds a NaN is
 *                outside this contract, as in _pick; it still writes only its own records.
 * K in [1, 8], max_steps as for the search, inv_temp > 0 and finite, prob in [0, 1] (NaN refused), the start token inside
 * the vocabulary; a refusal returns -1 before anything is launched.  want_alpha as in the rollout: the maps are the attention
 * over the mixed inputs.  fp32 only; dense encoder_out only.
 *   _workspace_ss / _layout_ss   _layout_ss writes SCNATTN_ROLLOUT_NOFF_SS offsets: the 8 of scnattn_rollout_layout (3 length
 *       now holds nmix), then 8 sample int[max_steps][N*K], 9 replaced int[max_steps][N*K], 10 gold int[max_steps][N*K].
 *   _init_ss   the gold words as device pointers: gold int32 [N*K][ld_tok] row-major with ld_tok >= max_steps (the first
 *       max_steps entries of a row are read), nmix int32 [N*K], each in [0, max_steps] (clamped into it).  The kernel of
 *       _init_sc copies the words into the workspace step-major and sets the counters from nmix as it does from ntok; then
 *       the set-up of _init.  A slot with nmix == 0 is empty, and an image whose slots are all empty is closed from the
 *       start: nothing but the zero-fill of _init_ss touches its records.
 *   _steps_ss  steps t0 .. t0+n_steps-1 (clipped to max_steps): the search's decode part, _pick_mixed, _advance -- the
 *       launches of a rollout step; chunks and the open_rows counter as in the rollout.
 *   scnattn_rollout_pick_mixed   the kernel alone for step t (state: the seven pointers 0..6 of scnattn_rollout_layout, 3
 *       holding nmix); gold_t / sample_t / replaced_t int[N*K] are the gold words and the records of that step. */
#define SCNATTN_ROLLOUT_NOFF_SS 11
int scnattn_rollout_workspace_ss(const scnattn_dims* d, int K, int max_steps, int want_alpha, size_t* bytes);
int scnattn_rollout_layout_ss(const scnattn_dims* d, int K, int max_steps, int want_alpha, long* offsets);
int scnattn_rollout_init_ss(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                            const float* enc, const float* tags, int start_token, const int32_t* gold, long ld_tok,
                            const int32_t* nmix, float* ws);
int scnattn_rollout_steps_ss(void* stream, const scnattn_dims* d, int K, int max_steps, int want_alpha, const scnattn_params* w,
                             const float* enc, float inv_temp, float prob, uint64_t seed, uint32_t draw, int greedy, int t0,
                             int n_steps, float* ws);
int scnattn_rollout_pick_mixed(void* stream, int N, int K, int V, const float* logits, long ld, float inv_temp, float prob,
                               uint64_t seed, uint32_t draw, int t, int greedy, int max_steps, void* const* state,
                               const int32_t* gold_t, int32_t* sample_t, int32_t* replaced_t);
/* The kernels of a step (csrc/beam.hip), one launch each; nsrc int[N] on the device.
 *   _attn_scores   e[n*K+j][p] = w . relu(att1[n][p][:] + att2[n*K+j][:]) + b0 for j < nsrc[n] (other rows untouched)
 *   _attn_context  alpha_out [N*K][P], awe [N*K][E] (either may be NULL), z = sigmoid(gpre + gate_bias) * awe (gpre NULL: awe)
 *   _row_topk      outv / outi [N*K][K]: per live row the top K of scores[row] + logits[row][v] - logsumexp(logits[row]);
 *                  force_passes != 0 reads the row from global memory in every pass (the path of a V beyond the LDS)
 *   _merge         one step's selection for every image, on the state arrays a scnattn_beam_layout describes (state:
 *                  pointers in that order, entries 0..11); t = 0-based step whose token / parent rows are written
 *   _advance       hd / cd [N*K][D] = hs / cs [n*K + parent_t[row]], emb [N*K][M] = table[token_t[row]] */
int scnattn_beam_attn_scores(void* stream, int N, int K, int P, int A, const float* att1, const float* att2, int nslab,
                             long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                             const int32_t* nsrc, float* e);
int scnattn_beam_attn_context(void* stream, int N, int K, int P, int E, const float* enc, const float* e, const float* gpre,
                              int nslab, long slab_stride, long gpre_ld, const float* gate_bias, const int32_t* nsrc,
                              float* alpha_out, float* awe, float* z);
int scnattn_beam_row_topk(void* stream, int N, int K, int V, const float* logits, long ld, const float* scores,
                          const int32_t* nsrc, float* outv, int32_t* outi, int force_passes);
int scnattn_beam_merge(void* stream, int N, int K, int V, int end_token, int t, const float* candv, const int32_t* candi,
                       void* const* state);
int scnattn_beam_advance(void* stream, int N, int K, int D, int M, int V, const float* hs, const float* cs,
                         const int32_t* parent_t, const int32_t* token_t, const float* table, float* hd, float* cd,
                         float* emb);

/* ---- primitives (each = one kernel launch); used by the stand-alone modules and the tests ------- */
/* C = alpha*op(A).op(B) + beta*C + bias[n]; rows with rowmask[m]==0 written as 0.  Replaces the
 * aten::mm / addmm calls behind nn.Linear and `@` on the path. */
int scnattn_sgemm(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A,
                  long lda, const float* B, long ldb, float beta, float* C, long ldc, const float* bias,
                  const float* rowmask, int batch, long strideA, long strideB, long strideC);
/* Same product with a caller-provided workspace of `ws_floats` floats for deterministic split-K partial sums:
 * when the 128x128 tile grid alone cannot fill the chip (few rows: beam search, batch-4 configurations) the K
 * range is divided over up to 16 workgroups per tile and reduced in a fixed order by a second launch.  ws may
 * be NULL (then identical to scnattn_sgemm).  The workspace must not be shared by calls on different streams. */
int scnattn_sgemm_ws(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A,
                     long lda, const float* B, long ldb, float beta, float* C, long ldc, const float* bias,
                     const float* rowmask, int batch, long strideA, long strideB, long strideC, float* ws,
                     long ws_floats);
/* Y[s][g][r][n] = sum_{k in slice s} X[r][g*xg+k] * W[g*wg + k*ldw + n]; ksplit<=0 picks one.
 * Returns the ksplit used through *ksplit_out. */
int scnattn_skinny_gemm(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                        const float* W, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                        int ksplit, int* ksplit_out);
/* Mixed precision (BASELINE configs[4]): the same product with the weight matrix stored as bf16 (raw 16-bit elements,
 * ldw / wg in elements), widened to fp32 in registers, fp32 accumulation.  scnattn_f32_to_bf16 makes such a copy
 * (round to nearest even; n % 4 == 0).  The sequence drivers use both when option "decoder_bf16" is 1: the operands
 * the recurrence streams every step (recurrent weights, att1, the encoder map) are then read as bf16 copies made once
 * per call; softmax, LSTM state, master weights and every gradient stay fp32. */
int scnattn_skinny_gemm_bf16w(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                              const void* W_bf16, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                              int ksplit, int* ksplit_out);
/* ... and with the activation rows rounded to bf16 in registers as well: v_mfma_f32_32x32x16_bf16, fp32 accumulation
 * (option "decoder_bf16" = 2 selects it inside the sequence drivers) */
int scnattn_skinny_gemm_bf16(void* stream, int rows, int N, int K, int groups, const float* X, long ldx, long xg,
                             const void* W_bf16, long ldw, long wg, float* Y, long ldy, long yg, long yslab,
                             int ksplit, int* ksplit_out);
int scnattn_f32_to_bf16(void* stream, long n, const float* in, void* out);

/* models/attention.py:37-39 */
int scnattn_attn_scores(void* stream, int rows, int P, int A, const float* att1, const float* att2, int nslab,
                        long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                        float* e, float* att2_out);
/* models/attention.py:40-42 (+ gate of attention_scn.py:147-148 when gpre != NULL) */
int scnattn_attn_context(void* stream, int rows, int P, int E, const float* enc, const float* e,
                         const float* gpre, int nslab, long slab_stride, long gpre_ld, const float* gate_bias,
                         float* alpha_out, long alpha_ld, float* alpha_save, float* awe, float* gate, float* z);
int scnattn_mean_pixels(void* stream, int rows, int P, int E, const float* enc, float* out);
int scnattn_attn_dalpha(void* stream, int rows, int P, int E, const float* enc, const float* dawe,
                        const float* dalpha_in, long dalpha_in_ld, float* dalpha);
int scnattn_attn_softmax_bwd(void* stream, int rows, int P, int A, const float* att1, const float* att2,
                             const float* w, const float* alpha, const float* dalpha, float* de, float* datt2,
                             long datt2_ld);
int scnattn_attn_datt1_post_blocks(int B, int P);
int scnattn_attn_datt1_post(void* stream, int B, int P, int A, int T, const int32_t* dl, const float* att1,
                            const float* att2_all, const float* de_all, const float* w, float* datt1,
                            float* dwpart);
/* The same five with the streamed operand (att1 / enc) stored as bf16 (raw 16-bit elements, dimensions in elements), widened
 * to fp32 in registers: what the sequence drivers launch under option "decoder_bf16".  Everything else stays fp32. */
int scnattn_attn_scores_bf16(void* stream, int rows, int P, int A, const void* att1_bf16, const float* att2, int nslab,
                             long slab_stride, long att2_ld, const float* dec_bias, const float* w, const float* b0,
                             float* e, float* att2_out);
int scnattn_attn_context_bf16(void* stream, int rows, int P, int E, const void* enc_bf16, const float* e,
                              const float* gpre, int nslab, long slab_stride, long gpre_ld, const float* gate_bias,
                              float* alpha_out, long alpha_ld, float* alpha_save, float* awe, float* gate, float* z);
int scnattn_attn_dalpha_bf16(void* stream, int rows, int P, int E, const void* enc_bf16, const float* dawe,
                             const float* dalpha_in, long dalpha_in_ld, float* dalpha);
int scnattn_attn_softmax_bwd_bf16(void* stream, int rows, int P, int A, const void* att1_bf16, const float* att2,
                                  const float* w, const float* alpha, const float* dalpha, float* de, float* datt2,
                                  long datt2_ld);
int scnattn_attn_datt1_post_bf16(void* stream, int B, int P, int A, int T, const int32_t* dl, const void* att1_bf16,
                                 const float* att2_all, const float* de_all, const float* w, float* datt1,
                                 float* dwpart);
/* The kernels of the pooled path (scnattn_pool above), one launch each.  Every entry that takes a descriptor returns -1 for
 * Q <= 0, qtap_max outside 1..64 or a null table before anything is launched.  bf16 != 0: x / att1 holds bf16 elements.
 *   _attn_context_pooled      x [rows][Q][E]; alpha = softmax(e) over the P pooled pixels (alpha_out / alpha_save),
 *                             alphaq[q] = sum_k qtap_w[q][k] * alpha[qtap_idx[q][k]] (alphaq_save [rows][Q], may be NULL),
 *                             awe = sum_q alphaq[q] * x[q]; gate / z as scnattn_attn_context.  Any E (no multiple of 4 needed).
 *   _attn_softmax_bwd_pooled  dalpha[p] = dalpha_in[p] (may be NULL; row stride dalpha_in_ld) +
 *                             sum_k tap_w[p][k] * dalphaq[tap_idx[p][k]], dalphaq [rows][Q], Q <= 1024; then as
 *                             scnattn_attn_softmax_bwd
 *   _weighted_rows            out[b][:] = sum_q wts[q] * x[b][q][:]   (x [rows][Q][E], wts [Q])
 *   _pool_expand              out[b][p][:] = sum_k tap_w[p][k] * y[b][tap_idx[p][k]][:] + bias[:]   (y [B][Q][A], bias may be NULL)
 *   _pool_transpose           out[b][q][:] = sum over the live taps k of qtap_w[q][k] * in[b][qtap_idx[q][k]][:]   (in [B][P][A])
 *   _add_bcast_rows_w         out[b][q][:] += wts[q] * v[b][:]        (out [B][Q][E], v [B][E])
 * The last three need a width that is a multiple of 4 and 16-byte aligned operands, and return -1 otherwise. */
int scnattn_attn_context_pooled(void* stream, int rows, int P, int E, const void* x, int bf16, const scnattn_pool* pool,
                                const float* e, const float* gpre, int nslab, long slab_stride, long gpre_ld,
                                const float* gate_bias, float* alpha_out, long alpha_ld, float* alpha_save,
                                float* alphaq_save, float* awe, float* gate, float* z);
int scnattn_attn_softmax_bwd_pooled(void* stream, int rows, int P, int A, const void* att1, int bf16, const float* att2,
                                    const float* w, const float* alpha, const scnattn_pool* pool, const float* dalphaq,
                                    const float* dalpha_in, long dalpha_in_ld, float* de, float* datt2, long datt2_ld);
int scnattn_weighted_rows(void* stream, int rows, int Q, int E, const float* x, const float* wts, float* out);
int scnattn_pool_expand(void* stream, int B, int P, int A, const scnattn_pool* pool, const float* y, const float* bias,
                        float* out);
int scnattn_pool_transpose(void* stream, int B, int P, int A, const scnattn_pool* pool, const float* in, float* out);
int scnattn_add_bcast_rows_w(void* stream, int B, int Q, int E, const float* wts, const float* v, float* out);
/* models/scn_cell.py:73-91 / 134-144 element-wise parts */
int scnattn_scn_mix_fwd(void* stream, int rows, int F4, const float* pz, int pz_nslab, long pz_stride, long pz_ld,
                        const float* ex, const float* ph, int ph_nslab, long ph_stride, long ph_ld,
                        const float* qx, const float* qh, float* pa, float* phs, float* xcat);
/* models/scn_cell.py:146-152 */
int scnattn_lstm_fwd(void* stream, int rows, int H, const float* r, int nslab, long slab_stride, long r_ld,
                     long r_gate_stride, const float* bih, const float* bhh, const float* c_prev, float* gates,
                     float* c_new, float* h_new, float* tanhc);
int scnattn_lstm_bwd(void* stream, int rows, int rows_next, int H, const float* dh_fc, const float* dh_next,
                     int nslab, long slab_stride, long dh_ld, float* dc, const float* gates, const float* c_prev,
                     const float* tanhc, float* dr);
int scnattn_scn_mix_bwd(void* stream, int rows, int F4, const float* dxcat, int nslab, long slab_stride, long dx_ld,
                        long dx_gate_stride, const float* qx, const float* qh, const float* pa, const float* phs,
                        float* dpx, float* dph, long dph_ld, float* dqx_acc, float* dqh_acc);
int scnattn_gate_bwd(void* stream, int rows, int E, const float* dz, int nslab, long slab_stride, long dz_ld,
                     const float* awe, const float* gate, float* dawe, float* dgpre, long dgpre_ld);
/* helpers */
int scnattn_transpose2d(void* stream, int R, int C, const float* in, long ldi, float* out, long ldo);
int scnattn_colsum(void* stream, int R, int N, const float* X, long ld, float* out, float beta);
int scnattn_mul_bcast(void* stream, int T, int B, int N, const float* x, const float* q, float* out);
/* The sequence glue of scnattn_seq_fwd / scnattn_seq_bwd, each launcher alone.  Every entry returns -1 for a null operand or a
 * bad shape before anything is launched, and 0 without a launch for an empty problem.
 * gather:  out_tm[t][b][:] = table[caps[b][t]][:] (caps [B][L] int64, T <= L; a token outside [0, V) reads row 0 or V-1);
 * scatter: dtable[v][:] += sum over the cells (b, t < decode_lengths[b]) with caps[b][t] == v of demb_tm[t][b][:], in a fixed
 *          order; a token outside [0, V) is skipped; present [V] ints is a workspace (1 where the token occurs). */
int scnattn_gather_rows_tm(void* stream, int B, int T, int L, int M, const int64_t* caps, const float* table, int V,
                           float* out_tm);
int scnattn_scatter_add_rows_tm(void* stream, int B, int T, int L, int M, const int64_t* caps, const int32_t* decode_lengths,
                                const float* demb_tm, int V, float* dtable, int32_t* present);
/* out_bm[b][t][:] = t < decode_lengths[b] ? hs_tm[t][b][:] * mask_bm[b][t][:] : 0 (mask_bm may be NULL: no mask);
 * rowmask[b*T+t] = t < decode_lengths[b] (may be NULL).  hidden_from_bm is the same the other way round. */
int scnattn_hidden_to_bm(void* stream, int B, int T, int D, const int32_t* decode_lengths, const float* hs_tm,
                         const float* mask_bm, float* out_bm, float* rowmask);
int scnattn_hidden_from_bm(void* stream, int B, int T, int D, const int32_t* decode_lengths, const float* dbm,
                           const float* mask_bm, float* out_tm);
/* out[n] = beta*out[n] + sum over the rows with rowmask[r] != 0 of X[r][n]; a masked-out row is not summed whatever it holds,
 * and beta == 0 does not read out */
int scnattn_colsum_masked(void* stream, int R, int N, const float* X, long ld, const float* rowmask, float* out, float beta);
/* out[r][c] (dense [rows][N]) = sum over 1..16 slabs of slabs[s*slab_stride + r*slab_ld + c], in slab order */
int scnattn_reduce_slabs(void* stream, int rows, int N, const float* slabs, int nslab, long slab_stride, long slab_ld,
                         float* out);
int scnattn_copy2d(void* stream, int R, int C, const float* in, long ldi, float* out, long ldo);
/* x[b][p][e] += scale * v[b][e] (x dense [B][P][E], v dense [B][E]) */
int scnattn_add_bcast_rows(void* stream, int B, int P, int E, const float* v, float scale, float* x);
/* models/encoders/caption.py:41-43: AdaptiveAvgPool2d((Ho,Wo)) + permute(0,2,3,1); x given by strides */
int scnattn_pool_permute_fwd(void* stream, int B, int C, int Hin, int Win, int Ho, int Wo, const float* x,
                             long sxb, long sxc, long sxh, long sxw, float* y);
int scnattn_pool_permute_bwd(void* stream, int B, int C, int Hin, int Win, int Ho, int Wo, const float* dy,
                             float* dx, long sxb, long sxc, long sxh, long sxw);
/* The loss of the train step, trains/attention_scn.py:222-236, without materialising the packed batch:
 *   loss = mean over rows (b, t < decode_lengths[b]) of  logsumexp(scores[b,t,:]) - scores[b,t,targets[b,t]]
 *        + alpha_c * mean over (b,p) of (1 - sum_t alphas[b,t,p])^2            (alphas may be NULL)
 * scores [B,T,V]; targets int64 with row stride ldt (pass caps_sorted + 1, ldt = L: `targets = caps_sorted[:, 1:]`);
 * n_tokens = sum_b min(decode_lengths[b], T) (the row count of pack_padded_sequence(...).data).
 * Workspaces (kept for the backward): row_lse, row_loss [B*T], sm1 [B*P], reg_part [B]; loss [1].
 * bwd: grad_loss is the DEVICE scalar d/d loss; dscores [B,T,V] is written everywhere (0 for rows that were
 * not decoded), dalphas [B,T,P] likewise.  A target outside [0,V) (compared in 64 bits) makes the loss NaN instead of
 * faulting; its row of dscores is the softmax term without a one-hot. */
int scnattn_caption_loss_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                             long ldt, const int32_t* decode_lengths, long n_tokens, const float* alphas, float alpha_c,
                             float* row_lse, float* row_loss, float* sm1, float* reg_part, float* loss);
int scnattn_caption_loss_bwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                             long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_lse,
                             const float* sm1, float alpha_c, const float* grad_loss, float* dscores, float* dalphas);
/* scnattn_caption_loss_fwd with the caption loops' metrics counted in the same pass over the scores (the top-5 accuracy of
 * trains/attention_scn.py:255-257 / :338-339 and the arg-max hypotheses of :366-372); new symbol only, the version stays.
 * Elements of a row are ordered by (value descending, index ascending), the beam search's tie rule.  For a decoded row
 * r = b*T + t (t < decode_lengths[b]) with target tg:
 *   row_rank[r]       = #{v : x[v] > x[tg]} + #{v < tg : x[v] == x[tg]}: the target's position in that order, so the target
 *                       is among the top k exactly when row_rank[r] < k; INT32_MAX for a target outside [0,V) (never a hit;
 *                       the loss is NaN as above);
 *   preds[b*ldp + t]  = the index of the first element in that order: the arg-max, the lowest index among equal maxima.
 * A row that was not decoded gets row_rank = -1 and preds = 0, and its scores are not read.  hits[0] = #{0 <= row_rank < k},
 * hits[1] = #{row_rank == 0}: exact counts, so top-k accuracy in percent is hits[0] * (100 / n_tokens).  k > V is legal
 * (every decoded row with a valid target is a hit).  row_rank [B*T] is a workspace like row_lse; row_lse, row_loss and loss
 * hold the same bits as after scnattn_caption_loss_fwd, so scnattn_caption_loss_bwd runs on them unchanged.  k < 1,
 * ldp < T or a null output returns -1 before anything is launched.  With NaN scores the metrics are unspecified. */
int scnattn_caption_loss_metrics_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                     long ldt, const int32_t* decode_lengths, long n_tokens, const float* alphas,
                                     float alpha_c, float* row_lse, float* row_loss, float* sm1, float* reg_part,
                                     float* loss, int k, int32_t* row_rank, int32_t* preds, long ldp, int32_t* hits);
/* The reward-weighted loss of self-critical training: the pair above with row_weight [B] (device, fp32; the advantage of
 * each sampled caption, a constant: no gradient flows to it):
 *   loss = (1/n_tokens) * sum_b row_weight[b] * sum_{t < decode_lengths[b]} (logsumexp(scores[b,t,:]) - scores[b,t,tg])
 *        + alpha_c * (the regulariser above, unweighted)
 * The weight enters as ONE product per row -- row_loss[b,t] = nll * row_weight[b], and (grad_loss / n_tokens) *
 * row_weight[b] in front of the softmax term -- so weights of 1.0 give loss, row_lse, row_loss, dscores and dalphas with the
 * bits of the unweighted entry points (the same kernels; those pass no weights and multiply nothing).  row_lse is not
 * weighted.  The weight of a row with decode length 0 is not read.  New symbols only, the version stays. */
int scnattn_caption_loss_weighted_fwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                      long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_weight,
                                      const float* alphas, float alpha_c, float* row_lse, float* row_loss, float* sm1,
                                      float* reg_part, float* loss);
int scnattn_caption_loss_weighted_bwd(void* stream, int B, int T, int V, int P, const float* scores, const int64_t* targets,
                                      long ldt, const int32_t* decode_lengths, long n_tokens, const float* row_weight,
                                      const float* row_lse, const float* sm1, float alpha_c, const float* grad_loss,
                                      float* dscores, float* dalphas);
/* The head of the tagger step (models/encoders/tagger.py, trains/tagger.py:161-176) around its Linear layer.
 * The trunk map is addressed as x[b, q, c], q over the HW pixels, by ELEMENT strides sb / sp / sc; it holds fp32, or bf16
 * when bf16 != 0.  The channel-contiguous case (sc = 1, C and the other strides multiples of 16 bytes, aligned base) runs
 * on 16-byte accesses, anything else on the scalar form.
 *   tag_pool_fwd  pooled[b][c] (ldo) = (sum_q x[b,q,c]) / HW * ks[b][c] (ldk); ks = pre-scaled dropout keep mask or NULL
 *                 bf16 = 2: a bf16 map whose mean is rounded to bf16 (nearest even) before the mask, as
 *                 nn.AdaptiveAvgPool2d returns it for a bf16 map (the module path under bf16 autocast); pooled stays fp32
 *   tag_pool_bwd  dx[b,q,c] = dpooled[b][c] (ldd) * ks[b][c] / HW for every q, in the map's dtype (bf16: one round to
 *                 nearest even)
 *   bce_fwd       probs = 1 / (1 + expf(-z)); out[0] = mean over B*S of -(t * max(logf(p), -100) + (1 - t) *
 *                 max(log1pf(-p), -100)) (nn.BCELoss on nn.Sigmoid, evaluated at the rounded p, clamped before the
 *                 multiplication); out[1] = count of (p >= 0.5) == (t >= 0.5) (binary_accuracy's numerator, exact as a
 *                 float: B*S <= 2^24).  targets fp32 in [0, 1]; rows: workspace of 2*B floats (row sums, row counts).
 *   bce_bwd       dz = grad_loss[0] / (B*S) * (p - t) * p(1-p) / max(p(1-p), 1e-12) from the stored probs (grad_loss is
 *                 the DEVICE scalar d/d loss); exactly 0 where p saturated to 0 or 1.
 * Fixed summation order (bit-reproducible).  Every refusal returns -1 before anything is launched. */
int scnattn_tag_pool_fwd(void* stream, int B, int HW, int C, const void* x, int bf16, long sb, long sp, long sc,
                         const float* ks, long ldk, float* pooled, long ldo);
int scnattn_tag_pool_bwd(void* stream, int B, int HW, int C, const float* dpooled, long ldd, const float* ks, long ldk,
                         void* dx, int bf16, long sb, long sp, long sc);
int scnattn_bce_fwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt, float* probs,
                    long ldp, float* rows, float* out);
int scnattn_bce_bwd(void* stream, int B, int S, const float* probs, long ldp, const float* targets, long ldt,
                    const float* grad_loss, float* dz, long lddz);
/* Tagger losses for rare tags: the per-tag positive weight, the focal loss (Lin et al. 2017) and the asymmetric loss (Ridnik
 * et al. 2021) as ONE family of element-wise terms ON THE LOGITS, in the place of bce_fwd / bce_bwd.  The reference has none
 * (it trains under nn.BCELoss only); the semantics below are this library's own.
 * For a logit z, a target t in [0, 1] and a tag weight w_s >= 0 (pos_weight[s]; 1 when pos_weight is NULL), with
 * p = sigmoid(z), q = 1 - p and sp(x) = max(x, 0) + log1p(exp(-|x|))  (sp(z) = -log q, sp(-z) = -log p):
 *   term(z, t) = t * w_s * Lpos(z) + (1 - t) * Lneg(z)
 *   Lpos = (1 - p)^gamma_pos * (-log p)     = exp(-gamma_pos * sp(z)) * sp(-z)
 *   Lneg = p^gamma_neg * (-log(1 - p))      = exp(-gamma_neg * sp(-z)) * sp(z)                          margin = 0
 *   Lneg = p_m^gamma_neg * (-log1p(-p_m)),  p_m = max(p - margin, 0),  0^0 := 1                         margin > 0
 *   out[0] = sum(term) / (B * S)            (BCELoss's normaliser, so that the losses stay comparable)
 * and the derivative by the logit (q is formed as exp(-|z|) / (1 + exp(-|z|)) or 1 / (1 + exp(-|z|)), never as 1 - p):
 *   dLpos/dz = -exp(-gamma_pos * sp(z)) * (gamma_pos * p * sp(-z) + q)
 *   dLneg/dz =  exp(-gamma_neg * sp(-z)) * (gamma_neg * q * sp(z) + p)                                  margin = 0
 *   dLneg/dz =  [p > margin] * (gamma_neg * p_m^(gamma_neg - 1) * (-log1p(-p_m)) + p_m^gamma_neg / (1 - p_m)) * p * q
 *   dz       = grad_loss[0] / (B * S) * (t * w_s * dLpos/dz + (1 - t) * dLneg/dz)
 * Nothing is clamped at -100: at z = -120, t = 1 the term is w_s * 120 and dz = -w_s * grad_loss / (B * S), where the BCE
 * pair above has gradient 0.  (w, 0, 0, 0) is BCEWithLogitsLoss(pos_weight = w); gamma_pos = gamma_neg, margin 0 is the focal
 * loss with its alpha balance carried by w; (0, 4, 0.05) is the asymmetric loss's published default.
 *   tagloss_fwd   probs and out[1] (the agreement count) hold the bits bce_fwd writes for the same z and targets; rows:
 *                 workspace of 2*B floats (row sums, row counts); out[0] as above
 *   tagloss_bwd   reads the LOGITS, not the stored probs (a saturated p has lost what the gradient needs); grad_loss is the
 *                 DEVICE scalar d/d loss
 * Rows on 16-byte accesses when S % 4 == 0 and every base pointer (pos_weight included) and leading dimension allow it, the
 * scalar form otherwise.  Fixed summation order (bit-reproducible).  Refused with -1 before anything is launched: gamma_pos
 * or gamma_neg outside [0, 16] or not finite; margin outside [0, 1); margin > 0 together with 0 < gamma_neg < 1 (the gradient
 * is unbounded at p -> margin+); a null pointer other than pos_weight; B or S < 1, B*S > 2^24, a leading dimension below S. */
typedef struct scnattn_tag_loss_options {
    float gamma_pos, gamma_neg, margin;
} scnattn_tag_loss_options;
int scnattn_tagloss_fwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt,
                        const float* pos_weight, const scnattn_tag_loss_options* opt, float* probs, long ldp, float* rows,
                        float* out);
int scnattn_tagloss_bwd(void* stream, int B, int S, const float* z, long ldz, const float* targets, long ldt,
                        const float* pos_weight, const scnattn_tag_loss_options* opt, const float* grad_loss, float* dz,
                        long lddz);
/* Input assembly: replaces the per-sample host arithmetic of datasets/caption.py:51-53
 * (`torch.FloatTensor(imgs[i // cpi] / 255.)` + torchvision Normalize, trains/attention_scn.py:121-126).
 * src: n_src uint8 images [n_src][C][HW] in HBM (a staged batch or the whole dataset); idx: n_out int64
 * source rows on the device, or NULL for rows 0..n_out-1; lut: C*256 floats,
 * lut[c][v] = ((float)(v/255.0) - mean[c]) / std[c] computed by the caller with the reference's own
 * arithmetic, so the output is bit-identical to the reference's tensor.  dst: [n_out][C][HW]
 * (channels_last = 0) or [n_out][HW][C] (1), fp32 or bf16 (round-to-nearest-even of the fp32 value).
 * A row index outside [0, n_src) yields a NaN image instead of a fault. */
int scnattn_u8_gather_normalize(void* stream, const uint8_t* src, long n_src, const int64_t* idx, long n_out, int C,
                                long HW, const float* lut, void* dst, int dst_bf16, int channels_last);
/* Image augmentation in the same gather: random resized crop, horizontal flip, colour jitter.  The reference has none (it
 * feeds Normalize only) and torchvision's differ; the semantics below are this library's own.  Images are C = 3 planes
 * [N][3][H][W]; the output has the size of the source.
 *   scnattn_u8_mean_grey    per source image the exact integer byte sums SR, SG, SB of its planes (sums: int64 [N][3], or
 *                           NULL) and grey[i] = (0.299 SR + 0.587 SG + 0.114 SB) / (255 HW), formed in fp64 and rounded once
 *                           to fp32.  Once over a resident dataset, or per staged batch.
 *   scnattn_augment_draw    params[i] = (x0, y0, w, h, flip, bright, contr, sat), fp32 [n][8], a function of (seed, epoch,
 *                           sid[i]) alone.  Uniforms u_k = (word_k >> 8) * 2^-24 of Philox4x32-10 with key (seed &
 *                           0xffffffff, seed >> 32) and counter (q, sid & 0xffffffff, sid >> 32, epoch): q = 0 gives u0 area,
 *                           u1 aspect, u2 x offset, u3 y offset; q = 1 gives u4 flip, u5 brightness, u6 contrast, u7
 *                           saturation.
 *                             a = scale_lo + u0 (scale_hi - scale_lo)      r = exp(log ratio_lo + u1 (log ratio_hi - log ratio_lo))
 *                             w = min(W, W sqrt(a r))                      h = min(H, H sqrt(a / r))
 *                             x0 = u2 (W - w)     y0 = u3 (H - h)          flip = u4 < flip_p ? 1 : 0
 *                             bright / contr / sat = 1 + (2 u - 1) strength
 *                           No rejection loop, no integer rounding of the rectangle.  Evaluated in fp64 on the fp32 values of
 *                           cfg, each result rounded once to fp32.  Requires 0 < scale_lo <= scale_hi <= 1, 0 < ratio_lo <=
 *                           ratio_hi, flip_p and the strengths in [0, 1], epoch >= 0.
 *   scnattn_u8_gather_augment   row i of the output is image idx[i] (NULL: i) of src seen through params[i].  For output
 *                           pixel (oy, ox):
 *                             1. mirror: ox' = flip != 0 ? W - 1 - ox : ox
 *                             2. sx = clamp(x0 + (ox' + 0.5) (w / W) - 0.5, 0, W - 1), sy likewise from (y0, h, H, oy): the
 *                                half-pixel convention with border clamp of grid_sample(align_corners=False,
 *                                padding_mode="border"); magnification is >= 1 for a drawn record, so there is no antialias filter
 *                             3. v_c = bilinear blend of the four bytes around (sy, sx) (the right / lower neighbour index
 *                                clamped to the border), divided by 255
 *                             4. brightness: v_c = clamp(bright v_c, 0, 1)
 *                             5. contrast: m = min(1, bright grey[row]); v_c = clamp(contr v_c + (1 - contr) m, 0, 1); skipped
 *                                when grey is NULL.  grey is scnattn_u8_mean_grey of src (N entries): the mean of the SOURCE
 *                                image, not of the crop
 *                             6. saturation: g = 0.299 v_R + 0.587 v_G + 0.114 v_B; v_c = clamp(sat v_c + (1 - sat) g, 0, 1)
 *                             7. dst = (v_c - mean[c]) / std[c], fp32 or bf16 (round to nearest even), [n][3][H][W] or,
 *                                channels_last, [n][H][W][3]
 *                           fp32 arithmetic in that order.  mean, std: HOST arrays of 3 floats.  A row index outside [0, N)
 *                           yields a NaN image.  The coordinates are clamped whatever a record holds (NaN counts as 0), so a
 *                           hand-made table never reads outside its image.  The record (W, H crop, 0 flip, 1, 1, 1) is the
 *                           identity: ((byte / 255) - mean) / std with three roundings.
 * 1 <= H, W <= 16384.  Every refusal returns -1 before anything is launched. */
typedef struct scnattn_augment_config {
    float scale_lo, scale_hi;      /* crop area as a fraction of the image */
    float ratio_lo, ratio_hi;      /* aspect change of the crop, log-uniform */
    float flip_p;                  /* probability of the mirror */
    float brightness, contrast, saturation;      /* strengths: each factor is uniform in [1 - s, 1 + s] */
} scnattn_augment_config;
#define SCNATTN_AUGMENT_NPARAM 8
int scnattn_u8_mean_grey(void* stream, const uint8_t* src, long N, long HW, int64_t* sums, float* grey);
int scnattn_augment_draw(void* stream, long n, const int64_t* sid, int epoch, uint64_t seed, const scnattn_augment_config* cfg,
                         int H, int W, float* params);
int scnattn_u8_gather_augment(void* stream, const uint8_t* src, long N, const int64_t* idx, long n, int H, int W,
                              const float* params, const float* grey, const float* mean, const float* std, void* dst,
                              int dst_bf16, int channels_last);
/* Image resize of the inference path: replaces the host-side `scipy.misc.imresize(img, (OH, OW))` of inference.py:33-38
 * and utils/dataset.py:368-373, i.e. `PIL.Image.resize((OW, OH), BILINEAR)` on the uint8 image, the grey -> three planes
 * replication before it and the `transpose(2, 0, 1)` after it -- bit for bit: Pillow's 8-bit resize is integer
 * arithmetic (per pass clip8((2^21 + sum coeff * byte) >> 22), horizontal pass first, its result a uint8 before the
 * vertical pass reads it) on coefficient tables the host computes in double (scnattn.data.resize_taps).
 *   src      packed device buffer of src_bytes bytes holding N decoded images, each H x W x C interleaved uint8
 *   desc     one descriptor per image; desc_host is validated here, before the launch, desc_dev is the same array in
 *            device memory and is what the kernel reads (a device copy that disagrees skips the image, it never reads
 *            out of range)
 *   taps     device int32 buffer of taps_len words holding the axis tables.  A table of (in, out), in != out, is
 *            xmin[out], n[out], coeff[out][ksize] with ksize = 2 * ceil(max(in / out, 1)) + 1, in all
 *            scnattn_resize_table_ints(in, out) words; output i is clip8((2^21 + sum_{k < n[i]} coeff[i][k] *
 *            in[xmin[i] + k]) >> 22).  An axis with in == out has no pass and no table (tab_* is ignored).
 *   dst      dst_kind 0: uint8 [N][3][OH][OW] (channels_last must be 0);  1 / 2: fp32 / bf16 lut[c][byte], lut as for
 *            scnattn_u8_gather_normalize with C = 3, [N][3][OH][OW] or, channels_last, [N][OH][OW][3] -- the tensor
 *            scnattn_u8_gather_normalize writes from the uint8 rows.  A C == 1 image fills all three planes.
 * One launch for the whole batch.  1 <= H, W, OH, OW <= SCNATTN_RESIZE_MAX_DIM, N <= 65535.  Every refusal (C not 1 or
 * 3, a size out of range, a null pointer, an image or table that runs past its buffer) returns -1 with a message
 * before anything is launched.  scnattn_resize_table_ints returns -1 for a size out of range. */
#define SCNATTN_RESIZE_MAX_DIM 16384
typedef struct scnattn_image_desc {
    int64_t offset;      /* byte offset of the image in src */
    int32_t H, W, C;
    int32_t tab_h;       /* word offset in taps of the (W, OW) table */
    int32_t tab_v;       /* word offset in taps of the (H, OH) table */
    int32_t reserved;
} scnattn_image_desc;
long scnattn_resize_table_ints(int in_size, int out_size);
int scnattn_u8_resize_bilinear(void* stream, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                               const scnattn_image_desc* desc_dev, int N, const int32_t* taps, long taps_len, int OH,
                               int OW, const float* lut, void* dst, int dst_kind, int channels_last);
/* The same resize on tables of any filter (new symbols only, the version stays): scnattn.data.resize_taps(in, out,
 * filter="lanczos") is Pillow's `lanczos_filter` (support 3, negative weights), and the launch then gives
 * `PIL.Image.resize((OW, OH), LANCZOS)` byte for byte -- what utils/vizualize.py:26 shows under the attention maps.
 * Pillow's 8-bit arithmetic is the same for every filter; only the tables differ.  Source, descriptors, lut and dst are
 * as for scnattn_u8_resize_bilinear (which keeps its own table layout and ignores `reserved`, as this one does).
 *   taps     A table of (in, out), in != out, is  ksize, xmin[out], n[out], coeff[out][ksize]  -- 1 + out * (2 + ksize)
 *            words, tab_h / tab_v point at the header word ksize.  The row length is CARRIED, never re-derived from
 *            (in, out): Pillow computes it as (int)ceil(support * max(in / out, 1)) * 2 + 1 in double, which an integer
 *            formula need not reproduce for support 3.
 *   taps_host  the host copy of taps_dev (taps_len words each).  Checked before the launch, every row of every table
 *            the batch uses: 1 <= ksize <= 6 * SCNATTN_RESIZE_MAX_DIM + 1, 1 <= n <= ksize, xmin >= 0, xmin + n <= in,
 *            every |coeff| < 2^23 and sum |coeff| * 255 + 2^21 < 2^31 -- so the kernel's 24-bit multiplies and 32-bit
 *            sums are a checked precondition, not a property of one filter.  Any failure returns -1 with a message.
 * The kernel reads taps_dev only; a device copy that disagrees with the host copy skips the image or clamps the row, it
 * never reads out of range. */
int scnattn_u8_resize_taps(void* stream, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                           const scnattn_image_desc* desc_dev, int N, const int32_t* taps_host, const int32_t* taps_dev,
                           long taps_len, int OH, int OW, const float* lut, void* dst, int dst_kind, int channels_last);
/* Attention overlays (new symbols only, the version stays): the per-word pictures of utils/vizualize.py:38-48.  Each
 * h x w attention map is blown up and smoothed -- `skimage.transform.pyramid_expand(alpha, upscale, sigma)`, DEFINED here
 * as scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) followed by gaussian_filter(sigma, mode='reflect',
 * truncate=4.0); both are linear and separable, so S = Mv . a . Mh^T with the operators Mv [OH][h] and Mh [OW][w] the
 * caller builds in fp64 and uploads as fp32 (scnattn.viz.expand_operator; entries >= 0, rows sum to 1) -- and laid over
 * a photograph with a linear grey ramp.  fp32, fixed order, one fused multiply-add per term:
 *     U[i][X] = sum_j a[i][j] * Mh[X][j]  (j ascending),    S[Y][X] = sum_i Mv[Y][i] * U[i][X]  (i ascending);
 * a map whose entries are all equal is returned as that value (the exact result, the rows summing to 1).
 *   scnattn_attn_strips(OH)  strips of output rows a map is cut into; `partial` holds n_maps * strips * 2 floats
 *            (per strip min and max of S); -1 for OH out of range.
 *   scnattn_attn_expand   alphas [n_maps][h][w] -> S [n_maps][OH][OW] (may be NULL), lohi [n_maps][2] = {min, max} of S
 *            (may be NULL; exact, independent of order) and `partial`, which scnattn_attn_overlay reads.
 *   scnattn_attn_overlay  out [n_maps][OH][OW][3] uint8 from the same alphas / operators and the `partial` of
 *            scnattn_attn_expand.  S NULL: the maps are recomputed with the same code, bit for bit; S given: the maps
 *            scnattn_attn_expand stored are read back (the same bytes out, 4 * OH * OW bytes of memory per map more).  With {lo, hi} of map
 *            m, norm = hi > lo ? clamp((S - lo) / (hi - lo), 0, 1) : 0 and p = img[img_index[m]][c][Y][X],
 *                v = (1 - beta[m]) * p + (beta[m] * 255) * norm,   out = (uint8) clamp((int)(v + 0.5f), 0, 255),
 *            every operation a separately rounded fp32 one.  img: uint8 [n_img][3][OH][OW], the rows of the resize above;
 *            beta [n_maps] floats on the device; beta = 0 gives the photograph exactly.  img_index is validated on the
 *            host copy before the launch, the kernel reads the device copy and clamps it.
 * 1 <= h, w <= SCNATTN_OVERLAY_MAX_MAP, 1 <= OH, OW <= SCNATTN_OVERLAY_MAX_OUT, n_maps <= 65535, and the LDS a
 * workgroup needs, 4 * (h * w + 16 * h + OW * w) + 48 * OW bytes (each term rounded up to 16), at most 65280.  Every
 * refusal (a size out of range, a null pointer, an img_index out of range) returns -1 before anything is launched. */
#define SCNATTN_OVERLAY_MAX_MAP 32
#define SCNATTN_OVERLAY_MAX_OUT 1024
int scnattn_attn_strips(int OH);
int scnattn_attn_expand(void* stream, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh,
                        int OH, int OW, float* S, float* lohi, float* partial);
int scnattn_attn_overlay(void* stream, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh,
                         int OH, int OW, const float* S, const float* partial, const uint8_t* img, int n_img,
                         const int32_t* img_index_host, const int32_t* img_index_dev, const float* beta, uint8_t* out);
/* ---- caption text metrics over token ids (csrc/textmetrics.hip): what eval_caption.py:135-165 gets from NLGEval after the
 * beam search -- Bleu_1..4, ROUGE_L, CIDEr -- and the counting half of corpus BLEU in validate() ----------------------------
 * Inputs, all int32 on the device: hyp [N][Lh] with hyp_len [N]; ref [N][R][Lr] with ref_len [N][R], a NEGATIVE length marks
 * an absent reference slot.  skip_hyp / skip_ref are HOST arrays of 0..4 token ids; the kernel drops those ids from the
 * sequence (order kept) before anything else, and every length below is the length AFTER that.  Lengths read from memory are
 * clamped to [0, padded width], so a wrong length never indexes out of bounds.  1 <= Lh, Lr <= SCNATTN_TEXT_MAX_LEN,
 * 1 <= R <= SCNATTN_TEXT_MAX_REFS, N >= 0.  Token values are compared (and, for CIDEr-D, packed), never used as indices.
 *   scnattn_text_ngram_stats   stats int32 [N][10], exact:
 *        [n-1], n = 1..4   clipped matches: sum over the DISTINCT n-grams g of the hypothesis of
 *                          min(count of g in hyp, max over the present refs of count of g in that ref);
 *        [4 + n-1]         guesses max(0, len_hyp - n + 1);   [8] len_hyp;
 *        [9]               the present reference length closest to len_hyp, the shorter one on a tie; 0 when no slot is present.
 *   scnattn_text_lcs           lcs int32 [N][R]: length of the longest common subsequence of hyp and each ref (0 for an absent
 *        slot); score fp64 [N]: with P = max_r lcs/len_hyp, Rc = max_r lcs/len_ref (terms with a zero length left out) and
 *        beta = 1.2, (1 + beta^2) P Rc / (Rc + beta^2 P), and 0 when P or Rc is 0 (pycocoevalcap's Rouge).  mean (may be
 *        NULL): one fp64, the mean of score[0..N) summed in a fixed order (0 for N = 0).
 *   scnattn_text_ref_keys      keys int64 [N][R][Lr] for ONE order n in 1..4: at [i][r][j] the n-gram starting at position j of
 *        reference r of image i, its tokens t_0..t_{n-1} packed as sum t_k << 16k -- exact, no hashing -- or the sentinel -1
 *        where no n-gram starts there, the slot is absent, or the same n-gram stands earlier in image i's references: every
 *        image emits each of its n-grams once, so sorting the keys and counting runs gives the document frequencies.
 *        Tokens must lie in 0..SCNATTN_TEXT_CIDER_MAX_TOKEN (65534), which keeps 0xffff out of every field and the sentinel
 *        apart from every real key; a token outside sets *flag (int32 on the device, cleared by the call) to 1.
 *   scnattn_text_cider         score fp64 [N], CIDEr-D with n = 1..4, sigma = 6, x10 (pycocoevalcap's Cider).  The table: per
 *        order n the unique keys ascending AS SIGNED int64 with their df, the four orders one after the other in table_keys /
 *        table_df (device), order n at [table_off[n-1], table_off[n]) (table_off: HOST, 5 entries, [0] = 0).  Per order, the
 *        weight of a distinct n-gram g of a sentence is tf(g) * (log n_images - log max(1, df(g))); with h, r the weight
 *        vectors of the hypothesis and one reference, val_n = sum_g min(h_g, r_g) r_g, divided by |h| |r| when that is non-zero,
 *        times exp(-(len_hyp - len_ref)^2 / (2 sigma^2)); score = 10 * (sum_n (sum_refs val_n) / 4) / (present refs), 0 when
 *        none is present.  All of it in fp64, sums in a fixed order.  n_images = 1 gives exactly 0.  flag as above; mean as
 *        for scnattn_text_lcs.
 * Every refusal (a null pointer, N < 0, R or a padded width out of range, more than four skip ids, n outside 1..4, a table
 * that is not ascending) returns -1 before anything touches the GPU. */
#define SCNATTN_TEXT_MAX_LEN 128
#define SCNATTN_TEXT_MAX_REFS 32
#define SCNATTN_TEXT_CIDER_MAX_TOKEN 65534
int scnattn_text_max_len(void);
int scnattn_text_ngram_stats(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                             int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                             int n_skip_ref, int32_t* stats);
int scnattn_text_lcs(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref, int Lr,
                     const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref, int n_skip_ref,
                     int32_t* lcs, double* score, double* mean);
int scnattn_text_ref_keys(void* stream, int n, int N, int R, const int32_t* ref, int Lr, const int32_t* ref_len,
                          const int32_t* skip_ref, int n_skip_ref, int64_t* keys, int32_t* flag);
int scnattn_text_cider(void* stream, int N, int R, const int32_t* hyp, int Lh, const int32_t* hyp_len, const int32_t* ref,
                       int Lr, const int32_t* ref_len, const int32_t* skip_hyp, int n_skip_hyp, const int32_t* skip_ref,
                       int n_skip_ref, const int64_t* table_keys, const int32_t* table_df, const long* table_off, long n_images,
                       double* score, double* mean, int32_t* flag);
/* ---- tagger evaluation over tag probabilities (csrc/tagmetrics.hip; new symbols only, the version stays): ranking and
 * per-class measures next to the reference's binary_accuracy, which an all-zero tagger passes at about 99 % ----------------
 * Inputs: probs fp32 [B][S] (row stride ld_probs >= S), targets fp32 or uint8 [B][S] (row stride ld_targets >= S, in
 * elements), on the device.  An entry is POSITIVE iff target >= 0.5 (binary_accuracy's convention; for uint8: non-zero).
 * Scores must be finite and in [0, 1]: any other value sets *flag (int32 on the device; the calls only ever set it, the caller
 * clears it) and the results are then unspecified.  Every comparison is an IEEE fp32 comparison of the stored values.
 * AVERAGE PRECISION, tie-invariant counting form: for scores s with labels t and m >= 1 positives
 *        AP = (1/m) * sum over positive i of TP(i) / N(i),   N(i) = #{j : s_j >= s_i},   TP(i) = #{j positive : s_j >= s_i}.
 *   Both counts are exact integers, each quotient is one fp64 division, the sum is fp64 in ascending i, then one division by
 *   m.  The value does not depend on how ties are ordered: sklearn's average_precision_score of a column, and (0 < m < S)
 *   label_ranking_average_precision_score of a row.  m = 0 gives AP = 0 and the row / tag is left out of every mean.
 * PER IMAGE (row): AP, npos, and hits@k for nk <= SCNATTN_TAG_MAX_K values of k (HOST array, each >= 1, clamped to S): the
 *   number of positives among the top k, where entry i is in the top k iff #{j : s_j > s_i} + #{j < i : s_j == s_i} < k (ties
 *   go to the lower index).  precision@k = hits / k (the clamped k), recall@k = hits / npos.
 * PER TAG (column) over the n images stored: AP, npos, and for nt <= SCNATTN_TAG_MAX_THRESHOLDS thresholds (HOST fp32 array)
 *   the counts tp, fp, fn with the prediction p >= threshold; agree = #{(p >= 0.5) == positive}.
 *   scnattn_tag_store_size  bytes of the tag-major store of the caller: scores fp32 [S][cap], labels uint8 [S][cap].
 *   scnattn_tag_rows        one batch: writes row_ap fp64 [cap], row_npos int32 [cap], row_hits int32 [cap][nk] at rows
 *        row0 .. row0 + B - 1 and appends the batch to the store at the same columns.  Never synchronises.
 *   scnattn_tag_cols        over store columns 0 .. n - 1: col_ap fp64 [S], col_npos int32 [S], col_counts int32 [S][nt][3]
 *        (tp, fp, fn), col_agree int32 [S].
 *   scnattn_tag_finalize    summary fp64 [SCNATTN_TAG_SUMMARY_LEN]:
 *        [0] mean AP over the tags with a positive;  [1] mean AP over the images with a positive;
 *        [2 + q] mean precision@k_q and [6 + q] mean recall@k_q over the images with a positive, q < nk;
 *        [10 + 6 t ..] per threshold t < nt: micro P, R, F1 from the counts summed over tags, then macro P, R, F1 = means of
 *        the per-tag values over the tags with a positive; P = tp / (tp + fp), R = tp / (tp + fn), F1 = 2 tp / (2 tp + fp +
 *        fn), a 0 / 0 quotient counts as 0 (sklearn's zero_division = 0);
 *        [58] binary_accuracy = 100 * agree / (n * S);  [59] n;  [60] images without a positive;  [61] tags without a
 *        positive;  [62] *flag;  the rest 0.  A mean over nothing is NaN.  Every mean is summed in index order.
 * Every floating-point sum has one fixed order and there is no floating-point atomic: results are the same bits from run to
 * run and however the same images, in the same order, are split into batches.  Micro-averaged AP over all n * S entries is
 * not computed (in counting form it costs #positives * n * S).  Refused with -1 before anything is launched: a null pointer,
 * S outside 1..SCNATTN_TAG_MAX_S, cap outside 1..SCNATTN_TAG_MAX_IMAGES, row0 + B > cap or n > cap, n < 1, a leading
 * dimension below S, more than 4 values of k or one below 1, more than 8 thresholds. */
#define SCNATTN_TAG_MAX_S 4096
#define SCNATTN_TAG_MAX_K 4
#define SCNATTN_TAG_MAX_THRESHOLDS 8
#define SCNATTN_TAG_MAX_IMAGES 1073741824L
#define SCNATTN_TAG_SUMMARY_LEN 64
int scnattn_tag_store_size(int S, long cap, size_t* score_bytes, size_t* label_bytes);
int scnattn_tag_rows(void* stream, int B, int S, const float* probs, long ld_probs, const void* targets, int targets_u8,
                     long ld_targets, long row0, long cap, const int32_t* ks, int nk, float* store_scores, uint8_t* store_labels,
                     double* row_ap, int32_t* row_npos, int32_t* row_hits, int32_t* flag);
int scnattn_tag_cols(void* stream, int S, long n, long cap, const float* store_scores, const uint8_t* store_labels,
                     const float* thresholds, int nt, double* col_ap, int32_t* col_npos, int32_t* col_counts,
                     int32_t* col_agree);
int scnattn_tag_finalize(void* stream, int S, long n, const int32_t* ks, int nk, int nt, const double* row_ap,
                         const int32_t* row_npos, const int32_t* row_hits, const double* col_ap, const int32_t* col_npos,
                         const int32_t* col_counts, const int32_t* col_agree, const int32_t* flag, double* summary);
/* Fused BatchNorm2d (+ residual) (+ ReLU) on channels-last maps viewed as [R = N*H*W, C] (C % 4 == 0):
 * the `bn -> relu` / `bn -> (+identity) -> relu` groups of torchvision's Bottleneck behind
 * models/encoders/caption.py:17-22.  `partial` needs scnattn_bn_workspace_floats(C) floats.
 *   bn_stats : batch mean / 1/sqrt(var+eps) per channel (+ running-stat update with `momentum`)
 *   bn_apply : y = relu?(gamma*(z-mean)*invstd + beta + res?)
 *   bn_bwd   : dbeta, dgamma, dz (batch-stat form when train != 0) and dres = dy*[y>0] */
int scnattn_bn_workspace_floats(int C);
/* bf16 != 0: the feature maps (x, z, res, y, dy, dz, dres) are bf16 in memory (trunk under bf16 autocast,
 * BASELINE config 5); statistics, parameters and arithmetic stay fp32. */
int scnattn_bn_stats(void* stream, int R, int C, const void* x, int bf16, float eps, float momentum, float* partial,
                     float* mean, float* invstd, float* run_mean, float* run_var);
int scnattn_bn_apply(void* stream, int R, int C, const void* z, const void* res, int bf16, const float* mean,
                     const float* invstd, const float* gamma, const float* beta, int relu, void* y);
/* relu != 0: the mask is [y > 0]; with y == NULL and beta given it is recomputed from z with the forward's own
 * expression fma((z-mean)*invstd, gamma, beta) > 0 (only valid when no residual was added before the ReLU) and
 * the backward pass never reads y. */
int scnattn_bn_bwd(void* stream, int R, int C, const void* dy, const void* y, const void* z, int bf16,
                   const float* mean, const float* invstd, const float* gamma, const float* beta, int relu, int train,
                   float* partial, float* dbeta, float* dgamma, void* dz, void* dres);
/* ---- 1x1 convolutions of the ResNet-152 trunk as fused GEMMs (csrc/cgemm.hip) --------------------------------
 * Replaces the `nn.Conv2d(kernel_size=1)` layers of torchvision's Bottleneck (conv1, conv3, downsample.0) behind
 * models/encoders/caption.py:17-22 -- forward, d input, d weight -- on channels-last maps, where such a convolution
 * is the product [R = N*Ho*Wo, Cin] x [Cin, Cout], together with the BatchNorm work that can ride on it:
 *   pro_ss [Cin][2] = {scale, shift} (fwd, wgrad): the input operand is taken as relu(x * scale[c] + shift[c]) --
 *       the previous BatchNorm + ReLU folded to one fma per element (scale = gamma*invstd, shift = beta - mean*scale,
 *       written interleaved by scnattn_bn_finalize) -- so the normalised map is never written to or read from HBM;
 *   stat_partial [2][Cout][scnattn_cgemm_stat_ld(R)] (fwd; channel-major): per output channel and 64-row block, sum(y - s)
 *       and sum((y - s)^2) with s = stat_shift[c] (or 0): the statistics pass of the NEXT BatchNorm, fixed order;
 *   ez / emean / einvstd / egamma / ebeta (dgrad): the result is masked with the ReLU mask recomputed from the
 *       BatchNorm input z ([R][Cin], leading dimension ldz), g = dx * [fma((z-mean)*invstd, gamma, beta) > 0] -- or,
 *       when pro_ss is given, * [fma(z, scale, shift) > 0], bit for bit the mask of what a forward prologue computed --
 *       and stat_partial receives sum(g), sum(g * xhat): the two reductions of that BatchNorm's backward pass.
 * stride > 1 (downsample.0): input rows are gathered / scattered at (n, ho*stride, wo*stride) of an Hi x Wi map.
 * ws / ws_floats: split-K partial sums (shapes whose 128x128 tile grid cannot fill the chip); may be NULL. */
typedef struct scnattn_conv_extra {
    int pro;                  /* 0 none, 1: A operand prologue (per k), 2: B operand prologue (per n) */
    int epi;                  /* 0 plain, 1: statistics of the output, 2: ReLU mask from z + BatchNorm-backward sums */
    const float* pro_ss;
    float* stat_partial; const float* stat_shift;
    const float* ez; const float* emean; const float* einvstd; const float* egamma; const float* ebeta; long ldz;
    int stride, Hi, Wi, Ho, Wo;
    int force_split;          /* > 0: force the split-K factor (tests, tuning) */
    int force_mi;             /* 1 / 2: force the 64- / 128-row tile (tests, tuning) */
} scnattn_conv_extra;
/* C = alpha*op(A).op(B) + beta*C + bias, rows with rowmask == 0 written as 0: same contract as scnattn_sgemm_ws, on
 * the LDS-DMA pipelined kernel; needs 16-byte aligned operands (returns -1 otherwise; scnattn_sgemm_ws picks the
 * kernel by itself).  ex may be NULL. */
int scnattn_cgemm(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, long lda,
                  const float* B, long ldb, float beta, float* C, long ldc, const float* bias, const float* rowmask,
                  int batch, long strideA, long strideB, long strideC, float* ws, long ws_floats,
                  const scnattn_conv_extra* ex);
int scnattn_cgemm_row_tiles(int M);
/* y [R][Cout] = f(x) . w^T, w [Cout][Cin] (a channels-last 1x1 conv weight); R = output rows */
int scnattn_conv1x1_fwd(void* stream, int R, int Cin, int Cout, const float* x, const float* w, float* y,
                        const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* dx [R][Cin] = dy [R][Cout] . w (+ beta * dx: the residual branch's gradient is accumulated in place).
 * w_transposed != 0: `w` is the weight already transposed to [Cin][Cout] (scnattn_transpose2d), which puts both
 * operands on the k-contiguous LDS image -- worth it when Cin is large and Cout small (conv1 of a bottleneck). */
int scnattn_conv1x1_dgrad(void* stream, int R, int Cin, int Cout, const float* dy, const float* w, int w_transposed,
                          float beta, float* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* dw [Cout][Cin] = dy^T . f(x) */
int scnattn_conv1x1_wgrad(void* stream, int R, int Cin, int Cout, const float* dy, const float* x, float* dw,
                          const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* 3x3 convolutions (padding 1, stride s) of the trunk -- conv2 of every Bottleneck -- as IMPLICIT GEMMs on the same
 * kernel: no im2col buffer; the nine taps are a walk over K (forward, d input) or a property of the column tile
 * (d weight); a tap that falls outside the image is a lane whose LDS-DMA offset is out of range, i.e. zeros.
 * x [N*Hi*Wi][Cin], y / dy [N*Ho*Wo][Cout] channels-last maps, w / dw [Cout][3][3][Cin] (a channels-last conv weight).
 * Cin, Cout multiples of 16.  ex may carry epi = 1 (fwd: statistics of y) or epi = 2 (dgrad: ReLU mask from z +
 * BatchNorm-backward sums). */
int scnattn_conv3x3_fwd(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* x,
                        const float* w, float* y, const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* d input of a stride-1 convolution: the nine taps (flipped) walk K */
int scnattn_conv3x3_dgrad(void* stream, int N, int Hi, int Wi, int Cin, int Cout, const float* dy, const float* w,
                          float* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* d input of a STRIDE-2 convolution (conv2 of layer2.0 / 3.0 / 4.0; Hi, Wi even): ONE launch whose grid.y runs over the
 * four parity classes (hi & 1, wi & 1) of d-input pixels; a class sees only the taps that reach it (1, 2, 2 or 4 of the
 * nine), so nothing is multiplied by the zeros a zero-inserted dy would carry.  dy [N*(Hi/2)*(Wi/2)][Cout]. */
int scnattn_conv3x3_dgrad_strided(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* dy,
                                  const float* w, float* dx, float* ws, long ws_floats);
/* d weight.  stride 1, Cin % 32 == 0, Cout % 32 == 0 (every identity Bottleneck of the trunk): the
 * HALO-STAGED kernel of csrc/conv3.hip -- a wave owns a 32 x 32 block of dw for all nine taps (nine accumulators), walks
 * output pixels strip by strip and reads each staged activation line at nine shifted LDS addresses, so an activation
 * byte is staged once instead of nine times; the four waves of a workgroup split K and meet in LDS; k_slices > 0 fixes
 * the workgroup-level K split (0: policy, ~512 workgroups), whose slabs (k_slices * |dw| floats in ws) a second launch
 * sums in slab order.  Otherwise (strided, or k_slices < 0): the gathered [K][M] x [K][N] form on scnattn_cgemm's
 * kernel (needs Cin % 128 == 0). */
int scnattn_conv3x3_wgrad(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* dy,
                          const float* x, float* dw, float* ws, long ws_floats, int k_slices);
/* ---- forward convolutions of an EVAL-mode trunk with the BatchNorm folded into the epilogue (csrc/cgemm.hip, EPI 3) ------
 * With running statistics a BatchNorm is the per-channel map z*scale + shift, scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale; the kernel forms scale / shift per output column from the module's own parameters and
 * buffers when it finishes a tile (nothing to precompute, nothing cached), so the pre-BatchNorm map z is never written:
 *     y [R][Cout] = act(conv(x, w) * scale + shift (+ res)),   act = ReLU when relu != 0, identity otherwise.
 * res (optional, NULL: none) is a [R][Cout] map with leading dimension ldres (16-byte aligned, ldres % 4 == 0,
 * ldres >= Cout) added before the activation: the residual of a Bottleneck's last convolution.  gamma / beta / mean /
 * var are [Cout] fp32 vectors (16-byte aligned).  Nothing is written to the running statistics.
 * ex (may be NULL) carries only geometry -- stride / Hi / Wi / Ho / Wo of a strided 1x1 (downsample) whose input rows are
 * gathered, as for scnattn_conv1x1_fwd -- and force_split / force_mi; a non-zero pro or epi is an error.  Split-K runs
 * only as the in-launch combine (at most the cgemm_combine_max slices; otherwise unsplit).  Cin, Cout multiples of 16.
 * scnattn_conv3x3_fwd_bn_eval: the 3x3 (pad 1, stride 1 or 2) forward of scnattn_conv3x3_fwd with the same epilogue,
 * x [N*Hi*Wi][Cin], w [Cout][3][3][Cin], y / res [N*Ho*Wo][Cout], Ho = (Hi-1)/stride + 1 (odd maps allowed). */
typedef struct scnattn_bn_eval {
    const float* gamma; const float* beta; const float* mean; const float* var; float eps;
    const float* res; long ldres;   /* optional residual added before the activation (NULL: none) */
    int relu;
} scnattn_bn_eval;
int scnattn_conv1x1_fwd_bn_eval(void* stream, int R, int Cin, int Cout, const float* x, const float* w, float* y,
                                const scnattn_bn_eval* bn, const scnattn_conv_extra* ex, float* ws, long ws_floats);
int scnattn_conv3x3_fwd_bn_eval(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const float* x,
                                const float* w, float* y, const scnattn_bn_eval* bn, const scnattn_conv_extra* ex,
                                float* ws, long ws_floats);
/* ---- the stem: conv1 7x7 / 2 / pad 3 (3 -> 64) -> BatchNorm -> ReLU -> MaxPool 3x3 / 2 / pad 1 (csrc/stem.hip) ----------
 * children 0..3 of the trunk behind models/encoders/caption.py:17-22; frozen in every configuration of the reference, so
 * forward only.  x is the (N,3,H,W) image batch in ANY memory format (element strides sn, sc, sh, sw), w the (64,3,7,7)
 * weight in any format (wn, wc, wh, ww).  scnattn_stem_conv7 writes z [N*Ho*Wo][64] (Ho = (H-1)/2+1) and, when
 * stat_partial is given, per-workgroup sums {sum(z - s), sum((z - s)^2)} [2][64][(scnattn_stem_tiles(N,H,W)+3)&~3] for
 * scnattn_bn_finalize (s = stat_shift[c] or 0).  scnattn_stem_bn_relu_maxpool: out [N*Hp*Wp][C] = max over the 3x3 window
 * of relu(z*scale[c] + shift[c]) with ss [C][2] = {scale, shift} (scnattn_bn_finalize's ss_out), Hp = (Hz-1)/2+1. */
int scnattn_stem_tiles(int N, int H, int W);
int scnattn_stem_conv7(void* stream, int N, int H, int W, const float* x, long sn, long sc, long sh, long sw,
                       const float* w, long wn, long wc, long wh, long ww, float* z, float* stat_partial,
                       const float* stat_shift);
int scnattn_stem_bn_relu_maxpool(void* stream, int N, int Hz, int Wz, int C, const float* z, const float* ss, void* out,
                                 int out_bf16);       /* out_bf16 != 0: the pooled map is written as bf16 (mixed-precision trunk) */
/* ---- BatchNorm statistics that ride on the convolutions, finalized ON LOAD (csrc/batchnorm.hip) --------------------------
 * The statistics epilogues above (and scnattn_stem_conv7, scnattn_bn_bwd_reduce, the dgrad mask pass) leave CHANNEL-MAJOR
 * partials  partial[2][C][ldp]:  entry (which, channel, chunk), ldp = chunk count rounded up to 4
 * (scnattn_cgemm_stat_ld(R) for a product of R rows: one chunk per 64 rows).  A dependent launch costs ~8-9 us on MI355X,
 * so the tiny per-BatchNorm `finalize` launches are folded into the element-wise kernel that consumes the statistics:
 * each of its workgroups owns 64 channels and sums their partial rows itself (fixed order: every workgroup gets the same
 * bits), the workgroups of the first row chunk also write the per-channel results.
 *   scnattn_bn_finalize    statistics only: mean, 1/sqrt(var+eps), running-stat update (momentum; run_* may be NULL) and,
 *                          when ss_out is given, the folded {scale = gamma*invstd, shift = beta - mean*scale} pairs [C][2]
 *                          for a consumer that normalises on load (conv3's prologue, the stem's pooling kernel);
 *   scnattn_bn_apply_fin   y = [relu](gamma*(z-mean)*invstd + beta [+ res]) with the same finalize inside;
 *                          partial holds {sum(z - s), sum((z - s)^2)}, s = shift[c] (NULL: 0).  `shift` must be the vector the
 *                          producer's epilogue used and must NOT alias run_mean (this kernel updates it while other
 *                          workgroups still read shift): callers pass the previous step's batch mean;
 *   scnattn_bn_bwd_reduce  relu != 0: g = dy * [y > 0] -> gout (may be NULL); relu == 0: g is dy itself, nothing is written
 *                          and gout must be NULL (refused otherwise); partial = {sum g, sum g*xhat};
 *                          *nchunk_out = chunk count (ldp = that rounded up to 4 <= ldp_cap);
 *   scnattn_bn_bwd_dx_fin  dz = gamma*invstd*(g - dbeta/R - xhat*dgamma/R) from an already masked g, dbeta = sum g and
 *                          dgamma = sum g*xhat summed from the partials inside (and written out as the parameter gradients). */
int scnattn_cgemm_stat_ld(int M);
int scnattn_bn_finalize(void* stream, long R, int C, const float* partial, int ldp, int nchunk, const float* shift,
                        float eps, float momentum, float* mean, float* invstd, float* run_mean, float* run_var,
                        const float* gamma, const float* beta, float* ss_out);
/* bf16 != 0: every MAP argument (z, res, y / dy, y, z, gout / g, z, dz) holds bf16 elements; statistics, partials and
 * parameters are fp32 either way */
int scnattn_bn_apply_fin(void* stream, long R, int C, const void* z, const void* res, int bf16, const float* partial, int ldp,
                         int nchunk, const float* shift, float eps, float momentum, const float* gamma, const float* beta,
                         int relu, void* y, float* mean, float* invstd, float* run_mean, float* run_var, float* ss_out);
int scnattn_bn_bwd_reduce(void* stream, int R, int C, const void* dy, const void* y, const void* z, int bf16, const float* mean,
                          const float* invstd, int relu, float* partial, int ldp_cap, void* gout, int* nchunk_out);
int scnattn_bn_bwd_dx_fin(void* stream, long R, int C, const void* g, const void* z, int bf16, const float* mean,
                          const float* invstd, const float* gamma, const float* partial, int ldp, int nchunk, float* dbeta,
                          float* dgamma, void* dz);

/* ---- mixed-precision trunk (BASELINE configs[4]): bf16 maps and operand copies, fp32 accumulation / statistics / master
 * weights / weight gradients (csrc/cgemm16.hip, csrc/wgrad16.hip) ------------------------------------------------------------
 * The same convolutions of torchvision's Bottleneck (models/encoders/caption.py:17-22) on v_mfma_f32_32x32x16_bf16.
 *   scnattn_bf16_weights   ONE launch per step: every convolution weight [Cout][taps][Cin] fp32 -> a bf16 copy in the same
 *                          layout (forward B operand) and a transposed bf16 copy [Cin][taps][Cout] (d-input B operand);
 *                          desc / tile_prefix are device arrays (tile_prefix[i] = number of 32 x 32 tiles of weights 0..i-1,
 *                          a weight has taps * Cout/32 * Cin/32 of them; Cout, Cin multiples of 32);
 *   scnattn_cgemm16        C[M][N] = A[M][K] . B[N][K]^T (+ beta*C): A, B bf16 k-contiguous, C bf16 (out_bf16) or fp32;
 *                          ex: epi 1 (statistics of C from the fp32 accumulators, channel-major partials), stride (row
 *                          gather of a strided 1x1 convolution); a 1x1 d input is this with B = the transposed copy;
 *   scnattn_conv3x3_fwd16 / _dgrad16   implicit GEMMs as in fp32 (taps over K; stride-2 d input by parity classes);
 *                          epi 2 (scnattn_cgemm16 with a bf16 output, and the stride-1 _dgrad16; ex->ez is then the consumer
 *                          BatchNorm's bf16 pre-activation): the ReLU mask recomputed with the forward pass's expression,
 *                          g stored, column sums of g and g*xhat as channel-major partials -- that BatchNorm's backward
 *                          reduce pass inside the d-input product (the product then runs un-split);
 *   scnattn_wgrad16_3x3    dw [Cout][3][3][Cin] fp32 of a stride-1 3x3 convolution from bf16 maps: contraction over pixels
 *                          with both operands read through the transposing LDS load (ds_read_b64_tr_b16), halo staged once;
 *   scnattn_wgrad16_rows   dw[co][ci] (ldo) = sum_r dy[r][co] * x[src(r)][ci]: 1x1 weight gradients (gs = 0), the strided
 *                          downsample (gs = stride, goh = gow = 0) and ONE TAP of a stride-2 3x3 (gs = 2, goh = dh - 1,
 *                          gow = dw - 1, dw offset by tap*Cin, ldo = 9*Cin); Cin, Cout multiples of 64. */
typedef struct scnattn_weight_desc {
    const float* src; void* dst; void* dst_t; int cout, taps, cin, pad;
} scnattn_weight_desc;
int scnattn_bf16_weights(void* stream, int n, const scnattn_weight_desc* desc, const int* tile_prefix, int total_tiles);
int scnattn_cgemm16(void* stream, int M, int N, int K, const void* A, long lda, const void* B, long ldb, float beta, void* C,
                    long ldc, int out_bf16, float* ws, long ws_floats, const scnattn_conv_extra* ex);
int scnattn_conv3x3_fwd16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* x, const void* w,
                          void* y, const scnattn_conv_extra* ex, float* ws, long ws_floats);
int scnattn_conv3x3_dgrad16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* dy, const void* wt,
                            void* dx, const scnattn_conv_extra* ex, float* ws, long ws_floats);
/* Forward convolutions of an EVAL-mode trunk on bf16 maps, the BatchNorm folded into the epilogue (csrc/cgemm16.hip, EPI 3):
 * scnattn_conv1x1_fwd_bn_eval / scnattn_conv3x3_fwd_bn_eval above with x, w, y and res bf16 -- what a Bottleneck computes
 * under torch.autocast("cuda", dtype=torch.bfloat16) after encoder.eval().
 *     y [R][Cout] = bf16(act(fma(conv(x, w), scale, shift) (+ res))),  scale = gamma / sqrt(var + eps), shift = beta - mean * scale
 * formed per output column from the four fp32 vectors (non-null, 16-byte aligned) at every call; accumulation and the epilogue
 * are fp32, the result is rounded once (to nearest even).  w is [Cout][Cin] (1x1) or [Cout][3][3][Cin] (3x3); res (NULL:
 * none) is a bf16 [R][Cout] map, 16-byte aligned, ldres % 8 == 0, ldres >= Cout, below 2 GB.  ex (may be NULL): geometry of
 * the gathered 1x1 (stride, Hi / Wi / Ho / Wo), force_split, force_mi; pro = epi = 0.  1x1: Cin, Cout multiples of 8;
 * 3x3: Cin a multiple of 32, Cout of 8, stride 1 or 2, odd maps allowed.  A split product (the policy of scnattn_cgemm16,
 * or force_split) writes fp32 slabs to ws and a second launch sums them in slab order and applies the same epilogue.
 * Every refusal returns -1 before anything is launched: y is untouched. */
typedef struct scnattn_bn_eval16 {
    const float* gamma; const float* beta; const float* mean; const float* var; float eps;
    const void* res; long ldres;   /* bf16 residual, elements; NULL: none */
    int relu;
} scnattn_bn_eval16;
int scnattn_conv1x1_fwd_bn_eval16(void* stream, int R, int Cin, int Cout, const void* x, const void* w, void* y,
                                  const scnattn_bn_eval16* bn, const scnattn_conv_extra* ex, float* ws, long ws_floats);
int scnattn_conv3x3_fwd_bn_eval16(void* stream, int N, int Hi, int Wi, int Cin, int Cout, int stride, const void* x,
                                  const void* w, void* y, const scnattn_bn_eval16* bn, const scnattn_conv_extra* ex,
                                  float* ws, long ws_floats);
int scnattn_wgrad16_3x3(void* stream, int N, int H, int W, int Cin, int Cout, const void* dy, const void* x, float* dw,
                        float* ws, long ws_floats, int k_slices);
int scnattn_wgrad16_rows(void* stream, int R, int Cin, int Cout, const void* dy, const void* x, long src_rows, float* dw,
                         long ldo, int gs, int gHi, int gWi, int gHo, int gWo, int goh, int gow, float* ws, long ws_floats,
                         int k_slices);
/* ---- one mixed-precision Bottleneck from ONE call per direction (csrc/block16.cpp) -------------------------------------------
 * torchvision's Bottleneck.forward (conv1-bn1-relu-conv2-bn2-relu-conv3-bn3 [+ downsample] + identity, relu; the blocks of the
 * trunk built at models/encoders/caption.py:17-22) and its gradient as the launch sequences above, enqueued by the library:
 * the bf16 step is bound by what the HOST spends per launch (~25 calls per block and direction from Python), not by the GPU.
 * The library still allocates nothing: the caller sizes three buffers with scnattn_block16_sizes and owns them.
 *   save  (bf16): z1 a1 | z2 a2 | z3 out | [zd idn]   -- everything the backward pass re-reads; `out` (the block's result,
 *                 [N*Ho*Wo][4p]) starts at out_offset elements;
 *   stats (fp32): [4][2][4p]  mean, invstd of bn1, bn2, bn3, downsample.1 (written by the forward call);
 *   tmp   (bf16, backward): dres dz3 | dz2 | dz1 | [dzd dx dxd];  dgb (fp32, backward): [4][2][4p]  d beta, d gamma.
 * BatchNorm index: 0 bn1, 1 bn2, 2 bn3, 3 downsample.1; convolution index: 0 conv1, 1 conv2, 2 conv3, 3 downsample.0.
 * shift[i]: conditioning shift of BatchNorm i (scnattn_bn_apply_fin); w / wt: the bf16 copies of scnattn_bf16_weights.
 * Backward: weight gradients with a non-null dw[i] are written there (fp32, the parameter's layout); with side_stream they run
 * on it, forked from `stream` by events (the caller joins it and keeps save / tmp / x alive until then).  dx_out receives the
 * gradient of the block input: for an identity block it is dres (accumulated in place); with a downsample the caller adds
 * dxd_out (the [N*Ho*Wo][Cin] gradient through downsample.0) into the strided rows of dx_out itself.  dx_out / dxd_out
 * receive NULL when need_dx == 0, dxd_out also for an identity block.
 * Scratch, in floats (Rin = N*Hi*Wi, Rout = N*Ho*Wo, ld = scnattn_cgemm_stat_ld):
 *   part, bnpart: 2 * max(p * ld(Rin), 4p * ld(Rout)) each (scnattn/block.py part_floats).  bnpart_floats is checked: the
 *                 forward call needs 2 * 4p * ld(Rout) of it with a downsample (nothing without), the backward call all of
 *                 it.  part has no size field: the caller guarantees it (forward only).
 *   ws (side_ws): the split workspace scnattn_cgemm16 / scnattn_wgrad16_* are given; their policies size the split to it.
 * Every refusal -- geometry (p, Cin multiples of 64; even maps at stride 2; an identity block keeps its shape), a null
 * buffer or parameter, a bnpart that is too small -- returns -1 before anything is launched: nothing is written. */
typedef struct scnattn_block16 {
    int N, Cin, Hi, Wi, p, stride, has_down, pad;
    const float* gamma[4]; const float* beta[4]; float* run_mean[4]; float* run_var[4]; const float* shift[4];
    float eps[4], momentum[4];
    const void* w[4]; const void* wt[4];
    float* ws; long ws_floats; float* part; float* bnpart; long bnpart_floats;
    const void* x; void* save; float* stats;
    /* backward only */
    const void* dout; void* tmp; float* dgb; float* dw[4]; int need_dx, pad2;
    void* side_stream; float* side_ws; long side_ws_floats;
} scnattn_block16;
int scnattn_block16_sizes(const scnattn_block16* b, long* save_elems, long* out_offset, long* stats_floats, long* tmp_elems,
                          long* dgb_floats);
int scnattn_block16_fwd(void* stream, const scnattn_block16* b);
int scnattn_block16_bwd(void* stream, const scnattn_block16* b, void** dx_out, void** dxd_out);
/* scnattn_bn_stats (fp32 maps) that also writes the folded {scale, shift} pairs [C][2] for a consumer's prologue */
int scnattn_bn_stats_fold(void* stream, int R, int C, const void* x, float eps, float momentum, float* partial,
                          float* mean, float* invstd, float* run_mean, float* run_var, const float* gamma,
                          const float* beta, float* ss_out);

/* ---- launch plans: what a dense product would launch, asked of the code that launches it ----------------------------------
 * Each of the seven host launchers behind the dense-product entry points (cgemm, cgemm16, sgemm_ws, skinny_gemm,
 * conv3x3_wgrad_halo, wgrad16_3x3, wgrad16_rows) checks its arguments, computes a plan -- a pure function of shapes, layout
 * and alignment facts, the scnattn_conv_extra selectors, the workspace size and the options -- and launches from that plan
 * alone.  scnattn_plan_next(out) arms the calling thread: the next call on it that reaches one of those launchers
 * (scnattn_sgemm(_ws), _cgemm, _cgemm16, _conv1x1_*, _conv3x3_*, the four _bn_eval(16) forms, _wgrad16_*, _skinny_gemm*) runs
 * its checks and its plan, fills *out, launches nothing, calls no HIP API, disarms and returns 0.  A refusal returns its
 * usual error and message, an empty problem 0; both disarm with out->family == 0.  scnattn_plan_next(NULL) disarms; a second
 * arming replaces the first.  scnattn_block16_* makes many launches per call and cannot be planned: it disarms and runs.
 * Fields a family does not use are 0. */
enum { SCNATTN_PLAN_NONE = 0, SCNATTN_PLAN_CGEMM, SCNATTN_PLAN_SGEMM, SCNATTN_PLAN_SKINNY, SCNATTN_PLAN_CGEMM16,
       SCNATTN_PLAN_CONV3_WGRAD, SCNATTN_PLAN_WGRAD16_W9, SCNATTN_PLAN_WGRAD16_W1 };
/* the launch that follows the product, if any */
enum { SCNATTN_SECOND_NONE = 0,
       SCNATTN_SECOND_CREDUCE,          /* creduce<vec>: sum of the slabs + the plain epilogue */
       SCNATTN_SECOND_CSTATS1,          /* cstats<1>: slab sum + column statistics */
       SCNATTN_SECOND_CSTATS2_SLABS,    /* cstats<2>: slab sum + mask epilogue */
       SCNATTN_SECOND_CSTATS2_C,        /* cstats<2> on the un-split product read back from C */
       SCNATTN_SECOND_CREDUCE16,        /* creduce16<out_bf16, second_mode>: 0 plain, 1 statistics, 2 eval BatchNorm */
       SCNATTN_SECOND_CGEMM_REDUCE,     /* creduce<1> over the slabs of a wave-split weight gradient */
       SCNATTN_SECOND_SPLITK_REDUCE };  /* sgemm's splitk_reduce */
typedef struct scnattn_launch_plan {
    int family;                 /* SCNATTN_PLAN_* */
    int mi;                     /* cgemm / cgemm16: row tile (1: 64 rows, 2: 128 rows, 4: 128 x 64) */
    int tA, tB;                 /* cgemm / sgemm: operand layouts as launched */
    int pro, epi;               /* prologue / epilogue of the product KERNEL (a split product's epilogue may move to `second`) */
    int gather, c3;             /* row gather of a strided 1x1 convolution; 3x3 mode */
    int vec;                    /* cgemm: 16-byte C stores; sgemm: 16-byte operand loads; skinny: XVEC */
    int out_bf16;               /* cgemm16 */
    int wbf;                    /* skinny: 0 fp32 weights, 1 bf16 weights, 2 bf16 matrix instruction */
    int nb, chunks, empty;      /* skinny: 8-k blocks per wave and chunk (NB), chunks per wave, empty K-slices */
    int kslice;                 /* skinny: k per slice */
    int seg;                    /* wave-split weight gradients: pixels per line (SEG of conv3_wgrad) */
    int Q, ntiles;              /* wave-split weight gradients: lines, output blocks */
    int S, kper;                /* K-slices and their length */
    int mt, nt;                 /* cgemm / cgemm16: tile grid */
    long tiles;                 /* output tiles (x batch) */
    int grid_x, grid_y, grid_z;
    int in_launch;              /* cgemm: the split product is finished inside the launch (arrival counters) */
    int second, second_mode;    /* SCNATTN_SECOND_* */
} scnattn_launch_plan;
int scnattn_plan_next(scnattn_launch_plan* out);

/* ---- data-parallel gradient exchange (the reference has no distributed code) ---------------------
 * One process per GPU.  RCCL SUM all-reduce of gradient buckets on a library-owned communication stream, ordered
 * against the caller's compute stream by HIP events, so a bucket's reduction overlaps the rest of the backward pass:
 *   id    = scnattn_dp_unique_id() on rank 0, sent to the other ranks by any out-of-band channel (128 bytes);
 *   comm  = scnattn_dp_comm_create(id, world, rank) on every rank (current HIP device; collective);
 *   scnattn_dp_comm_allreduce_bucket(comm, compute_stream, buf, n): in-place SUM of n floats once everything enqueued
 *           on compute_stream so far has run; returns at once;
 *   scnattn_dp_comm_finish(comm, compute_stream): compute_stream waits for every bucket handed over so far
 *           (call before the optimizer reads the gradients; the 1/world scale is folded into scnattn_clamp_adam);
 *   scnattn_dp_comm_set_stream(comm, stream): optional -- reduce on a caller-owned stream instead of the library's
 *     (HIP maps streams onto a few hardware queues; a host that has probed which of its streams really run beside
 *     the compute stream hands that one over; NULL returns to the library's own stream);
 *   scnattn_dp_comm_destroy(comm).
 * Return codes >= 1000 are 1000 + ncclResult_t. */
typedef struct scnattn_dp_comm scnattn_dp_comm;
int scnattn_dp_unique_id(char out[128]);
int scnattn_dp_comm_create(const char id[128], int world, int rank, scnattn_dp_comm** out);
int scnattn_dp_comm_allreduce_bucket(scnattn_dp_comm* comm, void* compute_stream, float* buf, long n);
int scnattn_dp_comm_finish(scnattn_dp_comm* comm, void* compute_stream);
int scnattn_dp_comm_set_stream(scnattn_dp_comm* comm, void* stream);
int scnattn_dp_comm_world(const scnattn_dp_comm* comm);
int scnattn_dp_comm_destroy(scnattn_dp_comm* comm);

/* utils/optimizer.py:1-11 (element-wise clamp) fused with torch.optim.Adam's update
 * (trains/attention_scn.py:244-252); g is first scaled by gscale (1/world for data parallel).  The clamp keeps a NaN
 * gradient, as grad.clamp_ does: that element's m, v and p become NaN (a diverged step shows, it does not train on). */
int scnattn_clamp_adam(void* stream, long n, float* p, const float* g, float* m, float* v, double lr,
                       double beta1, double beta2, double eps, int step, double clip, double gscale);

#ifdef __cplusplus
}
#endif
#endif /* SCNATTN_H */
