/*
 * ccr_retrieval.h -- C ABI of the MI355X-native retrieval hot path
 *                    (encode output -> bf16 pack -> exhaustive Q.D^T -> top-k -> shard merge).
 *
 * The reference (awslabs/crowd-coachable-recommendations) has no FFI for this path: it is plain
 * Python over torch ops.  Each entry point below names the reference code it replaces
 * (file:line under the reference tree); INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is DEVICE memory unless marked host;
 *   - the caller owns every buffer; an index BORROWS the corpus pointer it was created on;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return value: CCR_OK (0) or a negative CCR_ERR_* code; ccr_last_error() gives the text
 *     (thread-local);
 *   - embeddings are bf16 bit patterns (uint16_t), row-major [rows][dim];
 *   - canonical arithmetic: score(q,d) = (float) sum_{i ascending} (double)q_i*(double)d_i,
 *     rank order = score descending, id ascending on equal scores.  Results of ccr_search are
 *     exactly that ordering for ANY input (near-ties and exact ties included).
 */
#ifndef CCR_RETRIEVAL_H
#define CCR_RETRIEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCR_OK 0
#define CCR_ERR_INVALID (-1)     /* bad argument (null pointer, dim not supported, k > rows, ...) */
#define CCR_ERR_HIP (-2)         /* a HIP runtime call failed */
#define CCR_ERR_WORKSPACE (-3)   /* workspace too small: see ccr_search_workspace_bytes */
#define CCR_ERR_BLOCK_ID (-4)    /* a blocked id is outside the corpus ("block id not found") */

#define CCR_DTYPE_F32 0
#define CCR_DTYPE_F16 1
#define CCR_DTYPE_BF16 2

/* ccr_search flags */
#define CCR_SEARCH_DEFAULT 0
#define CCR_SEARCH_FORCE_DENSE 1   /* fp64 brute-force path for every query (tests; the default path of a tiny corpus scores on the matrix
                                      cores and re-scores only the rows inside the error margin in fp64 -- same result) */
#define CCR_SEARCH_FORCE_FUSED 2   /* MFMA fused path even where the planner would pick dense */
#define CCR_SEARCH_ASYNC 4         /* do not synchronise: flagged queries (rare) are completed by ccr_search_finish() */

/* ccr_scores modes */
#define CCR_SCORES_CANONICAL 0     /* fp64-ordered canonical scores (bit-identical to the ranking's scores) */
#define CCR_SCORES_MFMA 1          /* the same bf16 rows through the MFMA tile kernel (fp32 accumulation, |err| < 1e-6) */

typedef struct ccr_index ccr_index;

/* statistics of the last ccr_search on an index (host struct, filled after the call returns) */
typedef struct ccr_search_stats {
    int32_t path;              /* 0 = dense exact, 1 = fused MFMA */
    int32_t n_fallback;        /* queries the first fused attempt flagged (candidate overflow / mass ties) */
    int32_t sample_tiles;      /* 256-row corpus tiles scored by the threshold (sample) pass */
    int32_t ranges;            /* corpus ranges of the main pass */
    int32_t cap;               /* candidate slots per sub-list */
    int32_t sublists;          /* sub-lists per (range, query): 8 = main pass on v_mfma_f32_16x16x32_bf16, 4 = 32x32x16 */
    int64_t n_candidates;      /* total stage-1 survivors over all queries */
    /* device time of each phase of the last search, from HIP events on the search stream (ms) */
    float ms_sample;           /* sample pass GEMM (group maxima) */
    float ms_threshold;        /* query norms + threshold select */
    float ms_main;             /* main pass GEMM + filter (the dominant kernel) */
    float ms_select;           /* stage-2 select + canonical re-score */
    float ms_fallback;         /* retry pass + dense path for flagged queries (0 if none) */
    float ms_total;
    int32_t n_retried;         /* flagged queries re-done by the fused retry pass (thresholds re-tightened from their own lists) */
    int32_t n_dense;           /* flagged queries finished by an exact whole-row path (margin select or fp64: mass ties, flagged again,
                                  on-stream chunk); path 0: queries the margin select left to the fp64 path */
    int32_t main_launches;     /* launches of the main-pass kernel in this search (phases: thresholds are re-tightened between them) */
    int32_t opt_rank;          /* > 0: the thresholds were ESTIMATED (the opt_rank-th largest sampled group maximum; one launch, verified by
                                  the select stage); 0: conservative lower bounds with re-tightening */
    int32_t main_tile_queries; /* queries per tile of the main pass: 256, or 384 (the 256 x 384 form, gemm_topk16w_kernel); 0 on the
                                  dense path and for the streaming pass of small batches */
    int32_t skipped_tiles;     /* corpus tiles the main pass did not score: the sampled tiles, whose rows the select stage joins from the
                                  sample pass's group maxima (CCR_SKIP_SAMPLED); 0: every tile was scored */
    int32_t tile_cap;          /* opt_rank > 0: groups of one sampled tile that count towards that rank (CCR_TILE_CAP; 16 = all of them);
                                  0 without estimated thresholds.  The struct grew from 80 to 88 bytes with it */
    int32_t main_grid;         /* workgroups of the main pass's tile kernel (0: the streaming pass of a small batch, the dense path) */
    int32_t side_cus;          /* CUs that main pass left free for the caller's side work (ccr_search_stream_wait_main_pass, CCR_SIDE_CUS);
                                  0: it ran on every CU.  The last field: the struct grew from 88 to 96 bytes with these two
                                  (ccr_version() >= 113) */
} ccr_search_stats;

const char *ccr_last_error(void);
int ccr_version(void);

/*
 * fp32 -> bf16 pack of encoder outputs, optionally L2-normalising each row first.
 * Replaces: the fp32 host copy + vstack of scripts/ms_marco_eval.py:141-149 (embeddings stay on
 * device as a packed bf16 shard) and, with normalize=1, the F.normalize calls of cos_sim
 * (scripts/ms_marco_eval.py:160-161; twin src/ccrec/models/bbpr.py:490-491).
 *   src   [rows][dim] fp32          dst  [rows][dim] bf16 (RNE; NaN stays NaN)
 *   norms [rows] fp32 or NULL: L2 norm of the fp32 row (before normalisation)
 * dim % 4 == 0.  normalize: y = x / max(||x||, 1e-12), fixed reduction order (oracle/ccr_oracle.c).
 */
int ccr_pack_bf16(const float *src, uint16_t *dst, float *norms, int64_t rows, int dim, int normalize, void *stream);
/* Same, plus row_norm_bounds ([rows] device floats, may be NULL): entry r receives an upper bound of the L2 norm of the
 * PACKED row r (one plain store per row: no initialisation needed, batches write disjoint slices of one shard-sized
 * array).  Passing the array on to ccr_index_create_with_norms saves the index build's own pass over the shard; the
 * index uses the bounds only inside its filter margins. */
int ccr_pack_bf16_ex(const float *src, uint16_t *dst, float *norms, float *row_norm_bounds, int64_t rows, int dim, int normalize,
                     void *stream);

/* Embeddings of ANY width (the reference takes any factor width: src/rime_lite/util/score_array.py:320-339,
 * src/ccrec/models/bbpr.py:536-540): rows of src_dim floats are packed into rows of dst_dim = src_dim rounded up to a multiple
 * of 8, the tail zero-filled -- inner products, norms and cosines are unchanged, and every search path takes the padded width
 * (the fused kernels zero-fill their last 32-element K step for widths that are not multiples of 32).
 *   norms / row_norm_bounds: as ccr_pack_bf16_ex.  The canonical sum of squares extends to any width by zero padding. */
int ccr_pack_bf16_padded(const float *src, int64_t rows, int src_dim, uint16_t *dst, int dst_dim, float *norms,
                         float *row_norm_bounds, int normalize, void *stream);

/*
 * Fused masked mean pooling (+ optional normalise) + pack of the encoder's last hidden state.
 * Replaces: src/ccrec/models/item_tower.py:137-147 (masked_fill, sum(dim=1), divide) followed by the pack.
 *   hidden [B][L][dim] of hidden_dtype (CCR_DTYPE_*), mask [B][L] int64 (0/1)
 *   dst_bf16 [B][dim] or NULL, dst_f32 [B][dim] or NULL (the un-rounded fp32 pooled rows)
 */
int ccr_meanpool_pack_bf16(const void *hidden, int hidden_dtype, const int64_t *mask, uint16_t *dst_bf16,
                           float *dst_f32, int B, int L, int dim, int normalize, void *stream);
/* Same for length-sorted (variable-length) encoder batches that write straight into the resident shard:
 *   dst_rows [B] int64 or NULL: pooled row b goes to row dst_rows[b] of dst_bf16 / dst_f32 (NULL = row b);
 *   row_norm_bounds (device floats, indexed like the destination rows) or NULL: a bound of each packed row's L2 norm,
 *   as ccr_pack_bf16_ex.
 * The pooled value does not depend on L (masked positions are skipped, real tokens are summed in order), so a batch
 * padded to its own longest text gives the same bits as the reference's fixed max_length padding (item_tower.py:29,
 * tokenizer_kw) whenever the encoder's hidden states for the real tokens are the same. */
int ccr_meanpool_pack_bf16_ex(const void *hidden, int hidden_dtype, const int64_t *mask, uint16_t *dst_bf16,
                              float *dst_f32, const int64_t *dst_rows, float *row_norm_bounds, int B, int L, int dim,
                              int normalize, void *stream);

/* Same for a PACKED token array (the kernel forward of the encoder layers runs on the real tokens only: no padding rows exist):
 *   hidden [T][dim]; sequence s is rows seq_start[s] .. seq_start[s] + seq_len[s] - 1 (int32 device arrays, as ccr_attention_bf16).
 * The sum runs over a sequence's tokens in order -- the same bits as the padded form gives for the same hidden states. */
int ccr_meanpool_pack_bf16_packed(const void *hidden, int hidden_dtype, const int32_t *seq_start, const int32_t *seq_len,
                                  uint16_t *dst_bf16, float *dst_f32, const int64_t *dst_rows, float *row_norm_bounds, int n_seq,
                                  int dim, int normalize, void *stream);

/*
 * The same packs into either 16-bit element type of a search index: half_dtype = CCR_DTYPE_BF16 or CCR_DTYPE_F16 (fp16 is what the
 * reference's autocast hands its `Q @ chunk.T`, scripts/ms_marco_eval.py:215: unit roundoff 2^-11 against bf16's 2^-8).  The arguments
 * are those of the bf16 entry points above -- which call these with CCR_DTYPE_BF16 and overflow = NULL -- plus
 *   overflow (device int32, may be NULL; the caller zeroes it once and may share it among any number of calls): incremented by the
 *   number of elements that were finite in fp32 and left fp16's range (|x| >= 65 520 -> +-inf, as torch's .to(float16)); one atomic
 *   per workgroup that saw any.  Never touched with CCR_DTYPE_BF16.
 * fp16 output is round-to-nearest-even and bit-identical to torch's conversion, subnormals included.  The normalising form, the norms
 * and row_norm_bounds are computed as in the bf16 form (a row with an out-of-range element gets an infinite bound).
 * ccr_version() >= 109.
 */
int ccr_pack_half_ex(const float *src, uint16_t *dst, float *norms, float *row_norm_bounds, int64_t rows, int dim, int normalize,
                     int half_dtype, int32_t *overflow, void *stream);
int ccr_pack_half_padded(const float *src, int64_t rows, int src_dim, uint16_t *dst, int dst_dim, float *norms, float *row_norm_bounds,
                         int normalize, int half_dtype, int32_t *overflow, void *stream);
int ccr_meanpool_pack_half_ex(const void *hidden, int hidden_dtype, const int64_t *mask, uint16_t *dst_half, float *dst_f32,
                              const int64_t *dst_rows, float *row_norm_bounds, int B, int L, int dim, int normalize, int half_dtype,
                              int32_t *overflow, void *stream);
int ccr_meanpool_pack_half_packed(const void *hidden, int hidden_dtype, const int32_t *seq_start, const int32_t *seq_len,
                                  uint16_t *dst_half, float *dst_f32, const int64_t *dst_rows, float *row_norm_bounds, int n_seq, int dim,
                                  int normalize, int half_dtype, int32_t *overflow, void *stream);

/* Backward of the pooling for the training forward (the reference's tower is called with gradients on in
 * src/ccrec/models/bbpr.py:130-141,195-197): dhidden[b][l][:] = mask[b][l] ? grad[b][:] / sum(mask[b]) : 0.
 *   grad [B][dim] fp32 (gradient w.r.t. the un-normalised pooled rows), dhidden [B][L][dim] of hidden_dtype. */
int ccr_meanpool_bwd(const float *grad, const int64_t *mask, void *dhidden, int hidden_dtype, int B, int L, int dim,
                     void *stream);

/*
 * The non-GEMM pieces of the encoder layer that produces `hidden` (the reference runs transformers' BertModel under autocast:
 * src/ccrec/models/item_tower.py:122 `cls_model(**inputs).last_hidden_state`, scripts/al_0_rank.py:92-101,125).  The
 * projections stay library GEMMs on the host side (hipBLASLt through torch); these two kernels replace the attention call
 * and the residual-add / LayerNorm / cast passes between them.  Arithmetic = the layer's under autocast(bf16): bf16 operands,
 * fp32 scores, softmax and accumulation, probabilities rounded to bf16 for the P.V product, fp32 residual sum and LayerNorm.
 *
 * ccr_attention_bf16: multi-head self-attention over n_seq sequences of a token array, head width 64.
 *   qkv [T][3 * n_heads * 64] bf16: row t = (Q | K | V) of token t, each n_heads * 64 wide -- the output of ONE projection with
 *     the query / key / value weights stacked (transformers' BertSelfAttention.query / .key / .value);
 *   seq_start [n_seq] int32: first row of sequence s in the token array; seq_len [n_seq] int32 (0 .. max_len; device memory, so the
 *     kernel itself cuts a larger entry to max_len and treats a negative one as 0): its real tokens
 *     (keys beyond are masked, as attention_mask = 0 is in the reference's inputs, scripts/al_0_rank.py:76-81 padding=True);
 *   out [T][n_heads * 64] bf16: context rows, heads side by side (the operand of BertSelfOutput.dense);
 *   max_len: longest seq_len (<= 512; sizes the LDS image of one head's keys and values);
 *   pad_len: 0 for a packed token array, or the padded length L of a right-padded [n_seq][L] batch (seq_start[s] = s * L):
 *     rows seq_len[s] .. pad_len - 1 of a sequence receive zeros;
 *   scale: 1 / sqrt(64) for BERT.
 * ccr_add_layernorm: y = LayerNorm(x + residual) * gamma + beta per row (BertSelfOutput / BertOutput: LayerNorm(dense(h) + input)).
 *   x_bf16 [rows][dim] bf16, residual [rows][dim] fp32 or NULL, gamma / beta [dim] fp32, dim % 256 == 0, dim <= 2048;
 *   out_f32 [rows][dim] or NULL (the residual stream), out_bf16 [rows][dim] or NULL (the next projection's operand).
 */
/* ccr_embed_layernorm: the embedding block in front of the layers (transformers BertEmbeddings.forward): row r =
 * LayerNorm((word_table[token_ids[r]] + type_table[token_types[r]]) + position_table[positions[r]]) * gamma + beta, fp32 tables
 * [n][dim], int64 indices (token_types NULL = type 0; an index outside its table is clamped), outputs as ccr_add_layernorm. */
int ccr_embed_layernorm(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                        const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                        const int64_t *token_types, const float *gamma, const float *beta, float eps, float *out_f32,
                        uint16_t *out_bf16, int64_t rows, int dim, void *stream);
/* ccr_gelu_bf16: y = GELU(x) elementwise on n bf16 values (n % 8 == 0, 16-byte aligned; y may be x), the exact erf form of
 * transformers' BertIntermediate (hidden_act "gelu") in fp32, rounded to bf16 once. */
int ccr_gelu_bf16(const uint16_t *x, uint16_t *y, int64_t n, void *stream);
int ccr_attention_bf16(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq,
                       int n_heads, int max_len, int pad_len, float scale, void *stream);
int ccr_add_layernorm(const uint16_t *x_bf16, const float *residual, const float *gamma, const float *beta, float eps,
                      float *out_f32, uint16_t *out_bf16, int64_t rows, int dim, void *stream);
/* The same four kernels on either 16-bit operand type: half_dtype = CCR_DTYPE_BF16 or CCR_DTYPE_F16, whichever the caller's autocast
 * context names.  The reference encodes under torch.cuda.amp.autocast() (scripts/al_0_rank.py:8,125), whose CUDA default is fp16:
 * fp16 operands and outputs for the projections, the attention call and the GELU, fp32 for the residual sum and LayerNorm
 * (src/ccrec/models/item_tower.py:122 runs transformers' BertLayer under it).  Every "bf16" array above is then an fp16 array; scores,
 * softmax, accumulation, residual stream and LayerNorm stay fp32 either way.  The *_bf16 / un-suffixed entry points above are these
 * with half_dtype = CCR_DTYPE_BF16. */
int ccr_attention_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq, int n_heads,
                       int max_len, int pad_len, float scale, int half_dtype, void *stream);
int ccr_add_layernorm_half(const uint16_t *x_half, const float *residual, const float *gamma, const float *beta, float eps,
                           float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype, void *stream);
int ccr_embed_layernorm_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                             const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                             const int64_t *token_types, const float *gamma, const float *beta, float eps, float *out_f32,
                             uint16_t *out_half, int64_t rows, int dim, int half_dtype, void *stream);
int ccr_gelu_half(const uint16_t *x, uint16_t *y, int64_t n, int half_dtype, void *stream);
/* ccr_attention_bias_half (library version 112; src/ccrec/models/bbpr.py:30, bert_mt.py:74: AutoModel.from_pretrained(MODEL_NAME) with an
 * MPNet checkpoint): ccr_attention_half with one additive relative position bias shared by every sequence -- the probability of (query i,
 * key j) of head h is proportional to exp(scale * q_i.k_j + rel_bias[h][R + j - i]) in fp32, keys beyond the sequence excluded, the
 * running maximum taken over the biased scores.  rel_bias: fp32 [n_heads][2 * R + 1] on the device, max_len - 1 <= R <= 511 (a table
 * built once for R = 511 serves every batch).  With an all-zero table `out` has ccr_attention_half's bits.  Inference only: the training
 * forward and the backward take no bias. */
int ccr_attention_bias_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, const float *rel_bias,
                            int R, int n_seq, int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *stream);
/* ccr_attention_head_half (library version 114; the MiniLM-class encoders: hidden 384, 12 heads of width 32): ccr_attention_half with the
 * head width as an argument.  head_width = 64 runs exactly what ccr_attention_half runs; head_width = 32 runs the narrow-head kernel on
 * qkv [T][3 * n_heads * 32] -> out [T][n_heads * 32] (scale: 1 / sqrt(32) for BERT), with the same rules for padding rows, empty and
 * over-long entries; any other head_width: CCR_ERR_INVALID.  Inference only, no bias form at width 32.
 * With the same library version ccr_add_layernorm(_half) and ccr_embed_layernorm(_half) also take the odd multiples of 128
 * (dim % 128 == 0, 256 <= dim <= 2048); the entry points that read keep bits, the training forward and the backward keep dim % 256 == 0. */
int ccr_attention_head_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq, int n_heads,
                            int head_width, int max_len, int pad_len, float scale, int half_dtype, void *stream);

/*
 * The layer kernels' training forward and backward (library version 103): fine-tuning through the encoder.  The reference's training
 * steps run the encoder three times per step with gradients on, then its backward (src/ccrec/models/bbpr.py:195-197 _pairwise over
 * i | j | k texts; bert_mt.py:105-113 the same three towers for the contrastive and the masked-token terms).  Arrays, layouts and
 * half_dtype as in the forward entry points above; scores, probabilities, dS and every reduction are fp32; no atomics: results are
 * bit-identical from run to run.
 * ccr_attention_fwd_train_half (bbpr.py:195-197, bert_mt.py:105-113): the attention forward, `out` bit-identical to ccr_attention_half's,
 *   which also writes lse [T][n_heads] fp32: the natural-log log-sum-exp of every real query row's scaled scores (0 on padding rows).
 * ccr_attention_bwd_half (bbpr.py:195-197, bert_mt.py:105-113: loss.backward() through BertSelfAttention): d_qkv [T][3 * n_heads * 64],
 *   the gradient of the stacked projection's output in qkv's type and layout, from qkv, the forward's out and lse, and d_out
 *   [T][n_heads * 64].  Every row inside a sequence's max(seq_len, pad_len) rows is written: padding rows and empty sequences get
 *   zeros; padding rows of qkv, out and d_out are never read.
 *   workspace: ccr_attention_bwd_workspace_bytes(n_seq, n_heads, max_len) bytes of DEVICE memory, 4-byte aligned; CCR_ERR_WORKSPACE
 *   if it is smaller.
 * ccr_attention_bwd_workspace_bytes (bbpr.py:195-197, bert_mt.py:105-113: the scratch of that backward): one fp32 per query row (max_len
 *   rounded up to 32) and head; 0 with a ccr_last_error() text for a shape outside the limits above.
 * ccr_add_layernorm_bwd_half (bbpr.py:195-197, bert_mt.py:105-113: BertSelfOutput / BertOutput LayerNorm): from x_half, residual (or
 *   NULL), gamma, eps as the forward took them and d_y [rows][dim] fp32, the summed gradient of the LayerNorm output:
 *   d_res [rows][dim] fp32 = the gradient of x + residual; d_x = the same values rounded to x's type; d_gamma, d_beta [dim] fp32.
 *   Any of the four may be NULL.  Mean and rstd are recomputed as the forward computes them.
 *   workspace (DEVICE, 16-byte aligned), needed when d_gamma or d_beta is asked for: min((rows + 3) / 4, 512) * 2 * dim * 4 bytes
 *   (per-workgroup column sums, added up by a second kernel in a fixed order); NULL / 0 otherwise.
 * ccr_gelu_bwd_half (bert_mt.py:105-113, bbpr.py:195-197: BertIntermediate): d_x = d_y * (Phi(x) + x * phi(x)) from the pre-activation
 *   x, n % 8 == 0, 16-byte aligned arrays, fp32 arithmetic rounded once (d_x may be d_y).
 */
int ccr_attention_fwd_train_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, float *lse,
                                 int n_seq, int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *stream);
size_t ccr_attention_bwd_workspace_bytes(int n_seq, int n_heads, int max_len);
int ccr_attention_bwd_half(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out, const int32_t *seq_start,
                           const int32_t *seq_len, uint16_t *d_qkv, int n_seq, int n_heads, int max_len, int pad_len, float scale,
                           int half_dtype, void *workspace, size_t workspace_bytes, void *stream);
int ccr_add_layernorm_bwd_half(const uint16_t *x_half, const float *residual, const float *gamma, float eps, const float *d_y,
                               float *d_res, uint16_t *d_x, float *d_gamma, float *d_beta, int64_t rows, int dim, int half_dtype,
                               void *workspace, size_t workspace_bytes, void *stream);
int ccr_gelu_bwd_half(const uint16_t *x, const uint16_t *d_y, uint16_t *d_x, int64_t n, int half_dtype, void *stream);

/*
 * Training dropout for the layer kernels (library version 104).  The reference fine-tunes its towers in train() mode with the
 * checkpoints' own dropout 0.1 (src/ccrec/models/bbpr.py:195-197, bert_mt.py:105-113).  No layer kernel draws a random number: two
 * generator kernels write PACKED KEEP BITS (1 = keep), and the *_drop_* entry points below are the layer kernels above reading those
 * bits plus one scale factor, so the forward and both backward passes see the same stored decisions and a caller may pass any mask.
 * A decision is a pure function of (seed, stream_id, indices): Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 / 0xBB67AE85, key = seed's low and high word); the four output words are eight 16-bit lanes (low half of word 0, high
 * half of word 0, low half of word 1, ..), lane j decides element 8 * group + j, keep iff lane >= thr = floor(p * 65536 + 0.5).  The
 * probability actually used is p_eff = thr / 65536 and the matching scale is inv_keep = 65536 / (65536 - thr).  0 <= p and thr < 65536,
 * else CCR_ERR_INVALID.  ccrec_amd/dropout_ref.py restates the generator on the CPU.
 * ccr_dropout_bits_rows (bbpr.py:195-197, bert_mt.py:105-113: the hidden-state dropouts of BertEmbeddings / BertSelfOutput / BertOutput):
 *   bits [rows][dim / 32] uint32 for a [rows][dim] tensor, dim % 256 == 0, dim <= 2048; bit i of word w <-> column 32 * w + i; counter =
 *   (row, column >> 3, stream_id, 0).
 * ccr_dropout_bits_attention (bbpr.py:195-197, bert_mt.py:105-113: the dropout on BertSelfAttention's probabilities): counter = (token
 *   row of the query = seq_start[s] + q, k >> 3, stream_id, head).  Two arrays [n_tokens][n_heads][W] uint32, W = ceil(max_len / 32), hold
 *   the same decisions: keep_q row = the query's token row, bit = key position; keep_k row = the key's token row, bit = query
 *   position (what the dK / dV pass reads).  Bits of positions >= seq_len[s] are unspecified, and no kernel lets them matter; rows of
 *   no sequence are not written.
 * ccr_dropout_apply (bbpr.py:195-197, bert_mt.py:105-113: BertEmbeddings.dropout after the embedding LayerNorm): y = x * keep * inv_keep
 *   elementwise, x [rows][dim] fp32 -> out_f32 and / or out_half (either may be NULL); its backward is the same call on the gradient.
 * ccr_attention_fwd_train_drop_half (bbpr.py:195-197, bert_mt.py:105-113): ccr_attention_fwd_train_half where the probability that is
 *   rounded to 16 bits for the P.V product is p * keep * inv_keep; the softmax and lse are those of the undropped scores.
 * ccr_attention_bwd_drop_half (bbpr.py:195-197, bert_mt.py:105-113): ccr_attention_bwd_half for that forward; with m = keep * inv_keep
 *   the P operand of dV is P * m and dS = P * (dP * m - delta).  Same workspace as ccr_attention_bwd_half.
 * ccr_add_layernorm_drop_half (bbpr.py:195-197, bert_mt.py:105-113: LayerNorm(dropout(dense(h)) + input)): ccr_add_layernorm_half on
 *   v = x * keep * inv_keep + residual, one fp32 fused multiply-add per element.
 * ccr_add_layernorm_bwd_drop_half (bbpr.py:195-197, bert_mt.py:105-113): ccr_add_layernorm_bwd_half with v recomputed from the same bits;
 *   d_res as there, d_x = d_res * keep * inv_keep rounded to x's type.
 * inv_keep: 1 .. 65536.  With all-ones bits and inv_keep = 1 every *_drop_* entry point returns the bits of its dropout-free twin.
 */
int ccr_dropout_bits_rows(uint32_t *bits, int64_t rows, int dim, uint64_t seed, uint32_t stream_id, double p, void *stream);
int ccr_dropout_bits_attention(uint32_t *keep_q, uint32_t *keep_k, const int32_t *seq_start, const int32_t *seq_len, int64_t n_tokens,
                               int n_seq, int n_heads, int max_len, uint64_t seed, uint32_t stream_id, double p, void *stream);
int ccr_dropout_apply(const float *x, const uint32_t *bits, float inv_keep, float *out_f32, uint16_t *out_half, int64_t rows, int dim,
                      int half_dtype, void *stream);
int ccr_attention_fwd_train_drop_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, float *lse,
                                      const uint32_t *keep_q, float inv_keep, int n_seq, int n_heads, int max_len, int pad_len,
                                      float scale, int half_dtype, void *stream);
int ccr_attention_bwd_drop_half(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out,
                                const int32_t *seq_start, const int32_t *seq_len, const uint32_t *keep_q, const uint32_t *keep_k,
                                float inv_keep, uint16_t *d_qkv, int n_seq, int n_heads, int max_len, int pad_len, float scale,
                                int half_dtype, void *workspace, size_t workspace_bytes, void *stream);
int ccr_add_layernorm_drop_half(const uint16_t *x_half, const uint32_t *bits, float inv_keep, const float *residual, const float *gamma,
                                const float *beta, float eps, float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype,
                                void *stream);
int ccr_add_layernorm_bwd_drop_half(const uint16_t *x_half, const uint32_t *bits, float inv_keep, const float *residual,
                                    const float *gamma, float eps, const float *d_y, float *d_res, uint16_t *d_x, float *d_gamma,
                                    float *d_beta, int64_t rows, int dim, int half_dtype, void *workspace, size_t workspace_bytes,
                                    void *stream);

/*
 * Build a search index over a resident bf16 corpus shard (borrowed pointer, no copy).
 * Replaces: the host-resident fp32 passage matrix of scripts/ms_marco_eval.py:199-201,208-210.
 *   global_row_offset: id of row 0 of this shard in the whole corpus (multi-GPU row sharding).
 * Synchronises `stream` once (one pass over the shard: the largest row norm of every 256-row tile, for the filter margins).
 */
int ccr_index_create(const uint16_t *D_bf16, int64_t n_rows, int dim, int64_t global_row_offset, void *stream,
                     ccr_index **out);
/* As ccr_index_create, but the caller supplies (device pointer, [n_rows] floats) an upper bound of every row's norm
 * (from ccr_pack_bf16_ex / ccr_meanpool_pack_bf16_ex): no pass over the corpus, no stream synchronisation.  The array is
 * BORROWED like the corpus: it must stay valid and unchanged until the index is destroyed (the main pass uses the largest
 * bound of each 256-row tile, the select stage each candidate row's own bound). */
int ccr_index_create_with_norms(const uint16_t *D_bf16, int64_t n_rows, int dim, int64_t global_row_offset,
                                const float *row_norm_bounds, void *stream, ccr_index **out);
/*
 * The same two over a shard of either 16-bit element type: half_dtype = CCR_DTYPE_BF16 (what the two names above pass) or
 * CCR_DTYPE_F16.  EVERY search-side entry point then takes query matrices of the index's type -- ccr_search, ccr_search_finish,
 * ccr_scores (both modes), ccr_search_blocked, ccr_search_sparse_prior, ccr_search_shard and the retry, margin and fp64 dense paths
 * behind them -- with unchanged signatures: the `Q_bf16` arguments read "16-bit rows of ccr_index_dtype(index)".  The canonical
 * score, the order and the path independence are those of the bf16 index (a product of two fp16 values is exact in fp64 as well);
 * only the MFMA instruction and the element-to-float conversion differ.  ccr_version() >= 109.
 */
int ccr_index_create_half(const uint16_t *D, int64_t n_rows, int dim, int half_dtype, int64_t global_row_offset, void *stream,
                          ccr_index **out);
int ccr_index_create_with_norms_half(const uint16_t *D, int64_t n_rows, int dim, int half_dtype, int64_t global_row_offset,
                                     const float *row_norm_bounds, void *stream, ccr_index **out);
int ccr_index_destroy(ccr_index *index);
int64_t ccr_index_rows(const ccr_index *index);
int ccr_index_dim(const ccr_index *index);
int ccr_index_dtype(const ccr_index *index);   /* CCR_DTYPE_BF16 or CCR_DTYPE_F16; -1 for NULL.  ccr_version() >= 109 */

/*
 * Exhaustive inner-product top-k of n_q queries against the shard.
 * Replaces: the score loop, the host [Q,N] matrix and the per-row full sort of
 * scripts/ms_marco_eval.py:203-218,228-230, and the per-batch topk of
 * src/rime_lite/util/__init__.py:136-142.
 *   Q_bf16 [n_q][dim]; out_scores [n_q][k] fp32; out_ids [n_q][k] int64 (global ids)
 *   1 <= k <= min(n_rows, 4096).
 * The call returns after the results are complete on `stream` (it synchronises the stream once
 * to read the fallback count).  With CCR_SEARCH_ASYNC in `flags` it returns without synchronising: the kernels are
 * enqueued and the caller may enqueue more work (e.g. the shard exchange); ccr_search_finish(index) -- which waits for THIS
 * search's own event (not for work enqueued after it), fills the statistics and re-does the queries the search flagged
 * (sub-list overflow, mass ties, an estimated threshold that failed its check: rare) -- must run before the results of
 * flagged queries are trusted (ccr_search_last_stats().n_fallback tells how many there were; the lists of all other queries
 * are final on the stream).  Buffers and workspace must stay valid until then.
 * Embeddings are expected to be finite.  NaN / Inf values do not fault: the filter margins become infinite, every
 * query takes the exact dense path, +-Inf scores rank as numbers and NaN scores rank by bit pattern (not torch.sort's
 * NaN-first rule) -- identically on every path.
 */
size_t ccr_search_workspace_bytes(const ccr_index *index, int n_q, int k);
int ccr_search(ccr_index *index, const uint16_t *Q_bf16, int n_q, int k, float *out_scores, int64_t *out_ids,
               void *workspace, size_t ws_bytes, int flags, void *stream);
int ccr_search_finish(ccr_index *index);
int ccr_search_last_stats(const ccr_index *index, ccr_search_stats *stats /* host */);
/*
 * Releases `stream` when SIDE WORK can usefully start beside the index's last search -- possibly still pending (CCR_SEARCH_ASYNC).
 * Side work is work that does not depend on that search's results and touches none of its buffers, inputs included (the select
 * stage reads them all): packing the NEXT corpus shard into another buffer, the reference's next `embedding_func` batch of
 * scripts/ms_marco_eval.py:141-149.
 *   - A main pass (the dominant kernel) that ran on every CU: `stream` waits until it has completed; the side work runs beside the
 *     select stage instead of behind it.
 *   - A main pass that left CUs free (ccr_search_stats.side_cus > 0): `stream` waits until that pass BEGINS, then for a one-wave gate
 *     kernel that returns when the pass's workgroups are resident (bounded: at most a few hundred microseconds); the side work runs
 *     on the free CUs beside the main pass.  An HBM-bound pack hides behind the matrix-core-bound pass that way.
 * The call is also the HINT that lets a search leave CUs free: a fused search does so only if this function was called for the
 * previous fused search on the same device (and CCR_SIDE_CUS is not 0: -1 = the planner's choice of their number, where it
 * prices them as paying; n = that many, rounded to a multiple of 8).  A search that is not followed by the call switches it off
 * again; the first search of a loop never leaves CUs free.  Results do not depend on any of this.
 * No-op when the last search took the dense path (nothing recorded).  No host synchronisation.  ccr_version() >= 113 for the second form.
 */
int ccr_search_stream_wait_main_pass(const ccr_index *index, void *stream);
/*
 * Query groups of the last search's main pass when they were UNEQUAL (2, 4 or 8 groups over the XCDs that do not divide the count
 * of query blocks: each keeps its whole blocks, the left-over blocks are shared range by range -- CCR_QSPLIT); 0: equal groups, the
 * streaming pass of a small batch, the dense path, or no search yet.  ccr_version() >= 105.
 */
int ccr_search_last_main_split(const ccr_index *index);
/*
 * Group phases per query of the last search's threshold kernel: 16 (workgroups of 256 threads) or 64 (1 024 threads, the form a
 * large sample gets; CCR_THR_PHASES = 16 / 64 pins it).  Both forms compute the same thresholds bit for bit.  0: the small-batch
 * threshold kernel, the dense path, or no search yet.  ccr_version() >= 106.
 */
int ccr_search_last_threshold_phases(const ccr_index *index);

/*
 * Dense score matrix of n_q queries against the shard: out [n_q][n_rows] fp32.
 * Replaces: cos_sim / the chunked `Q @ chunk^T` of scripts/ms_marco_eval.py:155-162,212-215 and
 * src/ccrec/models/bbpr.py:485-492,536-540 when a caller really wants the matrix (small problems; the ranking path
 * never materialises it).  mode: CCR_SCORES_CANONICAL or CCR_SCORES_MFMA.
 */
int ccr_scores(const ccr_index *index, const uint16_t *Q_bf16, int n_q, int mode, float *out, void *stream);

/*
 * Search with per-query blocked ids of ANY length (the reference blocks any number of ids per query:
 * scripts/ms_marco_eval.py:224-227, scores[block_ind] = -1e6, kept not removed).
 *   block_ptr_host [n_q + 1] (HOST), block_idx [block_ptr_host[n_q]] int64 GLOBAL ids (DEVICE), ascending and unique inside
 *   each query; ids outside this shard's [offset, offset + n_rows) are ignored (row-sharded search: every rank passes the
 *   whole list).  Queries with k + len <= min(n_rows, 4096) over-fetch through the fused path and post-filter
 *   (ccr_apply_block); longer lists take the exact dense path with the blocked columns set to -1e6 before the selection.
 *   Result: canonical order of the modified scores, exactly k entries per query.
 */
size_t ccr_search_blocked_workspace_bytes(const ccr_index *index, int n_q, int k, const int64_t *block_ptr_host);
int ccr_search_blocked(ccr_index *index, const uint16_t *Q_bf16, int n_q, int k, const int64_t *block_ptr_host,
                       const int64_t *block_idx, float *out_scores, int64_t *out_ids, void *workspace, size_t ws_bytes,
                       int flags, void *stream);

/*
 * Top-k of (low-rank score + sparse prior), the post-fit expression of the ranker API:
 *   bbpr.transform(gnd) + gnd.prior_score -> evaluate_item_rec(..., k)   (src/ccrec/models/bbpr.py:592-595;
 *   _assign_topk src/rime_lite/util/__init__.py:117-155 over ElementWiseExpression(add, [dense, sparse]),
 *   src/rime_lite/util/score_array.py:300-318).
 *   prior CSR: prior_ptr_host [n_q + 1] (HOST), prior_idx int64 GLOBAL column ids ascending and unique per row (DEVICE),
 *   prior_val fp64 (DEVICE); at most 4096 entries per row.
 *   final(q, j) = (double) canonical_score(q, j) + prior(q, j)  (fp64, as torch promotes fp32 + fp64);
 *   out_scores fp64 [n_q][k], out_ids [n_q][k] in the order (final desc, id asc).
 * Exact for any prior values (negative ones included): the candidates are the top-(k + nnz_q) of the low-rank score
 * plus every prior column of the row (those are re-scored canonically).
 */
size_t ccr_search_sparse_prior_workspace_bytes(const ccr_index *index, int n_q, int k, const int64_t *prior_ptr_host);
int ccr_search_sparse_prior(ccr_index *index, const uint16_t *Q_bf16, int n_q, int k, const int64_t *prior_ptr_host,
                            const int64_t *prior_idx, const double *prior_val, double *out_scores, int64_t *out_ids,
                            void *workspace, size_t ws_bytes, int flags, void *stream);

/*
 * Column sums of a bf16 matrix in fp64: out[c] = sum_r X[r][c] (fixed order per column block, deterministic).
 * Used by score_op(S, "sum") for a low-rank S = U V^T: sum_ij S_ij = colsum(U) . colsum(V)
 * (src/rime_lite/util/score_array.py:460-474 without materialising any batch of S).
 */
int ccr_colsum_bf16(const uint16_t *X, int64_t rows, int dim, double *out /* [dim] device */, void *stream);
/* The same for a matrix of half_dtype (CCR_DTYPE_BF16 / CCR_DTYPE_F16) elements.  ccr_version() >= 109. */
int ccr_colsum_half(const uint16_t *X, int64_t rows, int dim, int half_dtype, double *out /* [dim] device */, void *stream);

/*
 * Merge R per-shard top-k lists (after the RCCL all-gather) into the global top-k.
 * New (the reference scores on one GPU only: SURVEY 2a); order rule as above.
 *   scores [R][n_q][k], ids [R][n_q][k] -> out_scores [n_q][k], out_ids [n_q][k];  k <= 4096.
 */
int ccr_merge_topk(const float *scores, const int64_t *ids, int R, int n_q, int k, float *out_scores,
                   int64_t *out_ids, void *stream);
/* Same merge over rank-strided inputs: list (r, q) starts at scores + r * score_rank_stride + q * k and
 * ids + r * id_rank_stride + q * k (strides in elements).  This is the layout ONE all-gather of a packed per-rank
 * message {scores [n_q][k] fp32 | ids [n_q][k] int64} leaves behind: a single collective instead of two. */
int ccr_merge_topk_strided(const float *scores, const int64_t *ids, int64_t score_rank_stride, int64_t id_rank_stride,
                           int R, int n_q, int k, float *out_scores, int64_t *out_ids, void *stream);

/*
 * Packed per-shard result message of a row-sharded search: ONE all-gather (RCCL) moves it, one kernel merges the gathered copies.
 * New (the reference scores on one GPU only, scripts/ms_marco_eval.py:205-218); what it replaces there is the per-row
 * sort + keep-1001 of :228-230 for a corpus split over the GPUs of a node.
 *   layout: 32-byte ccr_shard_header | scores [n_q][k] fp32 | pad to 16 B | rows [n_q][k] u32 LOCAL row of this shard | pad to 16 B
 *   8 bytes per entry on the wire (12 with int64 global ids); the merge adds header.row_offset.
 * ccr_search_shard == ccr_search writing that message.  With CCR_SEARCH_ASYNC the call does not synchronise and the header's
 * n_flagged is written ON THE STREAM (the select stage's flag count): after the all-gather every rank reads every rank's
 * {n_flagged, n_covered} and all ranks take the same branch -- lists are final iff n_flagged <= n_covered (= 0) on every rank, otherwise
 * the flagged ranks call ccr_search_finish and the exchange is repeated by ALL ranks (a matched second collective).
 * 1 <= k <= min(n_rows, 4096); a shard smaller than k searches k_valid = n_rows entries and fills the message with
 * ccr_shard_message_fill instead.
 */
#define CCR_SHARD_MAGIC 0x4d524343u /* "CCRM" */
typedef struct ccr_shard_header {
    uint32_t magic;
    uint32_t n_flagged;   /* queries flagged by the shard's asynchronous search (0 after a synchronous one) */
    uint32_t k_valid;     /* entries of every list that are real rows; slots [k_valid, k) are padding */
    uint32_t n_covered;   /* flagged queries the search completed on the stream by itself (0: ccr_search_finish completes them) */
    int64_t row_offset;   /* global id of the shard's row 0 */
    int64_t n_rows;       /* rows of the shard */
} ccr_shard_header;
size_t ccr_shard_message_bytes(int n_q, int k);
int ccr_search_shard(ccr_index *index, const uint16_t *Q_bf16, int n_q, int k, void *message, void *workspace, size_t ws_bytes,
                     int flags, void *stream);
/* Build a message from ordinary results (blocked searches, shards smaller than k):
 *   scores [n_q][k_valid] fp32, ids [n_q][k_valid] int64 GLOBAL ids inside [row_offset, row_offset + n_rows), k_valid <= k. */
int ccr_shard_message_fill(void *message, int n_q, int k, int k_valid, const float *scores, const int64_t *ids, int64_t row_offset,
                           int64_t n_rows, void *stream);
/* Merge R gathered messages (message r at messages + r * message_stride_bytes) into the global top-k: out_scores [n_q][k] fp32,
 * out_ids [n_q][k] int64 global ids, order rule as everywhere.  Padding slots rank last (score -inf, distinct ids above 2^62), so
 * every output slot is written even when the whole corpus holds fewer than k rows.  k <= 4096, R <= 64. */
int ccr_merge_shard_messages(const void *messages, int64_t message_stride_bytes, int R, int n_q, int k, float *out_scores,
                             int64_t *out_ids, void *stream);
/* Short-list exchange (the k that scripts/ms_marco_eval.py:230 keeps -- 1001 -- over R shards).  A shard of exchangeable rows holds
 * k / R +- sqrt(k (1/R)(1 - 1/R)) of a global top-k, so every rank searches and sends only its canonical top-k_list, k_list ~ k / R + 6 sigma
 * (ccr_search_shard(..., k_list, ...): the select / re-score stage, which does not shrink with the shard, does k_list instead of k rows per
 * query, and the message is k_list / k of the size).  This merge keeps the k_out best of the R k_list entries and VERIFIES the shortcut: a
 * shard's list is its exact top-k_list, so if its last entry is not among the kept k_out, none of its unsent rows is either and the result
 * is the global top-k_out, bit for bit.  flags[q] = 1 (and *n_flagged counts them; both device memory, n_flagged zeroed by the call) where some
 * list was consumed to its end while its shard (header.n_rows > header.k_valid) holds more rows: the caller repeats THOSE queries with full
 * lists (every rank computes the same flags from the same gathered bytes, so the repeat is a matched collective).
 *   messages: R gathered messages of ccr_shard_message_bytes(n_q, k_list) layout; out_* [n_q][k_out]; k_list <= k_out <= R k_list;
 *   R k_list 12 B <= 96 KiB (the lists of a query are merged in LDS). */
int ccr_merge_short_lists(const void *messages, int64_t message_stride_bytes, int R, int n_q, int k_list, int k_out, float *out_scores,
                          int64_t *out_ids, uint32_t *flags, uint32_t *n_flagged, void *stream);

/*
 * Apply per-query blocked ids to an over-fetched result list.
 * Replaces: scripts/ms_marco_eval.py:224-227 (scores[block_ind] = -1e6, kept not removed).
 *   in_* [n_q][k_in] canonical top-k_in with k_in >= min(n_rows, k_out + max block length);
 *   block_ptr [n_q+1], block_idx [block_ptr[n_q]] int64 global ids, ascending inside each query;
 *   out_* [n_q][k_out]: unblocked entries in order, then (only if fewer than k_out remain)
 *   blocked ids ascending with score -1e6.  n_rows_total bounds valid ids (CCR_ERR_BLOCK_ID).
 */
int ccr_apply_block(const float *in_scores, const int64_t *in_ids, int n_q, int k_in, const int64_t *block_ptr,
                    const int64_t *block_idx, int64_t n_rows_total, float *out_scores, int64_t *out_ids, int k_out,
                    void *stream);

/*
 * In-batch-negative contrastive loss ("multiple_nrl"), forward and backward.
 * Replaces: src/ccrec/models/bbpr.py:205-212 (two mm + cat + scale + CrossEntropyLoss mean).
 *   Qe, Pe, Ne [B][dim] bf16; logits = [Qe Pe^T | Qe Ne^T] * inv_temperature (fp32 accumulate)
 *   fwd: loss (1 float, mean CE with labels arange(B)), lse [B] (saved for bwd)
 *   bwd: dQ, dP, dN [B][dim] fp32 = grad_out * dloss/d(.)
 *   workspace: ccr_inbatch_ce_workspace_bytes(B, dim) bytes of device memory (16-byte aligned); dim % 16 == 0 (the
 *   Python ops.inbatch_ce sends every other width to ccr_pool_ce_* below, zero-padded to a multiple of 8); the embedding
 *   pointers 16-byte aligned.  The FORWARD leaves the scaled logits ([2B][B] fp32) in it and the BACKWARD reads them there
 *   instead of recomputing them: pass the backward the same, unmodified workspace its forward call used (the Python autograd
 *   function saves it with the operands).  The forward also leaves a stamp {magic, B, dim, inv_temperature} behind its logits and
 *   the backward checks it ON THE DEVICE: a workspace that is not this (B, dim, inv_temperature) forward's -- scratch memory, or one
 *   another forward has started on since -- yields NaN gradients, not plausible garbage (no host round trip, so no error code).
 *   Launches: forward = one kernel (+ a memset of its tickets and stamp), backward = two kernels (the gradient of the logits evaluated
 *   and split into three bf16 parts once, in both orientations, + the embeddings' transposes; then one launch for dQ and dP | dN with
 *   every MFMA fragment read straight from L2); deterministic (fixed combine orders, no float atomics).
 *   ccr_inbatch_pack3_bf16: the step's three fp32 blocks [B][dim] -> out [3][B][dim] bf16 (RNE, torch's .to(bfloat16) bits) in ONE
 *   launch (dim % 8 == 0, 16-byte aligned pointers); ccr_inbatch_ce_fwd_f32 = that pack into `packed` + the forward on the packed
 *   blocks in one call (the autograd function's host path: the backward takes packed, packed + B dim, packed + 2 B dim).
 */
size_t ccr_inbatch_ce_workspace_bytes(int B, int dim);
int ccr_inbatch_pack3_bf16(const float *q, const float *p, const float *n, int B, int dim, uint16_t *out, void *stream);
int ccr_inbatch_ce_fwd_f32(const float *q, const float *p, const float *n, int B, int dim, float inv_temperature, uint16_t *packed,
                           float *loss, float *lse, void *workspace, size_t ws_bytes, void *stream);
int ccr_inbatch_ce_fwd(const uint16_t *Qe, const uint16_t *Pe, const uint16_t *Ne, int B, int dim,
                       float inv_temperature, float *loss, float *lse, void *workspace, size_t ws_bytes, void *stream);
int ccr_inbatch_ce_bwd(const uint16_t *Qe, const uint16_t *Pe, const uint16_t *Ne, const float *lse, int B, int dim,
                       float inv_temperature, float grad_out, float *dQ, float *dP, float *dN, void *workspace,
                       size_t ws_bytes, void *stream);
/* Same with the upstream gradient read from device memory (a 1-element fp32 tensor, as autograd hands it over):
 * no host read-back of the scalar, so the training step stays asynchronous. */
int ccr_inbatch_ce_bwd_dev(const uint16_t *Qe, const uint16_t *Pe, const uint16_t *Ne, const float *lse, int B, int dim,
                           float inv_temperature, const float *grad_out_dev, float *dQ, float *dP, float *dN,
                           void *workspace, size_t ws_bytes, void *stream);

/*
 * Contrastive cross-entropy of n_q queries over a pool of n_c candidates, with a label and a weight per query: the general form
 * of the loss above (several hard negatives per query, per-sample weights, candidates gathered from other ranks).
 *   Q [n_q][dim], C [n_c][dim] bf16 (16-byte aligned); label [n_q] int32 (DEVICE); weight [n_q] fp32 (DEVICE) or NULL = all ones
 *   s_ij = inv_temperature <Q_i, C_j> (fp32 accumulate);  ce_i = logsumexp_j s_ij - s_{i,label_i};  loss = sum w_i ce_i / sum w_i
 *   fwd: out3 [3] fp32 (DEVICE) = {loss, numerator sum w_i ce_i, denominator sum w_i}; lse [n_q] fp32 (saved for the backward)
 *   bwd: dQ [n_q][dim], dC [n_c][dim] fp32 (16-byte aligned) = sum over the pool / the queries of
 *        G_ij = (softmax_ij - [j = label_i]) w_i inv_temperature grad_out / W
 *        grad_out_dev: the upstream gradient, one fp32 on the device; W_dev: NULL = the forward's own denominator, or one fp32 on the
 *        device (the cross-rank form hands over the denominator summed over all ranks)
 *   Sizes: n_q >= 1, n_c >= 1, dim % 8 == 0; n_q <= 65 536, n_c <= 1 048 576, dim <= 8 192 and at most 2^28 logits (1 GiB) after
 *   padding both counts to multiples of 64: 4 096 x 65 536 at any supported width is the largest.  Beyond that: CCR_ERR_INVALID with a
 *   ccr_last_error() text, and ccr_pool_ce_workspace_bytes returns 0.
 *   workspace: ccr_pool_ce_workspace_bytes(n_q, n_c, dim) bytes of device memory (16-byte aligned).  The FORWARD leaves the scaled
 *   logits ([n_q][n_c] fp32: 64 MB at 1 024 x 16 384), its numerator and denominator and a stamp {magic, n_q, n_c, dim,
 *   inv_temperature} in it; pass the BACKWARD the same, unmodified workspace with the same label, weight and lse.  Checked ON THE
 *   DEVICE, no read-back, hence no error code: a label outside [0, n_c) makes the loss, the numerator and every gradient NaN (no
 *   address depends on a label's value); sum w = 0 gives NaN as the expression does; a workspace whose stamp is not this
 *   forward's -- scratch memory, another shape's, or one another forward has started on -- makes every gradient NaN.
 *   Launches: forward = logits GEMM, per-query log-sum-exp, finish (3); backward = transposes, dQ GEMM, dC GEMM, + one fixed-order sum
 *   per GEMM whose contraction was split (3 to 5).  Every GEMM stages both operands in LDS; the gradient of the logits is evaluated
 *   from the kept logits while it is staged and split into three bf16 parts (fp32-product accuracy).  Deterministic: no atomics.
 *   ccr_pool_ce_fwd_f32 = fp32 -> bf16 (RNE, torch's .to(bfloat16) bits) of q and c into packed [(n_q + n_c)][dim] + the forward on
 *   packed, packed + n_q dim, in one call (the backward takes the same two pointers).
 */
size_t ccr_pool_ce_workspace_bytes(int n_q, int n_c, int dim);
int ccr_pool_ce_fwd(const uint16_t *Q, const uint16_t *C, const int32_t *label, const float *weight, int n_q, int n_c, int dim,
                    float inv_temperature, float *out3, float *lse, void *workspace, size_t ws_bytes, void *stream);
int ccr_pool_ce_fwd_f32(const float *q, const float *c, const int32_t *label, const float *weight, int n_q, int n_c, int dim,
                        float inv_temperature, uint16_t *packed, float *out3, float *lse, void *workspace, size_t ws_bytes,
                        void *stream);
int ccr_pool_ce_bwd_dev(const uint16_t *Q, const uint16_t *C, const int32_t *label, const float *weight, const float *lse, int n_q,
                        int n_c, int dim, float inv_temperature, const float *grad_out_dev, const float *W_dev, float *dQ, float *dC,
                        void *workspace, size_t ws_bytes, void *stream);

/*
 * The "bpr" objective of _BertBPR.training_and_validation_step (src/ccrec/models/bbpr.py:153-185).
 *
 * ccr_bpr_sample -- prior-guided negative sampling.  Replaces bbpr.py:160-179:
 *   torch.multinomial((training_prior_fcn(prior[i].to_dense()) + item_proposal.log()).softmax(1), n_negatives, True).T
 * without the dense [B][n_items] matrix.  All pointers DEVICE.
 *   users [B] int64: the batch's rows of the prior.  prior CSR over all users: prior_ptr [n_users + 1] int64, prior_idx int64
 *   ascending and unique per row, prior_t fp32 = training_prior_fcn(value), ALREADY applied; t0 = training_prior_fcn(0), the value of
 *   every absent entry.  prior_ptr = NULL: the no-prior branch (bbpr.py:176-179), draws from the proposal alone.
 *   proposal [n_items] fp32 > 0; proposal_cdf [n_items] fp64 = its inclusive prefix sums; uniforms [n_neg][B] fp64 in [0, 1).
 *   In fp64, for the row's entries (c_1 < ... < c_m; t_1 ... t_m):  M = max(t0, max t_k), e0 = exp(t0 - M), e_k = exp(t_k - M),
 *     F(j) = e0 cdf[j] + sum_{k: c_k <= j} proposal[c_k] (e_k - e0),   Z = F(n_items - 1)
 *   out_nj[n][b] = the smallest j with F(j) > uniforms[n][b] Z: the inverse CDF of the softmax (its max-shift included, so
 *   training_prior_fcn values of 1e5 do not overflow).  out_nj [n_neg][B] int64, laid out as multinomial(...).T is.
 *   max_row_nnz (HOST): the longest row of the CSR; above 4096 (the limit of ccr_search_sparse_prior): CCR_ERR_INVALID.  A user
 *   outside [0, n_users) or a row longer than max_row_nnz gives -1 for every draw of that batch row (checked on the device).
 *   With replacement only.  One launch, one wave per batch row; the same uniforms give the same draws.
 *
 * ccr_bpr_frozen_* -- the loss of one step when the encoder is frozen and every item's CLS row is cached (all_cls, bbpr.py:436-438):
 * gather -> LayerNorm -> _pairwise products -> logsigmoid -> weighted sum (bbpr.py:144-147, 180-185) in one pass over the rows.
 *   table [n_rows][dim] fp32; gamma, beta [dim] fp32 and eps: the LayerNorm (biased variance, as torch); gamma and beta may both
 *   be NULL (elementwise_affine=False: forward only).  ptr_i, ptr_j [B], ptr_nj [n_neg][B] int64 rows of the table; w [B] fp32.
 *     e = LN(table[ptr]) gamma + beta;   D_nb = e_i . e_j - e_i . e_nb;   loss = sum_nb w_b softplus(-D_nb) / (n_neg sum_b w_b)
 *   fwd: out3 [3] fp32 = {loss, numerator, denominator n_neg sum w}.  bwd: dgamma, dbeta [dim] fp32 (the table is a buffer: no
 *   gradient) = grad_out_dev[0] times the gradient of numerator / den_dev[0] (den_dev: out3 + 2 of the forward); the rows are
 *   read and normalised again, the forward saves nothing.  Both scalars are read on the device: no host synchronisation.
 *   All fp32; softplus and sigmoid in their overflow-free forms (|D| in the hundreds is fine).  sum w = 0 gives NaN; a pointer
 *   outside [0, n_rows) gives a NaN loss and NaN gradients (checked on the device, every address clamped).  Deterministic: no
 *   atomics, fixed summation order.  dim % 64 == 0, dim <= 2048, B <= 2^20, n_neg <= 4096; anything else: CCR_ERR_INVALID, and
 *   ccr_bpr_frozen_workspace_bytes returns 0 with a ccr_last_error() text.  table, gamma, beta, dgamma, dbeta 16-byte aligned.
 *   workspace: ccr_bpr_frozen_workspace_bytes(B, n_neg, dim) bytes (DEVICE), scratch for either call.
 *   Launches: forward 2 (one wave per batch row; finish), backward 2 (one wave per batch row; fixed-order sum of the partial rows).
 */
int ccr_bpr_sample(const int64_t *users, int B, int n_neg, int64_t n_users, const int64_t *prior_ptr, const int64_t *prior_idx,
                   const float *prior_t, float t0, const float *proposal, const double *proposal_cdf, int n_items,
                   const double *uniforms, int max_row_nnz, int64_t *out_nj, void *stream);
size_t ccr_bpr_frozen_workspace_bytes(int B, int n_neg, int dim);
int ccr_bpr_frozen_fwd(const float *table, int64_t n_rows, int dim, const float *gamma, const float *beta, float eps,
                       const int64_t *ptr_i, const int64_t *ptr_j, const int64_t *ptr_nj, const float *w, int B, int n_neg,
                       float *out3, void *workspace, size_t ws_bytes, void *stream);
int ccr_bpr_frozen_bwd_dev(const float *table, int64_t n_rows, int dim, const float *gamma, const float *beta, float eps,
                           const int64_t *ptr_i, const int64_t *ptr_j, const int64_t *ptr_nj, const float *w, int B, int n_neg,
                           const float *den_dev, const float *grad_out_dev, float *dgamma, float *dbeta, void *workspace,
                           size_t ws_bytes, void *stream);

/*
 * Reciprocal rank / hit counts of every query at several cut-offs, from the id tensor of ccr_search.
 * Replaces: EvaluateRetrieval.evaluate_custom(qrels, ranking_profile, [1,5,10,100], metric="mrr")
 * (scripts/al_0_rank.py:130-133) and its python-dict traversal; the caller averages over queries.
 *   ids [n_q][k] int64 (rank order); qrel_ptr [n_q+1], qrel_idx ascending per query (relevant ids, score > 0);
 *   k_values [n_k] int32 (n_k <= 16); out_rr [n_q][n_k] fp32; out_hits [n_q][n_k] int32.
 */
int ccr_rank_metrics(const int64_t *ids, int n_q, int k, const int64_t *qrel_ptr, const int64_t *qrel_idx,
                     const int32_t *k_values, int n_k, float *out_rr, int32_t *out_hits, void *stream);

/*
 * BM25 as a sparse scorer (the lexical leg of the candidate builder).
 * Replaces: BM25.transform, scripts/bm_25.py:31-52 (scipy on the host, one query at a time) and the per-query full
 * sort + keep 1001 of ranking_bm25, scripts/ms_marco_eval.py:165-186.
 *   index  = term-major postings of the count matrix: indptr [n_terms + 1] (HOST), doc_ids [nnz] int32 -- STRICTLY ASCENDING
 *            inside a term (scipy's sorted CSC; the scorer walks every list with a cursor) and inside [0, n_docs): checked by
 *            ccr_bm25_index_create in one pass over the postings (CCR_ERR_INVALID names the first violation) -- and tf [nnz] fp32 (DEVICE,
 *            borrowed), doc_k [n_docs] fp64 (DEVICE, borrowed) = k1 * (1 - b + b * len_d / avdl)
 *   query  = CSR on the HOST: q_ptr [n_q + 1], q_terms strictly ascending term ids, q_idf = ln(n / df_t) per entry
 *   score(q, d) = sum_t ascending (tf * idf_t) * (k1 + 1) / (tf + doc_k[d]) in fp64, rounded once to fp32;
 *   out_scores / out_ids [n_q][k] in the order (score desc, document index asc); documents without any query term
 *   score 0 and follow in index order, as a stable sort of the reference's dense score vector would leave them.
 *   Queries of up to 256 distinct terms run the document-tile scorer (fp64 accumulators in LDS; one cursor group per lane up to 64 terms,
 *   four up to 256); from ~30 k documents up the top-k
 *   filter is fused into it (a sampled threshold per query, the documents that pass leave the tile's registers as candidate records,
 *   verified; rows the filter cannot finish are scored again with their fp32 rows stored and ranked exactly), so no [n_q][n_docs]
 *   score row exists and the workspace is ~130 KiB per query + 1 GiB.  Smaller corpora and CCR_BM25_DENSE_SELECT=1 store the fp32 rows
 *   (~8 GiB per batch) and rank them exactly; a call with a longer query runs the round kernels (fp64 rows in the workspace): same
 *   bits on every path.  CCR_BM25_TILE=-1 (read at ccr_bm25_index_create) forces the round kernels.
 *   ccr_bm25_search_workspace_bytes_k sizes the workspace for one k; ccr_bm25_search_workspace_bytes for any k (the larger layout).
 */
typedef struct ccr_bm25_index ccr_bm25_index;
int ccr_bm25_index_create(const int64_t *indptr_host, const int32_t *doc_ids, const float *tf, const double *doc_k,
                          int64_t n_terms, int64_t n_docs, double k1, ccr_bm25_index **out);
int ccr_bm25_index_destroy(ccr_bm25_index *index);
/* Optional, once per index: the idf of every term (HOST, [n_terms]; BM25.fit's ln(n / df), scripts/bm_25.py:21-29) -> a table of the
 * FINISHED contribution of every posting, contrib [nnz] fp64 (DEVICE, caller-owned, filled here; must outlive the index):
 * (tf idf_t)(k1 + 1) / (tf + doc_k[d]) by the scorer's own operations, so the same bits.  A search whose q_idf entries all equal this
 * idf bit for bit streams 12 bytes per posting and adds -- no doc_k gather, no fp64 division; any other search runs as before. */
int ccr_bm25_index_set_idf(ccr_bm25_index *index, const double *idf_host, double *contrib, void *stream);
size_t ccr_bm25_search_workspace_bytes(const ccr_bm25_index *index, int n_q, int max_terms_per_query);
size_t ccr_bm25_search_workspace_bytes_k(const ccr_bm25_index *index, int n_q, int max_terms_per_query, int k);
/* of the index's last search: out4 = {path: 0 round kernels + stored rows, 1 tile scorer + stored rows, 2 tile scorer + fused filter, + 4 if
 * the contribution table was used;
 * rows the filter could not finish (scored again and ranked exactly); batches; rank of the sampled threshold} */
int ccr_bm25_search_last_stats(const ccr_bm25_index *index, int64_t *out4);
int ccr_bm25_search(const ccr_bm25_index *index, const int64_t *q_ptr_host, const int32_t *q_terms_host,
                    const double *q_idf_host, int n_q, int k, float *out_scores, int64_t *out_ids, void *workspace,
                    size_t ws_bytes, void *stream);

/*
 * One AdamW step over a list of fp32 parameter tensors in a single pass, which also keeps 16-bit copies of the new values current
 * (the weight set FusedBertEncoder's layer kernels read: no forward casts a weight again).
 * Replaces: torch.optim.AdamW of configure_optimizers (src/ccrec/models/bert_mt.py:115-146).
 *   segments  HOST array, one entry per tensor: param / grad / exp_avg / exp_avg_sq fp32 [n] (DEVICE, contiguous), shadow = NULL or a
 *             16-bit buffer [n] (DEVICE; may be a row block of a larger tensor) of type shadow_dtype (0 none, 1 bf16, 2 fp16).
 *             decay = 1 - lr * wd, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t): formed in double by the caller from the
 *             tensor's own 1-based step count t and rounded once to fp32.
 *   per element, every operation fp32, round to nearest, not contracted, divide and square root correctly rounded:
 *     p1 = p * decay;  m' = m + w1 * (g - m);  v' = v * beta2 + (w2 * g) * g;  d = sqrt(v') / bc2_sqrt + eps;
 *     p' = p1 - step_size * (m' / d);  shadow = p' rounded to nearest even      (w1 = one_minus_beta1, w2 = one_minus_beta2)
 *   16-byte accesses where all four fp32 pointers of a segment sit on 16-byte boundaries (and the shadow on an 8-byte one), 4-byte
 *   accesses otherwise and on the last n % 4 elements.  The list is walked on the host and travels in the kernel arguments, 48 segments
 *   per launch: no device table, no copy, no allocation, no host wait.  n_segments == 0 and segments with n == 0 ask for nothing;
 *   n < 0, a NULL pointer of a non-empty segment or an unknown shadow_dtype: CCR_ERR_INVALID before anything is launched.
 */
typedef struct ccr_adamw_segment {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    void *shadow;
    int64_t n;
    float decay, step_size, bc2_sqrt;
    int32_t shadow_dtype;
} ccr_adamw_segment;
int ccr_adamw_step(const ccr_adamw_segment *segments, int n_segments, float one_minus_beta1, float beta2, float one_minus_beta2,
                   float eps, void *stream);

/*
 * Loss scaling, overflow skip and global-norm clipping inside the AdamW step (library version 110; opt-in: ccr_adamw_step is unchanged).
 * Replaces: the GradScaler that Lightning's Trainer(precision=16) puts around the optimizer (src/ccrec/models/bert_mt.py:314,
 * src/ccrec/models/bbpr.py:433) -- unscale_'s pass over every gradient, clip_grad_norm_'s two passes and the host read of found_inf.
 * Three calls on one stream: ccr_grad_stats (read only) -> ccr_adamw_control_update (one workgroup) -> ccr_adamw_step_scaled.
 *
 * ccr_adamw_control: 64 bytes of DEVICE memory, written by ccr_adamw_control_update, read by ccr_adamw_step_scaled.
 *   coef            the multiplier of every gradient: inv * min(1, max_norm / (norm + 1e-6f))
 *   skip            1: the step writes nothing
 *   norm            the UNSCALED global L2 norm of the gradients (what clip_grad_norm_ returns)
 *   scale           the loss scale (read and updated only with own_scale)
 *   growth_tracker  unskipped steps since the scale last changed (own_scale only)
 *   skipped_total   skipped steps so far (every mode)
 *
 * ccr_grad_stats: partials[c] = the fp32 sum of g * g over chunk c, c counting the 4096-element chunks of the non-empty segments in
 *   list order (ccr_adamw_step's chunks; only `grad` and `n` of a segment are read, the other pointers decide the access width as
 *   there).  No atomics, one fixed order whatever the access width: the element at offset j of its chunk belongs to thread (j / 4) % 256,
 *   which adds its squares in increasing j to a sum that starts at +0 (fp32, the square rounded, not contracted); the 64 sums of a wave
 *   fold as x[i] + x[i + h] for h = 32, 16, 8, 4, 2, 1; the four wave sums add as ((w0 + w1) + w2) + w3.
 *   ccr_grad_stats_workspace_bytes: 4 bytes per chunk (0 for an empty list, -1 for an ill-formed one).
 *
 * ccr_adamw_control_update: s = the sum of partials[0 .. n_partials) in double, in index order within 256 equal contiguous slices
 *   (slice t = indices [t * ceil(n / 256), ...)), then the slice sums in slice order; both start at +0.
 *   inv  = (float)(1 / (double)scale), scale = *ext_grad_scale if that is not NULL, else control->scale if own_scale, else inv = 1
 *   skip = s is not finite, or ext_found_inf != NULL and *ext_found_inf != 0.  A non-finite s covers a NaN, either infinity AND a finite
 *          gradient whose square passes fp32's range (|g| > 1.8e19): all three skip the step.  Squares cannot cancel.
 *   norm = (float)sqrt(s) * inv;  coef = inv * min(1, max_norm / (norm + 1e-6f)) in fp32 (torch's clip_grad_norm_); the clip factor is
 *          exactly 1 when max_norm is not positive, infinite or a NaN.
 *   own_scale (torch's _amp_update_scale_): on a skip scale *= backoff, growth_tracker = 0; else growth_tracker += 1 and, when it reaches
 *          growth_interval, scale *= growth if that product is finite, growth_tracker = 0.  As there, a product is formed in double
 *          from the double factor and rounded to fp32 once.  skipped_total += 1 on every skip.
 *   ext_grad_scale / ext_found_inf: NULL or fp32 DEVICE scalars, a stock torch.amp.GradScaler's; the block's own scale is then left
 *          alone (own_scale together with ext_grad_scale: CCR_ERR_INVALID).
 *
 * ccr_adamw_step_scaled: ccr_adamw_step with g replaced by g * control->coef (one fp32 multiply, rounded, not contracted); every
 *   workgroup reads control->skip first and, if it is set, returns without a store: p, exp_avg, exp_avg_sq and the shadow keep their
 *   bytes.  With coef == 1.0f and skip == 0 every stored bit is ccr_adamw_step's.
 */
typedef struct ccr_adamw_control {
    float coef;
    int32_t skip;
    float norm;
    float scale;
    int32_t growth_tracker;
    int32_t skipped_total;
    uint32_t reserved[10];   /* zero */
} ccr_adamw_control;
int64_t ccr_grad_stats_workspace_bytes(const ccr_adamw_segment *segments, int n_segments);
int ccr_grad_stats(const ccr_adamw_segment *segments, int n_segments, float *partials, void *stream);
int ccr_adamw_control_update(ccr_adamw_control *control, const float *partials, int64_t n_partials, float max_norm, int own_scale,
                             double growth, double backoff, int growth_interval, const float *ext_grad_scale, const float *ext_found_inf,
                             void *stream);
int ccr_adamw_step_scaled(const ccr_adamw_segment *segments, int n_segments, float one_minus_beta1, float beta2, float one_minus_beta2,
                          float eps, const ccr_adamw_control *control, void *stream);

/*
 * The fine-tune step in one packed pass (library version 108): the embedding block with a backward, and mean pooling over a packed token
 * array with a backward.  The reference encodes queries, positives and negatives in three tower calls per step
 * (src/ccrec/models/bbpr.py:195-197) and pools the last hidden state under its mask (src/ccrec/models/item_tower.py:141-146); with these
 * four entry points no piece of that step runs outside the library's kernels, and every gradient is bit-identical from run to run (no
 * atomics on floating-point data).
 * ccr_embed_layernorm_train_half (bbpr.py:195-197: BertEmbeddings.forward in train()): ccr_embed_layernorm_half's arguments and
 *   arithmetic -- (word + type) + position, the two-step mean, one fma with gamma and beta -- followed by the block's dropout,
 *   y * (keep ? inv_keep : 0) exactly as ccr_dropout_apply forms it, from bits [rows][dim / 32] (ccr_dropout_bits_rows' layout).
 *   bits == NULL: no dropout (inv_keep is ignored) and the outputs are ccr_embed_layernorm_half's; with all-ones bits and inv_keep = 1
 *   likewise.  Either output may be NULL.  Ids outside a table are clamped.
 * ccr_embed_layernorm_bwd_half (bbpr.py:195-197: loss.backward() through BertEmbeddings): from the forward's tables, index vectors,
 *   gamma, eps, bits and inv_keep, and d_y [rows][dim] fp32 = the summed gradient of both outputs: d_v = d_y * keep * inv_keep; v, mean
 *   and rstd are recomputed with the forward's bits; d_x [rows][dim] fp32 = rstd * (g - mean(g) - xhat * mean(g * xhat)) with
 *   g = d_v * gamma is the gradient of every gathered table row; d_gamma = sum_rows d_v * xhat and d_beta = sum_rows d_v, [dim] fp32.
 *   Any of the three may be NULL.  Nothing 16-bit is read or written (the name pairs it with its forward).
 *   workspace (DEVICE, 16-byte aligned), needed when d_gamma or d_beta is asked for: min((rows + 3) / 4, 512) * 2 * dim * 4 bytes
 *   (per-workgroup column sums, at most 512 rows of them, added up by a second kernel in a fixed order); NULL / 0 otherwise;
 *   CCR_ERR_WORKSPACE if it is smaller.
 * ccr_embedding_grad (bbpr.py:195-197: the gradient of word_embeddings / position_embeddings / token_type_embeddings .weight):
 *   grad [n_rows][dim] fp32 from d_x [T][dim] fp32 and idx [T]: grad[r] = the sum of d_x[row] over the rows whose id, clamped to
 *   0 .. n_rows - 1 as the forward clamps it, is r.  order [T] = the permutation that sorts (clamped idx, row) ascending (DEVICE; values
 *   outside 0 .. T - 1 are clamped, an order that does not sort gives unspecified sums).  EVERY row of grad is written: ids that do not
 *   occur get +0, so the caller needs no memset.  The summation order is normative: the rows of one id, in ascending row order, are cut
 *   into chunks of CCR_EMBED_GRAD_CHUNK consecutive entries; a chunk is summed sequentially in fp32 starting from its first entry; the
 *   chunk sums are then added sequentially, in order.  ccrec_amd/embed_grad_ref.py restates it in numpy, bit for bit.  Long runs (type 0
 *   holds every token) are spread over many workgroups.  dim % 4 == 0, 16-byte aligned d_x and grad, T < 2^31; T == 0 gives all +0.
 * ccr_meanpool_bwd_packed (item_tower.py:141-146 under autograd, over a packed token array): rows seq_start[s] .. + seq_len[s] - 1 of
 *   d_hidden [T][dim] (hidden_dtype: CCR_DTYPE_F32 / F16 / BF16) receive grad[s] / (float)seq_len[s], grad [n_seq][dim] fp32 -- the
 *   division of ccr_meanpool_bwd, hence the bits of the padded form's real rows.  Rows that belong to no sequence are LEFT ALONE (there
 *   is no padding to zero); a sequence of length <= 0 writes nothing.  dim % 4 == 0.
 */
#define CCR_EMBED_GRAD_CHUNK 64
int ccr_embed_layernorm_train_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                   const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                   const int64_t *token_types, const float *gamma, const float *beta, float eps, const uint32_t *bits,
                                   float inv_keep, float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype, void *stream);
int ccr_embed_layernorm_bwd_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                 const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                 const int64_t *token_types, const float *gamma, float eps, const uint32_t *bits, float inv_keep,
                                 const float *d_y, float *d_x, float *d_gamma, float *d_beta, int64_t rows, int dim, void *workspace,
                                 size_t workspace_bytes, void *stream);
int ccr_embedding_grad(const int64_t *idx, const int64_t *order, const float *d_x, int64_t T, int dim, float *grad, int64_t n_rows,
                       void *stream);
int ccr_meanpool_bwd_packed(const float *grad, const int32_t *seq_start, const int32_t *seq_len, void *d_hidden, int hidden_dtype, int n_seq,
                            int dim, void *stream);

/*
 * Ranking on the fp32 embeddings (library version 111; opt-in: no other entry point changes).  The reference's CPU path ranks fp32 scores
 * (scripts/ms_marco_eval.py:204-230); every search here ranks the rows after they were rounded to 16 bits.  These two entry points give
 * the fp32 ranking on top of the 16-bit search, with a proof per query (DESIGN.md 2.1;
 * ccrec_amd/rank_f32_ref.py restates both in numpy, bit for bit).
 * ccr_keep_f32: beside rows that are ALREADY packed (half_rows [rows][pdim], pdim = dim rounded up to a multiple of 8, half_dtype =
 *   CCR_DTYPE_BF16 / F16) keep the fp32 rows the pack rounded: dst_f32 [rows][pdim] = src [rows][dim] zero-padded, with normalize the
 *   value (float)((double) x_i / max(sqrt(ss), 1e-12)) of the normalising pack (the same sum of squares in the same order), so that
 *   rounding dst_f32 gives half_rows bit for bit.  res_bounds [rows] >= ||dst_f32[r] - half_rows[r]||_2: the fp64 norm, inflated by
 *   1 + 2^-20 and rounded UP to fp32.  One pass over the shard, a wave per row.
 * ccr_rescore_f32: one workgroup per query.  cand_ids / cand_s16 [n_q][n_cand]: the first n_cand results of the 16-bit search (GLOBAL
 *   ids = row + id_offset, canonical 16-bit scores, in that search's rank order).  Each candidate is re-scored on the fp32 rows,
 *   s32 = (float) sum_i ascending fma((double) q_i, (double) d_i, acc); an entry whose cand_s16 is exactly -1e6f (a blocked row) keeps
 *   -1e6.  out_scores / out_ids [n_q][k]: the k best by (s32 desc, id asc).  flags [n_q]: 0 = verified, no row outside the list can
 *   belong to -- or tie with -- the fp32 top-k; 1 = not verified (fetch more rows).  With tau = out_scores[q][k - 1],
 *   cut = cand_s16[q][n_cand - 1], A = q_norm_bounds[q] >= ||query row||, r = q_res_bounds[q] (the query's own ccr_keep_f32 bound),
 *   corpus_max = {Rmax, Nmax} (DEVICE: the maxima of the corpus's res_bounds and of its packed rows' norm bounds), in fp64:
 *     E = A * Rmax + r * Nmax,   slack = 2^-21 (|cut| + |tau|) + 2^-40 A (Nmax + Rmax),
 *     verified <=> n_cand == n_rows  or  cut == -1e6f  or  cut + E + slack < tau.
 *   A candidate id outside [id_offset, id_offset + n_rows) is not read and leaves its query unverified.
 *   workspace (DEVICE, 16-byte aligned, ccr_rescore_f32_workspace_bytes; 0 = the shape was refused): on return {tau, cut, E, slack} as
 *   4 floats per query.  CCR_ERR_INVALID on k > n_cand, n_cand > 4096, n_cand > n_rows, pdim % 8 != 0 or > 4096, or a null pointer: no
 *   output is touched.
 */
int ccr_keep_f32(const float *src, const uint16_t *half_rows, int half_dtype, int normalize, float *dst_f32, float *res_bounds, int64_t rows,
                 int dim, void *stream);
size_t ccr_rescore_f32_workspace_bytes(int n_q, int n_cand, int k, int pdim);
int ccr_rescore_f32(const float *queries_f32, const float *corpus_f32, int64_t n_rows, int pdim, const int64_t *cand_ids,
                    const float *cand_s16, int n_q, int n_cand, int k, int64_t id_offset, const float *q_norm_bounds,
                    const float *q_res_bounds, const float *corpus_max, float *out_scores, int64_t *out_ids, int32_t *flags, void *workspace,
                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CCR_RETRIEVAL_H */
