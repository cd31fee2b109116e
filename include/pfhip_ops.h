/*
 * pfhip_ops.h — operator-level C ABI over the same gfx950 kernels that pfhip_offline_forward launches.
 * Device pointers in, device pointers out, asynchronous on `stream` (hipStream_t, NULL = default).
 * Exists so that each kernel can be parity-tested and timed in isolation against the oracle; every
 * entry names the node of the reference graph it stands for (the graph itself is the opaque
 * `m_session_->Run`, onnxruntime/src/paraformer.cpp:541; architecture per SURVEY.md appendix A).
 * All return 0 on success, a hipError_t value otherwise.
 */
#ifndef PFHIP_OPS_H_
#define PFHIP_OPS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* MatMul/Gemm (+Add bias, +residual Adds, Relu): C[M,N] = A[M,K] W[N,K]^T ...; guard=1 bounds-checks. */
int pfhip_op_gemm_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                      const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu,
                      int guard, void* stream);
/* Same, with the kernel forced: kind 0 = by size (as above), 1 = 128x128 tiled, 2 = weight-streaming (M-small) kernel,
 * 3 = 64x128 tiled; 4 / 5 / 7 = bf16 three-plane kernels (256x128, 128x128, 64x128 tile); 8 / 9 / 10 = fp16 two-plane kernels. */
int pfhip_op_gemm_f32_kind(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                           const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu,
                           int guard, int kind, void* stream);
/* Same; w_scale = the power-of-two scale the fp16 two-plane kernels (kinds 8 / 9 / 10, and kind 0 by default) stage W with:
 * pfhip_op_best_w_scale(max |W|) keeps max |W| * w_scale <= 32768 (the model does this per weight matrix at load). */
int pfhip_op_gemm_f32_scaled(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                             const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int relu,
                             int guard, int kind, float w_scale, void* stream);
float pfhip_op_best_w_scale(float max_abs);
/* The launch context of the calling thread's later operator calls (csrc/kernels.h LaunchCtx): range_flag = a device word the
 * LayerNorm-folding kernels OR into when a row leaves the fp16 two-plane domain (one word per launch, not per row; the caller
 * clears and reads it), exact != 0 = every split-operand launch on the bf16 three-plane kernels.  (NULL, 0) restores the default. */
int pfhip_op_set_launch_ctx(int* range_flag, int exact);
/* The product path's in-loop-split GEMM with the LayerNorm hand-off (launch_gemm_f32_x6_ln: gemm_x3.hip by default, gemm_x6.hip under
 * `exact`; tile height by grid size as the model's launches): fp32 A [M, K], W [N, K], K % 32 == 0, row strides % 4 == 0.
 * ln_stats != NULL: LayerNormalization folded in — A is the raw row, W / bias the gamma / beta-folded ones, ln_colsum[n] =
 * sum_k W'[n][k], ln_stats [M][ln_tiles][2] the (mean, sum of squared deviations) pairs per 128 columns of A; eps = 1e-12.
 * stats_out != NULL (N % 128 == 0): the same pairs of the result, [M][N / 128][2]. */
int pfhip_op_gemm_f32_ln(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias, const float* R1, int ldr1,
                         const float* R2, int ldr2, int M, int N, int K, int relu, const float* ln_stats, int ln_tiles,
                         const float* ln_colsum, float* stats_out, float w_scale, void* stream);
/* Pre-split operands (csrc/gemm_p3.hip): plane images — two fp16 planes of an fp32 matrix, [K/16][rows][16] with the 16-byte halves
 * of a row swapped where row bit 3 is set; rows a multiple of 128 — and the GEMM that consumes and produces them:
 * C = A W^T (x 1 / w_scale, LayerNorm-fold finish, +bias, +R1, ReLU) as fp32 (C != NULL) and / or as plane images (Ph / Pl != NULL).
 * tile_rows: 0 = by grid size, 64 / 128 = that tile height (the results are bit-identical). */
size_t pfhip_op_plane_image_bytes(int rows, int K);
int pfhip_op_split_planes(const float* X, int ld, int rows_valid, int rows, int K, float scale, void* hi, void* lo, void* stream);
int pfhip_op_gemm_p3(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                     void* Ph, void* Pl, int rows_p, const float* bias, const float* R1, int ldr1, int M, int N, int K, int relu,
                     const float* ln_stats, int ln_tiles, const float* ln_colsum, float* stats_out, int tile_rows, void* stream);
/* The same with a tile-width selector.  tile_cols: 0 = as pfhip_op_gemm_p3; 256 = the 256 x 256 tile (one persistent workgroup per CU;
 * bit-identical results), which serves the LayerNorm-folded forms with ONE output (C or the plane images, not both), no residual, no
 * stats_out, N % 256 == 0, tile_rows 0 — anything else is refused with hipErrorInvalidValue and launches nothing. */
int pfhip_op_gemm_p3_cols(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                          void* Ph, void* Pl, int rows_p, const float* bias, const float* R1, int ldr1, int M, int N, int K, int relu,
                          const float* ln_stats, int ln_tiles, const float* ln_colsum, float* stats_out, int tile_rows, int tile_cols,
                          void* stream);
/* How many pfhip_op_gemm_p3* / model launches of this process the 256 x 256 tile has served (tests of the default dispatch, probes). */
long pfhip_op_gemm_p3_wide_launches(void);
/* LayerNormalization over the last axis. */
int pfhip_op_layernorm(const float* x, int ldx, float* y, int ldy, const float* g, const float* b, int M, int D,
                       int Dout, float eps, void* stream);
/* FSMN memory block: depthwise Conv1d k=11 over time + identity (+residual), per utterance segment. */
int pfhip_op_fsmn(const float* v, int ldv, const float* w, const float* res, int ldres, float* out, int ldo,
                  const int* off, const int* len, int B, int max_len, int C, void* stream);
/* The same with the window shifted into the past by `shift` frames (sanm_shfit; the online CT-Transformer's layers): taps over
 * [t - 5 - shift, t + 5 - shift].  hipErrorInvalidValue, before anything is launched, for a shift other than 0 or 5 (5 = causal),
 * C % 4 != 0, a NULL buffer (res may be NULL), a row stride below C or not a multiple of 4. */
int pfhip_op_fsmn_shift(const float* v, int ldv, const float* w, const float* res, int ldres, float* out, int ldo,
                        const int* off, const int* len, int B, int max_len, int C, int shift, void* stream);
/* MatMul-Softmax-MatMul of one attention block, d_k = 128. */
int pfhip_op_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                       const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                       int max_q_len, float scale, void* stream);
/* Same, head dimension 32, 80 or 128 chosen at run time (CT-Transformer: 256 / 8 heads; the small Paraformer: 320 / 4 heads).
 * hipErrorInvalidValue for any other width, before anything is launched. */
int pfhip_op_attention_hd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                          const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                          int max_q_len, float scale, int head_dim, void* stream);
/* pfhip_op_attention_hd with a per-query key limit, what the 256-wide online CT-Transformer launches in every layer (the masked branch
 * of attention.hip's fp32-MFMA kernel at every segment length): q_kv_limit [packed query rows] = the number of keys the row may see
 * (CTTransformerOnline::VadMask), >= 1 — the result of a row that may see no key is undefined.  hipErrorInvalidValue, before anything
 * is launched, for a head width other than 32, 80 or 128, H < 1, a NULL buffer, a row stride below H * head_dim or not a multiple of 4. */
int pfhip_op_attention_limit(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                             const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                             int max_q_len, float scale, int head_dim, const int* q_kv_limit, void* stream);
/* The same block for any head width 1 <= d_k <= 64 (the exact-width form of attention.hip's kernel; the large CT-Transformer:
 * 516 / 12 heads = 43), fp32, head h in columns [h * d_k, (h + 1) * d_k) of a row: no other column is read or written.  q_kv_limit: nullptr, or per packed query row the
 * number of keys it may see (CTTransformerOnline::VadMask).  hipErrorInvalidValue, before anything is launched, for d_k < 1,
 * d_k > 64, H < 1 or a leading dimension below H * d_k. */
int pfhip_op_attention_dk(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                          const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                          int max_q_len, float scale, int d_k, const int* q_kv_limit, void* stream);
/* The encoder layer's pair on one set of self-attention segments (off / len): the SAN-M memory block of V into mem (pfhip_op_fsmn
 * without a residual) and the attention block's context into O as fp32 rows.  ONE launch — the memory block runs in front of the
 * attention kernel's key loop — where pfhip_op_attention_fsmn_is_fused(max_len, head_dim) says so; then, and only then,
 * mem_accumulate adds the memory into mem instead of overwriting it.  Otherwise pfhip_op_fsmn followed by pfhip_op_attention_hd.
 * head_dim 80 or 128. */
int pfhip_op_attention_fsmn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, const int* off,
                            const int* len, int B, int H, int max_len, float scale, const float* fsmn_w, float* mem, int ldmem,
                            int mem_accumulate, int head_dim, void* stream);
int pfhip_op_attention_fsmn_is_fused(int max_len, int head_dim);
/* The same block (d_k = 128, attention_x3.hip) with the context written as the two fp16 plane images that pfhip_op_gemm_p3 takes as
 * its A operand ([K / 16][plane_rows][16] per plane, K = H * 128; row = q_off[b] + t) instead of fp32 rows: the encoder's
 * attention -> output-projection hand-off on large batches.  total_q_rows = the number of rows the offsets span (<= plane_rows,
 * plane_rows a multiple of 128). */
int pfhip_op_attention_planes(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, void* planes_hi, void* planes_lo,
                              int plane_rows, const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H,
                              int max_q_len, int total_q_rows, float scale, void* stream);
/* Row-major fp16 planes of an fp32 matrix: hi = fp16_rtz(x), lo = fp16_rn(x - hi), [rows][ldp] each (cols % 8 == 0). */
int pfhip_op_split_rows(const float* X, int ld, int rows, int cols, void* hi, void* lo, int ldp, void* stream);
/* The encoder's QKV projection on plane-image operands (pfhip_op_gemm_p3) whose result leaves in two forms: columns < q_cols as fp32
 * rows of C, columns >= q_cols (K | V) as row-major planes kv_hi / kv_lo [M][ldkv] (column n at element n - q_cols) — what
 * pfhip_op_attention_kvplanes stages by LDS-DMA.  q_cols % 128 == 0; tile_rows 0 / 64 / 128. */
int pfhip_op_gemm_p3_qkv(const void* Ah, const void* Al, int rows_a, const void* Wh, const void* Wl, int rows_w, float w_scale, float* C, int ldc,
                         void* kv_hi, void* kv_lo, int ldkv, int q_cols, const float* bias, int M, int N, int K, const float* ln_stats,
                         int ln_tiles, const float* ln_colsum, int tile_rows, void* stream);
/* MatMul-Softmax-MatMul (d_k = 128) with K and V given as row-major fp16 planes (attention_p3.hip: row stride ldkv elements, K at
 * column 0 and V at column v_col of each plane, head h in columns 128 h ..; total_kv_rows rows).  Context as fp32 rows (O) or as the
 * plane images of pfhip_op_attention_planes (planes_hi / planes_lo / plane_rows).  fsmn_w != NULL (self-attention): also the SAN-M
 * memory block of V into mem (+= when mem_accumulate).  Same arithmetic as pfhip_op_attention on the values hi + lo. */
int pfhip_op_attention_kvplanes(const float* Q, int ldq, const void* kv_hi, const void* kv_lo, int ldkv, int v_col, int total_kv_rows, float* O,
                                int ldo, void* planes_hi, void* planes_lo, int plane_rows, const int* q_off, const int* q_len,
                                const int* kv_off, const int* kv_len, int B, int H, int max_q_len, int total_q_rows, float scale,
                                const float* fsmn_w, float* mem, int ldmem, int mem_accumulate, void* stream);
/* CIF integrate-and-fire (onnxruntime/src/paraformer-online.cpp:301-327) + tail slot. */
int pfhip_op_cif(const float* hidden, int ldh, const float* alphas, const int* row_off, const int* len, int B, int D,
                 float threshold, float tail, float* stage, int* n_fires, int* token_num, void* stream);
/* The same scan by the sibling kernel that also records where each token fired: fire_frame[row_off[b] + b + j] = the step of
 * the scan in which fire j of utterance b happened (0..len[b]-1 = that LFR row, len[b] = the tail slot), laid out like stage's rows
 * ([sum len + B] ints).  Slots past n_fires[b] are not written.  stage, n_fires and token_num are pfhip_op_cif's bit for bit.
 * Refuses what pfhip_op_cif refuses, and a NULL fire_frame. */
int pfhip_op_cif_fires(const float* hidden, int ldh, const float* alphas, const int* row_off, const int* len, int B, int D,
                       float threshold, float tail, float* stage, int* n_fires, int* token_num, int* fire_frame, void* stream);
/* LogSoftmax + ArgMax (GreedySearch/FindMax, onnxruntime/src/paraformer.cpp:386-395, util.cpp:63-74). */
int pfhip_op_logsoftmax_argmax(const float* logits, int ldl, int ML, int V, float* logp, int32_t* ids, void* stream);
/* The same head with the k best columns of every row (topk.hip; beyond GreedySearch, which keeps only the arg-max): topk_ids /
 * topk_logp [M][k], larger logit first, equal logits smaller column first, so topk_ids[.., 0] == ids; a value equals the logp entry
 * of its column bit for bit.  logp may be NULL (the log-sum-exp is formed all the same).  hipErrorInvalidValue, before anything is
 * launched, for k outside 1..8, V < k, ldl < V, M < 0 or a NULL buffer other than logp. */
int pfhip_op_logsoftmax_topk(const float* logits, int ldl, int M, int V, int k, float* logp, int32_t* ids, int32_t* topk_ids,
                             float* topk_logp, void* stream);

/* The head of a CTC model (SenseVoiceSmall: the graph's ctc_lo MatMul + LogSoftmax and the per-frame arg-max of CTCSearch,
 * onnxruntime/src/sensevoice-small.cpp:331-337) WITHOUT the logits matrix (ctc_head.hip): X [M, K] fp32 (exactly M rows, K % 32 == 0,
 * row strides % 4 == 0), W [V, K] (exactly V rows), bias [V], w_scale as pfhip_op_gemm_f32_scaled.  ids [M] = arg-max column of
 * x W^T + bias (first maximum wins, std::max_element), logp_best [M] = that logit - log sum exp of the row, lse [M] (may be NULL) =
 * the log-sum-exp.  workspace: pfhip_op_ctc_head_workspace_bytes(M, V) bytes of device memory (per row and 128-column tile the
 * triple max / arg-max / sum of exp).  hipErrorInvalidValue, before anything is launched, for any other shape, a NULL buffer or a
 * short workspace. */
size_t pfhip_op_ctc_head_workspace_bytes(int M, int V);
int pfhip_op_ctc_head(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K,
                      int32_t* ids, float* logp_best, float* lse, void* workspace, size_t workspace_bytes, void* stream);
/* CTC collapse (CTCSearch's loop, sensevoice-small.cpp:340-347) for B utterances packed in frame_ids / frame_logp: utterance b owns
 * frames [row_off[b], row_off[b] + len[b]) (DEVICE arrays); frame t is kept when frame_ids[t] != blank and != frame_ids[t - 1] (the
 * first frame has no predecessor).  ids / tok_frame / tok_logp are [B][max_tokens]: the kept id, its 0-based frame in the utterance,
 * and frame_logp of that frame bit for bit (tok_frame, tok_logp and, with tok_logp NULL, frame_logp may be NULL).  token_num [B] =
 * the number of kept frames — the true count even above max_tokens, where the surplus is not stored.  A length of 0 gives 0. */
int pfhip_op_ctc_collapse(const int32_t* frame_ids, const float* frame_logp, const int* row_off, const int* len, int B, int blank,
                          int max_tokens, int32_t* ids, int32_t* tok_frame, float* tok_logp, int32_t* token_num, void* stream);
/* The number of frames one trip of the collapse kernel's scan covers (tests place lengths on both sides of it). */
int pfhip_op_ctc_collapse_chunk(void);
/* CTC forced alignment (ctc_align.hip), step 1: the emissions of the labels asked for, without the logits matrix.  Utterance b owns
 * rows [row_off[b], row_off[b] + len[b]) of X [., K] and the labels labels[lab_off[b] .. + n_lab[b]) (DEVICE arrays; e_off is int64).
 * E + e_off[b] is E_b [len[b]][n_lab[b] + 1], packed: E_b[t][j] = x_t . W[id_j] + bias[id_j] - lse[row_off[b] + t], where column 0 is
 * the blank (id `blank`) and column j is label j (1-based; the same id may occur in several columns).  The caller computes e_off (the
 * prefix sums of len * (n_lab + 1)) and the E_b must not overlap.  fp32 FMA arithmetic.  K % 32 == 0 and row strides % 4 == 0 as
 * pfhip_op_ctc_head; W [V, K] has exactly V rows.  Nothing outside X's rows of the utterance, W, bias or E_b is read or written: rows
 * are clamped to the utterance and a label outside 0 .. V - 1 is CLAMPED into it here (the model-level call refuses such a label on
 * the host).  hipErrorInvalidValue, before anything is launched, for any other shape, a blank outside 0 .. V - 1 or a NULL buffer. */
int pfhip_op_ctc_emissions(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* lse, const int* row_off,
                           const int* len, const int* lab_off, const int* n_lab, const int32_t* labels, const long long* e_off, int B,
                           int K, int V, int blank, float* E, void* stream);
/* The step between pfhip_op_ctc_collapse and the two alignment kernels when the GREEDY tokens are aligned with no host round trip
 * (pfhip_svs_forward_spans): token_num [B] is the collapse's (device), speech_len [B] the rows N_b each utterance is aligned against
 * (device; the host knows them before the forward).  n_lab[b] = max(token_num[b] - 4, 0) — the kept ids behind the four tags —,
 * lab_off[b] = b * maxT + 4, so that `labels` is the collapse's own ids [B][maxT], e_off[b] = the exclusive int64 prefix sum of
 * N_b * (n_lab[b] + 1), *total (may be NULL) = that sum over every b.  An utterance whose E_b would end beyond cap_floats gets
 * n_lab[b] = -1 (its e_off and the total are the sums all the same); pfhip_op_ctc_emissions leaves such an utterance unwritten and
 * pfhip_op_ctc_align answers it as infeasible.  token_num[b] > maxT or N_b < 0, which no collapse over maxT rows produces: n_lab -1 and
 * nothing added to the sums.  One workgroup of 256 threads, a block scan through LDS.  hipErrorInvalidValue, before anything is
 * launched, for B outside 0 .. 65535, maxT < 0, cap_floats < 0, B * maxT + 4 above INT_MAX or a NULL buffer other than total. */
int pfhip_op_ctc_greedy_plan(const int32_t* token_num, const int* speech_len, int B, int maxT, long long cap_floats, int* n_lab, int* lab_off,
                             long long* e_off, long long* total, void* stream);
/* Step 2: the best path through the CTC trellis of each utterance and the spans of its labels.  E / e_off / len / n_lab / labels /
 * lab_off as above (the label ids only decide which neighbours are the same label); e_floats = the floats of E.
 *   N = len[b] frames, labels y_1 .. y_L, states s = 0 .. 2 L: s even is the blank (column 0), s odd is label (s + 1) / 2.
 *   v_0[0] = E[0][0], v_0[1] = E[0][1] (L >= 1), every other state -inf.  For t >= 1: m = the largest of v_{t-1}[s], v_{t-1}[s-1]
 *   (s >= 1) and v_{t-1}[s-2] (s odd, s >= 3 and y_{(s+1)/2} != y_{(s-1)/2}), a later candidate replacing the running best only when
 *   strictly greater (stay, then 1, then 2); v_t[s] = m + E[t][column of s], one fp32 add.
 *   End state 2 L if v_{N-1}[2 L] >= v_{N-1}[2 L - 1], else 2 L - 1 (L = 0: state 0); score[b] = that value.  N = 0: score 0 for
 *   L = 0.  score -inf <=> infeasible (N < L + the number of equal neighbours; N = 0 with L > 0): every span of the utterance is
 *   -1 and the other utterances are served.  -inf emissions are legal.
 * tok_begin / tok_end / tok_logp [B][max_tokens] (tok_logp may be NULL): the first frame of the path in label j's state, one past the
 * last, and E[tok_begin][j + 1]; slots from n_lab[b] on hold -1 / -1 / -inf.  workspace: pfhip_op_ctc_align_workspace_bytes(e_floats)
 * bytes of device memory (one back-pointer byte per frame and state).  hipErrorInvalidValue, before anything is launched, for
 * max_tokens above pfhip_op_ctc_align_max_tokens() (the two score rows of 2 L + 1 states live in 64 KB of LDS: 4095), a short
 * workspace or a NULL buffer.  n_lab is device data: the caller, who wrote the labels, checks n_lab[b] <= max_tokens (ops.ctc_align
 * and pfhip_svs_align do, before the launch); the kernel answers an utterance that breaks it, or whose E_b leaves E, as infeasible. */
size_t pfhip_op_ctc_align_workspace_bytes(size_t e_floats);
int pfhip_op_ctc_align_max_tokens(void);
int pfhip_op_ctc_align(const float* E, const long long* e_off, size_t e_floats, const int* len, const int* n_lab, const int32_t* labels,
                       const int* lab_off, int B, int max_tokens, int32_t* tok_begin, int32_t* tok_end, float* tok_logp, float* score,
                       void* workspace, size_t workspace_bytes, void* stream);
/* pfhip_op_ctc_head with the k best columns of every row (ctc_head.hip; what CtcPrefixDecoder::CtcSearch's first prune, TopK of
 * onnxruntime/src/util.h:42-78, takes from a full log-softmax row — here without that row): 1 <= k <= 16, V >= k.  topk_ids /
 * topk_logp [M][k]: larger logit first, equal logits smaller column first; a value is that column's logit minus the row's
 * log-sum-exp.  ids, logp_best and lse are pfhip_op_ctc_head's on the same operands BIT FOR BIT (the same tile arithmetic; the
 * greedy kernel is its own instantiation and is untouched), topk_ids[.., 0] == ids and topk_logp[.., 0] == logp_best: a value is
 * formed as (logit - row maximum) - log(sum), which at rank 0 is logp_best's -log(sum) and never increases along a row.  Nothing of size [M][V] is written: per row and 128-column tile the
 * epilogue leaves the tile's k best (value, column) pairs beside the greedy triple, and the merge kernel selects k of tiles x k.
 * workspace: pfhip_op_ctc_head_topk_workspace_bytes(M, V, k).  hipErrorInvalidValue, before anything is launched, for k outside
 * 1..16, V < k, any shape pfhip_op_ctc_head refuses, a NULL buffer (lse may be NULL) or a short workspace. */
size_t pfhip_op_ctc_head_topk_workspace_bytes(int M, int V, int k);
int pfhip_op_ctc_head_topk(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int k,
                           int32_t* ids, float* logp_best, float* lse, int32_t* topk_ids, float* topk_logp, void* workspace,
                           size_t workspace_bytes, void* stream);
/* CTC prefix beam search with hotwords on the device (ctc_beam.hip): CtcPrefixDecoder::CtcSearch + CtcFinalizeDecode
 * (onnxruntime/src/ctc-prefix-decoder.cpp:157-299, PrefixScore of ctc-prefix-decoder.h:64-110) over rows of k best columns.
 * Utterance b owns rows [row_off[b], row_off[b] + len[b]) (DEVICE arrays; the ranges must not overlap) of topk_ids / topk_logp
 * [rows][k], a row's first `first_beam` columns being its candidates (expected distinct).  1 <= first_beam <= k <= 16,
 * 1 <= nbest <= second_beam <= 16, 0 <= blank < V.  graph: a pfhip_ctx_graph built for vocab == V, or NULL; the call copies it to
 * the front of the workspace on `stream`.
 *   A hypothesis is a token sequence with s (log-probability of the alignments ending in the blank), ns (of those ending in its
 *   last token), a context score and a context state.  Start: the empty sequence with s = 0, ns = -FLT_MAX ("no path"; not -inf).
 *   LogAdd(x, y) = the other operand where one is <= -FLT_MAX, else log(exp(x - m) + exp(y - m)) + m with m = max(x, y).
 *   Per row, for every hypothesis h and candidate (tok, p):  blank: h unchanged receives s <- LogAdd(s, LogAdd(s_h, ns_h) + p);
 *   tok == last token of h: h unchanged receives ns <- LogAdd(ns, ns_h + p), and h + tok receives ns <- LogAdd(ns, s_h + p);
 *   any other tok: h + tok receives ns <- LogAdd(ns, LogAdd(s_h, ns_h) + p).  An unchanged hypothesis keeps its context; h + tok
 *   has the state GetNextState(state_h, tok) and context_h + that arc's (or escape) weight.  total = LogAdd(s, ns) + context.  The
 *   second_beam largest totals survive.  A sequence receives at most two terms per field and row, and two-term LogAdd is
 *   commutative bit for bit, so the sums do not depend on the visiting order; the ORDER AMONG EQUAL TOTALS, which the reference
 *   leaves open (nth_element over an unordered_map), is: unchanged hypotheses first, in beam order, then extensions,
 *   hypothesis-major and candidate-minor (an extension that IS a live hypothesis counts as that unchanged hypothesis).
 *   End: a hypothesis whose context state is not 0 receives that state's escape weight (the back-off of an unfinished match),
 *   then the order by total, equal totals in beam order.  The Viterbi half and the boundary tags of the reference are not formed.
 * Out per utterance: n_hyp [B] <= nbest; ids [B][nbest][max_tokens] (-1 behind the tokens); n_tokens [B][nbest] = the TRUE
 * length, also above max_tokens (the surplus is not stored); score (total), ctc_score (LogAdd(s, ns)), ctx_score [B][nbest]
 * (-inf / -inf / 0 behind n_hyp).  len[b] == 0 gives n_hyp 0, as CtcSearch returns "" without searching; so does an utterance
 * whose rows leave [0, rows).  An id outside 0 .. V - 1 is CLAMPED into it; a log-probability that is NaN or below -FLT_MAX counts
 * as -FLT_MAX.  workspace: pfhip_op_ctc_prefix_beam_workspace_bytes(rows, B, second_beam, graph) bytes of device memory (the
 * graph, then a (parent, token) trie node per row and beam slot).  hipErrorInvalidValue, before anything is copied or launched,
 * for anything outside the above, a graph of another vocab, a NULL buffer (ids with max_tokens 0 excepted) or a short workspace. */
struct pfhip_ctx_graph;
size_t pfhip_op_ctc_prefix_beam_workspace_bytes(long long rows, int B, int second_beam, const struct pfhip_ctx_graph* graph);
int pfhip_op_ctc_prefix_beam(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                             int B, int V, int blank, int first_beam, int second_beam, const struct pfhip_ctx_graph* graph, int nbest,
                             int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score,
                             float* ctx_score, void* workspace, size_t workspace_bytes, void* stream);
/* The same search with every utterance on its own parameters, in one launch (the second instantiation of the kernel: the
 * arithmetic, the tie rule and the sanitising are those above).  topk_ids / topk_logp [rows][k], row_off and len are DEVICE arrays
 * as above; first_beam, second_beam, nbest and graph_of [B] are HOST arrays, and graphs is a HOST array of n_graphs handles.
 * Utterance b reads the first first_beam[b] columns of its rows (the row stride stays k) and searches with second_beam[b], nbest[b]
 * and graphs[graph_of[b]] (graph_of[b] == -1: no graph); first_beam[b] == 0: no search for b, n_hyp[b] = 0.  With nbest_max the
 * largest nbest[b] among the searching utterances (1 if none): ids [B][nbest_max][max_tokens], n_tokens / score / ctc_score /
 * ctx_score [B][nbest_max]; slots from nbest[b] on hold what slots behind n_hyp hold (-1 / 0 / -inf / -inf / 0).
 * workspace: pfhip_op_ctc_prefix_beam_multi_workspace_bytes(...) bytes of device memory (0 for descriptors the entry refuses): the
 * descriptors, a table of the graphs and their images, which the call copies there on `stream` in one copy, then a trie node per
 * row and slot of the largest second_beam.  hipErrorInvalidValue, before anything is copied or launched, for: a beam outside
 * 0..16, first_beam[b] > k, nbest[b] outside 1..second_beam[b] where first_beam[b] > 0, graph_of[b] outside -1 .. n_graphs - 1, a
 * NULL graph or one built for another vocabulary than V, k outside 1..16, blank outside 0 .. V - 1, a NULL buffer (ids with
 * max_tokens 0 excepted) or a short workspace. */
size_t pfhip_op_ctc_prefix_beam_multi_workspace_bytes(long long rows, int B, int k, const int* first_beam, const int* second_beam,
                                                      const int* nbest, const int* graph_of,
                                                      const struct pfhip_ctx_graph* const* graphs, int n_graphs);
int pfhip_op_ctc_prefix_beam_multi(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off,
                                   const int* len, int B, int V, int blank, const int* first_beam, const int* second_beam,
                                   const int* nbest, const int* graph_of, const struct pfhip_ctx_graph* const* graphs, int n_graphs,
                                   int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score,
                                   float* ctx_score, void* workspace, size_t workspace_bytes, void* stream);
/* Hotword-biased beam search over the candidates of a NON-AUTOREGRESSIVE head (nar_beam.hip): a Paraformer's token rows are
 * independent positions, so the search replaces tokens position by position and never changes the token count.  An EXTENSION: the
 * reference biases a Paraformer only inside its WFST search (BiasLm); this is not that path.
 * Utterance b owns rows [row_off[b], row_off[b] + len[b]) (DEVICE arrays; the ranges must not overlap) of cand_ids / cand_logp
 * [rows][k].  Row t's candidates are its first width[b] columns (tok_c, p_c), descending and distinct as the top-k head leaves them.
 * width, beam, nbest and graph_of [B] are HOST arrays and graphs a HOST array of n_graphs handles, each built for vocab == V
 * (graph_of[b] == -1: no graph).  1 <= width[b] <= k <= 8, 1 <= nbest[b] <= beam[b] <= 16: at most 128 (hypothesis, candidate) pairs.
 *   A hypothesis is (am, ctx, state, node).  Start: one hypothesis, am = 0, ctx = 0, state 0, the root node.
 *   Row t, for every live hypothesis h (beam order) and candidate c < width:  am' = am_h + p_c (one fp32 add, left to right along
 *   the sequence);  (state', w) = GetNextState(state_h, tok_c) of the graph (the arc's weight, else the state's escape weight and
 *   state 0);  ctx' = ctx_h + w;  total' = am' + ctx'.  The `beam` largest totals survive; EQUAL totals order hypothesis-major,
 *   candidate-minor.  Two extensions of a row differ in the parent or in the token, and the parents are distinct sequences of equal
 *   length, so two extensions never name the same sequence: there is NO MERGE STEP, and nothing is summed over alignments.
 *   End: a hypothesis whose state is not 0 receives escape[state] (the back-off of an unfinished match) into ctx, total is formed
 *   again, and the order is by total, equal totals in beam order.
 *   Without a graph w is 0 everywhere: hypothesis 0 is the greedy sequence (column 0 of every row) and its am the fp32
 *   left-to-right sum of cand_logp[.., 0].  Every sum is a single fp32 add in the order written: results are reproducible bit for bit.
 * Out per utterance, with nbest_stride the largest nbest[b]: n_hyp [B] <= nbest[b]; ids [B][nbest_stride][max_tokens] (-1 behind the
 * tokens); n_tokens [B][nbest_stride] = len[b] for a live hypothesis, also above max_tokens (the surplus is not stored); score
 * (total), am_score, ctx_score [B][nbest_stride] (-inf / -inf / 0 behind n_hyp and from nbest[b] on).  len[b] == 0 gives n_hyp 0; so
 * does an utterance whose rows leave [0, rows): its own slots hold that fill (ids -1, n_tokens 0) and nothing else is written.  An id outside 0 .. V - 1 is CLAMPED into it; a
 * log-probability that is NaN or below -FLT_MAX counts as -FLT_MAX; a NaN total ranks as -inf.
 * workspace: pfhip_op_nbest_ctx_beam_workspace_bytes(...) bytes of device memory (0 for descriptors the entry refuses): the
 * descriptors, a table of the graphs and their images, which the call copies there on `stream` in ONE copy, then a (parent, token)
 * trie node per row and slot of the largest beam.  hipErrorInvalidValue, before anything is copied or launched, for anything outside
 * the limits above, graph_of[b] outside -1 .. n_graphs - 1, a NULL graph or one built for another vocabulary than V, a NULL buffer
 * (ids with max_tokens 0 excepted) or a short workspace. */
size_t pfhip_op_nbest_ctx_beam_workspace_bytes(long long rows, int B, int k, const int* width, const int* beam, const int* nbest,
                                               const int* graph_of, const struct pfhip_ctx_graph* const* graphs, int n_graphs);
int pfhip_op_nbest_ctx_beam(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len,
                            int B, int V, const int* width, const int* beam, const int* nbest, const int* graph_of,
                            const struct pfhip_ctx_graph* const* graphs, int n_graphs, int max_tokens, int32_t* n_hyp, int32_t* ids,
                            int32_t* n_tokens, float* score, float* am_score, float* ctx_score, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The token n-gram language model of pfhip.h (pfhip_lm_graph_*) on the device.  lm_step(state, label) is the step pfhip.h states:
 * acc = 0; in state 0: acc += uni_w[label], next = uni_next[label]; elsewhere a binary search over the state's arcs — found: acc +=
 * weight, next = the arc's; not found: acc += backoff_w[state], state = backoff_state[state], again (at most PFHIP_LM_ORDER_MAX
 * trips, then state 0).  Every addition is a single fp32 add in that order; every index is clamped into its array.
 * pfhip_op_lm_score (lm_score.hip) — N-best rescoring and perplexity: sentence b is ids[b][0 .. len[b]) of ids [B][max_len]
 * (DEVICE arrays; len clamped to 0 .. max_len, an id outside 0 .. vocab - 1 CLAMPED into it), walked from the start state, one
 * lane per sentence.  tok_w [B][max_len]: acc of every token (0 behind the sentence); eos_w [B]: acc of </s> behind the last
 * token, 0 where the model has no </s>; total [B]: the fp32 sum of the sentence's tok_w left to right, then + eos_w.  All natural
 * logarithms with the graph's scale and bonus baked in.  workspace: pfhip_op_lm_score_workspace_bytes(lm) bytes of device memory,
 * where the call copies the graph's image on `stream`.  hipErrorInvalidValue, before anything is copied or launched: a NULL graph or
 * buffer (ids / tok_w with max_len 0 excepted), a negative size, B * max_len above 2^31 - 1, a short workspace. */
struct pfhip_lm_graph;
size_t pfhip_op_lm_score_workspace_bytes(const struct pfhip_lm_graph* lm);
int pfhip_op_lm_score(const int32_t* ids, const int* len, int B, int max_len, const struct pfhip_lm_graph* lm, float* tok_w, float* eos_w,
                      float* total, void* workspace, size_t workspace_bytes, void* stream);
/* pfhip_op_nbest_ctx_beam with that model fused in shallowly (its own kernel instantiation; one model serves every utterance of the
 * launch, lm built for vocab == V).  A hypothesis also carries (lm, lm_state): start lm = 0, lm_state = the model's start state.
 * An extension by tok_c: lm' = lm_h + acc(lm_step(lm_state_h, tok_c)), and total' = (am' + ctx') + lm', one more fp32 add.  End:
 * behind the context back-off, where the model has </s>, lm += acc(lm_step(lm_state, vocab)); total is formed again the same way
 * and the order is by total.  lm_score [B][nbest_stride] is the hypothesis's lm (0 behind n_hyp); score includes it, am_score and
 * ctx_score keep their meaning.  Tie rules, sanitising and the node layout are the sibling's.  lm == NULL: the sibling's launch and
 * outputs bit for bit, lm_score 0.  The workspace holds the model's image behind the graphs' (one copy for all of it):
 * pfhip_op_nbest_ctx_beam_lm_workspace_bytes.  Refusals as the sibling's, and a NULL lm_score or a model of another vocabulary. */
size_t pfhip_op_nbest_ctx_beam_lm_workspace_bytes(long long rows, int B, int k, const int* width, const int* beam, const int* nbest,
                                                  const int* graph_of, const struct pfhip_ctx_graph* const* graphs, int n_graphs,
                                                  const struct pfhip_lm_graph* lm);
int pfhip_op_nbest_ctx_beam_lm(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off,
                               const int* len, int B, int V, const int* width, const int* beam, const int* nbest, const int* graph_of,
                               const struct pfhip_ctx_graph* const* graphs, int n_graphs, const struct pfhip_lm_graph* lm,
                               int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* am_score,
                               float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, void* stream);
/* pfhip_op_ctc_prefix_beam_multi with the model fused in shallowly (its own kernel instantiation; one model serves every searching
 * utterance of the launch, lm built for vocab == V).  A hypothesis also carries (lm, lm_state), a function of its PREFIX alone:
 * start lm = 0, lm_state = the model's start state; an unchanged hypothesis keeps both; a new extension h + tok gets lm' = lm_h +
 * acc(lm_step(lm_state_h, tok)); an extension that names a live hypothesis is that hypothesis and keeps that one's (the same
 * values).  total = (LogAdd(s, ns) + ctx) + lm, one more fp32 add.  End: behind the context back-off, where the model has </s>,
 * lm += acc(lm_step(lm_state, vocab)); total again, then the order.  lm_score [B][nbest_max] is the hypothesis's lm (0 behind
 * n_hyp); score includes it, ctc_score and ctx_score keep their meaning.  Everything else is the sibling's.  lm == NULL: the
 * sibling's launch and outputs bit for bit, lm_score 0.  Workspace: pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes (the model's
 * image behind the graphs', one copy for all of it).  Refusals as the sibling's, and a NULL lm_score or a model of another vocabulary. */
size_t pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes(long long rows, int B, int k, const int* first_beam, const int* second_beam,
                                                         const int* nbest, const int* graph_of,
                                                         const struct pfhip_ctx_graph* const* graphs, int n_graphs,
                                                         const struct pfhip_lm_graph* lm);
int pfhip_op_ctc_prefix_beam_multi_lm(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off,
                                      const int* len, int B, int V, int blank, const int* first_beam, const int* second_beam,
                                      const int* nbest, const int* graph_of, const struct pfhip_ctx_graph* const* graphs, int n_graphs,
                                      const struct pfhip_lm_graph* lm, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens,
                                      float* score, float* ctc_score, float* ctx_score, float* lm_score, void* workspace,
                                      size_t workspace_bytes, void* stream);
/* One streaming window (M <= 32 rows): LayerNormalization (g != NULL; width D <= K) -> MatMul/Gemm (+bias, +residual Adds, Relu)
 * (+ the SAN-M FSMN memory of fsmn_v over the M rows, k = 11) in ONE launch — stream_fused.hip. */
int pfhip_op_fused_ln_gemm(const float* X, int ldx, int D, const float* g, const float* b, float eps, const float* W, int ldw,
                           float* C, int ldc, const float* bias, const float* R1, int ldr1, const float* R2, int ldr2,
                           const float* fsmn_v, int ldv, const float* fsmn_w, int M, int N, int K, int relu, void* stream);

/* The same node group with every operand requested in ONE trip to memory and the LayerNormalization applied algebraically
 * (M <= 20 rows, K = 64..2048 in the window shapes): when ln_colsum != NULL, W / bias are the gamma / beta-folded weights
 * (W' = W gamma, b' = b + W beta) and ln_colsum[n] = sum_k W'[n][k]; the LayerNorm is over exactly the K operand columns.
 * Returns hipErrorInvalidValue for shapes the kernel does not take (callers use pfhip_op_fused_ln_gemm there). */
int pfhip_op_fused_gemv_1trip(const float* X, int ldx, const float* W, int ldw, float* C, int ldc, const float* bias,
                              const float* ln_colsum, float eps, const float* R1, int ldr1, const float* fsmn_v, int ldv,
                              const float* fsmn_w, int M, int N, int K, int relu, void* stream);
/* Which kernel instantiation and launch geometry the two entries above take for a shape — the launchers' own choice, reported by the
 * function they call; nothing is launched and no device is needed; the PFHIP_* knobs of this process count.
 * pfhip_op_fused_gemv_1trip_route: out[8] = {ok, LN, FS, CW, CPL, RPL, NF, waves} (has_ln: ln_colsum given, has_fsmn: fsmn_v given;
 * ok = 0: the shape is refused and the rest is 0).  pfhip_op_fused_ln_gemm_route: out[6] = {kernel (1 = vector form, 2 = matrix
 * form), LN, CW, MR, waves, k_blocks}; hipErrorInvalidValue for the M and K that pfhip_op_fused_ln_gemm refuses, and for out == NULL. */
int pfhip_op_fused_gemv_1trip_route(int M, int N, int K, int has_ln, int has_fsmn, int* out);
int pfhip_op_fused_ln_gemm_route(int M, int N, int K, int has_ln, int* out);

/* MatMul-Softmax-MatMul of ONE streaming window: Lq <= 32 queries against Lk <= 32 keys (rows 0.. of the given pointers), H heads of
 * d_k = 128 (the streaming encoder's self-attention over its 20-row window, the decoder's tokens against it:
 * onnxruntime/src/paraformer-online.cpp:426-515).  hipErrorInvalidValue for other shapes (callers use pfhip_op_attention). */
int pfhip_op_window_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                              int H, float scale, void* stream);
/* The same with the head width chosen at run time: 128 or 80 (hipErrorInvalidValue for any other, before anything is launched). */
int pfhip_op_window_attention_hd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                                 int H, float scale, int head_dim, void* stream);
/* B such windows in ONE launch, as a round of streaming connections runs them (grid (H, B)): window b is rows [q_off[b], q_off[b] +
 * q_len[b]) of Q / O against rows [kv_off[b], kv_off[b] + kv_len[b]) of K / V (DEVICE arrays; every length <= 32, max_q_len /
 * max_kv_len their host-side maxima); a window with q_len[b] <= 0 or kv_len[b] <= 0 writes nothing.  fsmn_w != NULL (self-attention:
 * q segments == kv segments): the launch also writes the SAN-M memory block of V (pfhip_op_fsmn without a residual, bit for bit) into
 * mem.  Only columns [0, H * head_dim) of a row are read or written.  hipErrorInvalidValue, before anything is launched, for
 * max_q_len or max_kv_len outside 1..32, a head width other than 80 or 128, B < 1, H < 1, a NULL buffer, fsmn_w without mem, a row
 * stride (ldmem with fsmn_w) below H * head_dim or not a multiple of 4. */
int pfhip_op_window_attention_segments(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                                       const int* q_off, const int* q_len, const int* kv_off, const int* kv_len, int B, int H, int max_q_len,
                                       int max_kv_len, float scale, const float* fsmn_w, float* mem, int ldmem, int head_dim, void* stream);

/* The window's MatMul-Softmax-MatMul AND the MatMul/Gemm that projects its context (W [N, 512]; +bias, +residual Add, + the SAN-M
 * FSMN memory of fsmn_v over the Lq rows) in ONE launch: H = 4 heads of 128, Lq <= 20, Lk <= 32.  hipErrorInvalidValue otherwise. */
int pfhip_op_fused_att_out(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int Lq, int Lk, int H, float scale,
                           const float* W, int ldw, float* C, int ldc, const float* bias, const float* R1, int ldr1, const float* fsmn_v,
                           int ldfv, const float* fsmn_w, int N, void* stream);

/* Resampling ahead of the front end (Audio::WavResample, onnxruntime/src/audio.cpp:259-284; plan of resample.cpp:104-153).
 * Host only: the polyphase plan of a rate pair.  *n_phases = Q output samples per unit, *in_unit = P input samples per unit,
 * *taps = K, the longest weight row.  With first_index [Q], ntaps [Q] or weights [Q * K] (row ph zero-padded past ntaps[ph])
 * non-NULL and cap_floats >= Q * K they are filled.  Output sample s reads inputs first_index[s % Q] + (s / Q) * P + j. */
int pfhip_op_resample_table(int fs_in, int fs_out, int32_t* first_index, int32_t* ntaps, float* weights, size_t cap_floats,
                            int* n_phases, int* taps, int* in_unit);
/* The kernel on a packed batch (resample.hip): utterance b reads n_in[b] samples at d_in + in_off[b] and writes
 * pfhip_resample_len(fs_in, fs_out, n_in[b]) samples at d_out + out_off[b].  in_off / n_in / out_off are HOST arrays.
 * fs_in == fs_out is a device copy.  Unsupported pairs return hipErrorInvalidValue. */
int pfhip_op_resample(const float* d_in, const int64_t* in_off, const int* n_in, int batch, int fs_in, int fs_out, float* d_out,
                      const int64_t* out_off, void* stream);

/* ---- The scan, cache and row kernels, one entry each, for operator tests (no model path calls these entries).
 * Where a kernel reads per-connection device descriptors (csrc/kernels.h StreamSeg / VadSeg), the entry takes plain HOST arrays of
 * B entries plus a base pointer and a stride (in floats) for the per-connection state, builds the descriptors, uploads them with a
 * synchronous copy and returns after the stream has drained.  Every entry returns hipErrorInvalidValue, before anything is
 * launched, for what its kernel assumes: channel counts and row strides that are not multiples of 4, a NULL buffer. */
/* CifSearch (onnxruntime/src/paraformer-online.cpp:270-345) for B connections: connection b integrates its carry, rows
 * [row_off[b], row_off[b] + n[b]) of enc / alphas (alphas outside [pre[b], suf[b]) count as 0) and, with is_last[b], the tail slot.
 * Its fires land in emb[b * emb_rows ..] (D floats a row; fires past emb_rows are counted, not stored), their count in n_fire[b];
 * its carry (hidden [D], then the integrate scalar) lives at carry + b * carry_stride and is replaced.  D <= 1024. */
int pfhip_op_cif_stream(const float* enc, int lde, const float* alphas, const int* row_off, const int* n, const int* is_last,
                        const int* pre, const int* suf, float* carry, long long carry_stride, int B, int D, float threshold,
                        float tail, float* emb, int emb_rows, int* n_fire, void* stream);
/* The same scan by the sibling instantiation that also records where each token fired: fire_step[b * emb_rows + j] = the step of
 * the scan in which stored token j of connection b fired (0 = the carry slot, 1..n[b] = window rows 0..n[b]-1, n[b] + 1 = the tail
 * slot).  Slots past the stored fires are not written.  emb, n_fire and the carry are pfhip_op_cif_stream's bit for bit.  Refuses
 * what pfhip_op_cif_stream refuses, and a NULL fire_step. */
int pfhip_op_cif_stream_fires(const float* enc, int lde, const float* alphas, const int* row_off, const int* n, const int* is_last,
                              const int* pre, const int* suf, float* carry, long long carry_stride, int B, int D, float threshold,
                              float tail, float* emb, int emb_rows, int* n_fire, int* fire_step, void* stream);
/* The streaming decoder's FSMN with its 10-frame cache (paraformer-online.cpp:374, 500): connection b's tokens are rows
 * [tok_off[b], tok_off[b] + n_tok[b]) of t2 / res / out (row stride C; out may alias res), its caches [layers][10][C] live at
 * dcache + b * dcache_stride; out = res + t2 + conv over [cache; t2], and the layer's cache becomes the last 10 rows of [cache; t2]
 * (untouched where n_tok[b] == 0). */
int pfhip_op_fsmn_cached(const float* t2, const float* w, const float* res, float* out, const int* tok_off, const int* n_tok, float* dcache,
                         long long dcache_stride, int B, int layer, int C, void* stream);
/* The FSMN-VAD memory block, left order 20 (fsmn-vad.cpp:129-134): connection b's rows are [row_off[b], row_off[b] + T[b]) of p / out,
 * its caches [layers][19][C] at cache_in / cache_out + b * cache_stride; out = p + causal conv over [cache_in; p], cache_out = the
 * last 19 rows of [cache_in; p] — not written where final[b] != 0.  cache_out must not be cache_in. */
int pfhip_op_fsmn_causal20(const float* p, int ldp, const float* w, const int* row_off, const int* T, const int* final,
                           const float* cache_in, float* cache_out, long long cache_stride, int B, int layer, float* out, int ldo, int C,
                           void* stream);
/* Softmax over columns [0, N) of every row; y [M][N] packed, col0 (may be NULL) [M] = y[:, 0]. */
int pfhip_op_softmax_rows(const float* x, int ldx, int M, int N, float* y, float* col0, void* stream);
/* Frame energies of the end-point detector's decibel track (E2EVadModel::ComputeDecibel, e2e-vad.h:437-452): B utterances packed in
 * pcm; DEVICE arrays sample_off [B] (int64, in samples), frame_off [B + 1] (prefix sums of nframes) and nframes [B] with
 * nframes[b] = n_b < flen ? 0 : 1 + (n_b - flen) / fshift.  e[frame_off[b] + f] = sum_{i < flen} x[f * fshift + i]^2, one fp32
 * accumulator, i ascending, each product rounded to fp32 first: bit for bit the host loop.  s16: x = (float)s / 32768 (exact); an
 * utterance may start at an odd sample.  hipErrorInvalidValue when 63 * fshift + flen samples exceed 64 KB of LDS. */
int pfhip_op_frame_energy(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                          int flen, int fshift, float* e, void* stream);
int pfhip_op_frame_energy_s16(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                              int total_frames, int flen, int fshift, float* e, void* stream);
/* The predictor's Conv1d k = 3 operand: col[row] = [h[row - 1] | h[row] | h[row + 1]], zeros where row_pos[row] -/+ 1 leaves
 * [0, row_len[row]) (device arrays: the local index and the utterance length of every packed row). */
int pfhip_op_im2col3(const float* h, int ldh, float* col, int ldc, const int* row_pos, const int* row_len, int M, int D, void* stream);
/* alphas[row] = relu(sigmoid(o[row] . w + b[0]) * smooth - noise): CifPredictorV2's head; alpha2 the timestamp head's (b by value). */
int pfhip_op_alpha(const float* o, int ldo, const float* w, const float* b, float smooth, float noise, float* alphas, int M, int D,
                   void* stream);
int pfhip_op_alpha2(const float* y, int ldy, const float* w, float b, float smooth, float noise, float* a2, int rows, int D, void* stream);
/* Timestamp head, per utterance b (frames [off[b], off[b] + len[b]); device arrays; len[b] <= max_len): us_alphas = a2 rescaled to
 * sum to token_num[b], us_peaks = cif_wo_hidden(us_alphas, threshold). */
int pfhip_op_us_cif(const float* a2, const int* off, const int* len, const int* token_num, int B, int max_len, float threshold,
                    float* us_alphas, float* us_peaks, void* stream);
/* The timestamp head's bidirectional LSTM recurrence (hidden 512) over B <= 32 packed utterances (frames [off[b], off[b] + len[b]);
 * DEVICE arrays; len[b] <= Lmax): gx [rows, 4096] = input projections + biases (forward i,f,g,o | backward i,f,g,o), whh
 * [2][2048][512] with |w| < 32, y [rows, 1024] = forward h | backward h; only rows inside an utterance are written.  stepwise == 0:
 * the persistent kernel; stepwise != 0: one launch per step (bit-identical).  hx = pfhip_op_blstm_scratch_floats() floats that the
 * caller zeroed once; after the stream has drained, word pfhip_op_blstm_flag_word() of hx is the persistent kernel's error word
 * (0 = served; 1 = its h exchange timed out; 2 = the blocks of a direction were not on one XCD; y is then not valid) and the
 * words flag + 2, flag + 3 hold the XCC id + 1 of the forward and the backward direction.  cst = 2 * 32 * 512 floats of cell
 * state (stepwise only; may be NULL otherwise).  B = 0 or Lmax = 0 writes nothing.  hipErrorInvalidValue, before anything is
 * launched, for B > 32, B < 0, Lmax < 0 or a NULL buffer. */
int pfhip_op_blstm_scratch_floats(void);
int pfhip_op_blstm_flag_word(void);
int pfhip_op_blstm(const float* gx, const float* whh, float* y, const int* off, const int* len, int B, int Lmax, int stepwise, float* hx,
                   float* cst, void* stream);
/* One LSTM step of the hotword embedder on pre-activations G [H][4 D] (gates i, f, g, o): c, h [H][D] updated in place; rows with
 * lens[j] - 1 == t also copy h into sel[j]. */
int pfhip_op_lstm_cell(const float* G, float* c, float* h, const int32_t* lens, int t, float* sel, int H, int D, void* stream);

/* ---- The kernels that start every request, one entry each, for operator tests (no model path calls these entries).  Index arrays
 * named HOST are plain host arrays: the entry checks them, uploads them (or the descriptors built from them) with a synchronous copy
 * and returns after the stream has drained.  Every entry returns hipErrorInvalidValue before anything is launched for a NULL buffer
 * and for what its kernel assumes. */
/* The fused fbank kernel (csrc/fbank.hip; 16 kHz, 25-ms frames at a 10-ms shift, 80 mel bins, the tables of the model / VAD / stream
 * loaders) on B >= 1 utterances packed in pcm (pcm_samples samples on the DEVICE; f32 in [-1, 1) or 16-bit PCM standing for
 * s / 32768.f, the two bit for bit equal).  HOST arrays: sample_off [B] (in samples; odd offsets allowed for s16), frame_off [B + 1]
 * (prefix sums of nframes, frame_off[B] == total_frames), nframes [B].  Exactly one of two outputs:
 *   fb_out: raw log-mel frames [total_frames][80] (B == 1 by launch_fbank_frames, otherwise by launch_fbank_frames_batch);
 *   feats (feats_rows rows of 560) with row_off [B] (HOST), cmvn_mean / cmvn_istd [560] (device): LFR (m = 7, n = 6) and
 *   (x + mean) * istd fused, utterance b's ceil(nframes[b] / 6) rows at row row_off[b].
 * Refused: B < 1, frame_off that is not the prefix sum of nframes or does not end at total_frames, a frame outside pcm, a row outside
 * feats, both outputs or neither. */
int pfhip_op_fbank(const float* pcm, long long pcm_samples, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                   int total_frames, float* fb_out, float* feats, long long feats_rows, const int* row_off, const float* cmvn_mean,
                   const float* cmvn_istd, void* stream);
int pfhip_op_fbank_s16(const int16_t* pcm, long long pcm_samples, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                       int total_frames, float* fb_out, float* feats, long long feats_rows, const int* row_off, const float* cmvn_mean,
                       const float* cmvn_istd, void* stream);
/* LfrCmvn (fsmn-vad.cpp:198-238 == paraformer.cpp:421-461) for any (m, n, n_mels): fb [F][n_mels] -> out [ceil(F / n)][ldo], row i =
 * frames [i n - (m - 1) / 2, + m) with the first / last frame replicated, (x + mean) * istd, columns m * n_mels .. ldo zeroed. */
int pfhip_op_lfr_cmvn(const float* fb, int F, int m, int n, int n_mels, const float* mean, const float* istd, float* out, int ldo,
                      void* stream);
/* The same for B files whose frames lie in fb (fb_frames frames): file b is frames [frame_off[b], + nframes[b]) (HOST arrays), padded
 * at its own edges, its rows at row row_off[b] of out (out_rows rows).  A file without frames writes nothing. */
int pfhip_op_lfr_cmvn_packed(const float* fb, long long fb_frames, const int* frame_off, const int* nframes, const int* row_off, int B,
                             int m, int n, int n_mels, const float* mean, const float* istd, float* out, int ldo, long long out_rows,
                             void* stream);
/* OnlineLfrCmvn (fsmn-vad-online.cpp:90-133) for n_ops connections (HOST arrays): operation k reads Tin[k] frames from frame fb_off[k]
 * of fb (the splice cache first) and writes n_out[k] rows from row row_off[k]: row i = frames [i n, i n + m), the tail replicated
 * with the last frame, no left padding.  An operation with rows needs Tin >= 1. */
int pfhip_op_lfr_cmvn_online_batch(const float* fb, long long fb_frames, const int* fb_off, const int* Tin, const int* n_out,
                                   const int* row_off, int n_ops, int m, int n, int n_mels, const float* mean, const float* istd,
                                   float* out, int ldo, long long out_rows, void* stream);
/* The streaming front end's OnlineLfrCmvn + x * scale + GetPosEmb (paraformer-online.cpp:196-268, 549-555; m = 7, n = 6, 80 bins) for
 * n_ops connections (HOST arrays): row i of operation k = frames [6 i, 6 i + 7) of its T[k] frames at fb_off[k], the tail replicated,
 * out row row_off[k] + i columns [0, 560) = ((x + mean) * istd) * scale + PE(pos0[k] + i + 1); inv_ts [280].  Columns 560 .. ldo are
 * not written. */
int pfhip_op_stream_lfr_batch(const float* fb, long long fb_frames, const int* fb_off, const int* T, const int* n_rows, const int* pos0,
                              const int* row_off, int n_ops, const float* mean, const float* istd, float scale, const float* inv_ts,
                              float* out, int ldo, long long out_rows, void* stream);
/* n_ops row copies in one launch (HOST arrays): operation k writes nrows[k] rows of ldd[k] floats at dst + dst_off[k]: columns
 * [0, ncols[k]) from src + src_off[k] with row stride lds[k] (0: its row 0 repeated), or zeros where src_off[k] < 0; columns
 * ncols[k] .. ldd[k] zeroed.  dst_floats / src_floats: the floats behind dst / src, which every operation must stay inside. */
int pfhip_op_rows_copy_batch(float* dst, long long dst_floats, const long long* dst_off, const float* src, long long src_floats,
                             const long long* src_off, const int* ldd, const int* lds, const int* nrows, const int* ncols, int n_ops,
                             void* stream);
/* x0[row][0 .. D) = feats[row] * scale + PE(row_pos[row] + 1) (sin in columns < D / 2, cos above; inv_ts [D / 2]); columns D .. ldx
 * zeroed.  D even. */
int pfhip_op_embed(const float* feats, int D, float* x0, int ldx, const int* row_pos, int M, const float* inv_ts, float scale, void* stream);
/* out[row][0 .. D) = table[id] * scale + PE(pos + 1), id = ids[row] CLAMPED to [0, vocab - 1], pos = pos_of_row ? pos_of_row[row] : row;
 * columns D .. Dout zeroed, columns Dout .. ldo not written.  D even. */
int pfhip_op_embed_gather(const int32_t* ids, const float* table, int vocab, int D, int Dout, float* out, int ldo, int N,
                          const float* inv_ts, float scale, const int* pos_of_row, void* stream);
/* out[row] = the first maximum over columns [0, ncls) of logits[row] (std::max_element with operator<: a NaN never replaces the
 * running maximum, a NaN in column 0 is never replaced). */
int pfhip_op_argmax_first(const float* logits, int ldl, int N, int ncls, int32_t* out, void* stream);
/* Row gathers; D % 4 == 0 (rows move as float4s).  compact: emb[r] = stage[tok_row_src[r]]; gather_rows: out[r] = table[ids[r]];
 * svs_prompt_rows: rows row_off[b] .. + 3 of feats (row stride ld) = rows prompt[4 b .. 4 b + 3] of E, for every b with len[b] >= 4
 * (an utterance with fewer rows is left untouched).  Index arrays on the device; the indices themselves are the caller's to keep
 * inside the tables. */
int pfhip_op_compact(const float* stage, float* emb, const int* tok_row_src, int ML, int D, void* stream);
int pfhip_op_gather_rows(const int32_t* ids, const float* table, int D, float* out, int R, void* stream);
int pfhip_op_svs_prompt_rows(const float* E, int D, const int* prompt, const int* row_off, const int* len, int B, float* feats, int ld,
                             void* stream);
/* best[r] = logp[r][ids[r]]; lse[r] = log sum_c exp(logits[r][c]), c < V (a row of -inf gives -inf). */
int pfhip_op_gather_best(const float* logp, int ld, const int32_t* ids, int M, float* best, void* stream);
int pfhip_op_row_lse(const float* logits, int ld, int M, int V, float* lse, void* stream);

/* ---- The kernels of the DNSMOS speech-quality networks (utils/dnsmos_local.py with utils/DNSMOS/sig_bak_ovr.onnx and model_v8.onnx;
 * csrc/conv3x3.hip, csrc/dnsmos.hip), one entry each.  Arrays named HOST are plain host arrays; the entries that take one, and the
 * convolution for Cin >= 32, upload what they build with a synchronous copy and return after the stream has drained.  Every entry
 * returns hipErrorInvalidValue, before anything is launched, for a NULL buffer and for what its kernel does not take. */
/* A Conv (kernel 3x3, pads 1, strides 1, with bias) + Relu, and with pool != 0 the MaxPool (kernel 2x2, strides 2, VALID: an odd last
 * row or column is dropped) behind it — the graphs' nodes conv2d* / Relu* / *pooling* / MaxPool_*_conv —, on NHWC activations, which
 * makes the graphs' Transposes around them empty: x [N][H][W][Cin] -> y [N][H][W][Cout], pooled [N][H / 2][W / 2][Cout]; w is the
 * file's own [Cout][Cin][3][3], bias [Cout].  Cin == 1 (any Cout): nine fp32 FMAs per value, ky, kx ascending.  Cin 32 or a multiple of 64
 * with Cout 32 or 64: an implicit GEMM on the fp16 matrix cores, two planes per operand and three products, fp32 accumulation — as
 * close to fp64 as an fp32 chain; the weights must be finite and |x| < 65504; N <= 65535. */
int pfhip_op_conv3x3_relu(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int pool,
                          void* stream);
/* The primary net from `input_1` to `mos_estimator_logpow/truediv:0` (Slice x 2, Reshape x 2, Concat, the two 1x1 Convs stft-real /
 * stft-imag, Square, Square_1, Add, Sqrt, Pow, Max, Log, Div): window i = the 160 (n_frames + 1) samples at pcm + win_off[i] (HOST;
 * pcm_samples samples on the device, f32 in [-1, 1] or 16-bit PCM standing for s / 32768.f, the two bit for bit equal), frame f its
 * samples [160 f, 160 f + 320); stft_real / stft_imag the file's kernels [161][320] (device); floor_v, power, denom the initialisers
 * Maximum/x, pow/y and truediv/y (1e-12, 2, 2.3025851; a power other than 2 is refused).  out [n_win][n_frames][161] =
 * log(max(floor_v, sqrt(re^2 + im^2)^2)) / denom; fp32, four accumulators over k mod 4.  n_win <= 65535. */
int pfhip_op_dnsmos_logpow(const float* pcm, long long pcm_samples, const int64_t* win_off, int n_win, int n_frames, const float* stft_real,
                           const float* stft_imag, float floor_v, float power, float denom, float* out, void* stream);
int pfhip_op_dnsmos_logpow_s16(const int16_t* pcm, long long pcm_samples, const int64_t* win_off, int n_win, int n_frames,
                               const float* stft_real, const float* stft_imag, float floor_v, float power, float denom, float* out,
                               void* stream);
/* ComputeScore.audio_melspec (utils/dnsmos_local.py:29-33), the input of model_v8.onnx: out [n_win][900][120] = (power_to_db(
 * melspectrogram(y = the first 144000 samples of window i, sr 16000, n_fft 321, hop 160, 120 mels), ref = max) + 40) / 40,
 * transposed.  The library's defaults behind that line (periodic Hann window, centred frames padded with zeros, Slaney mel scale and
 * normalisation over 0 .. 8000 Hz, amin 1e-10, top_db 80) are recalled from librosa 0.10.0, not read from a file. */
int pfhip_op_dnsmos_melspec(const float* pcm, long long pcm_samples, const int64_t* win_off, int n_win, float* out, void* stream);
int pfhip_op_dnsmos_melspec_s16(const int16_t* pcm, long long pcm_samples, const int64_t* win_off, int n_win, float* out, void* stream);
/* ReduceMax over axes 1, 2 (global_max_pooling2d) and the three MatMul + Add (+ Relu after the first two) behind it: x [N][HW][C]
 * (NHWC with H and W merged), w_i [in][out] as the graph's MatMul holds them, out [N][D3].  One workgroup per window, fp32, k
 * ascending.  C, D1, D2, D3 in 1 .. 256. */
int pfhip_op_globalmax_mlp(const float* x, int N, int HW, int C, const float* w1, const float* b1, int D1, const float* w2, const float* b2,
                           int D2, const float* w3, const float* b3, int D3, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
