// Internal launcher declarations for the gfx950 kernels behind include/pfhip.h.
// All pointers are device pointers unless a name says host.  All launches are asynchronous on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfhip {

constexpr int kTileM = 128;      // GEMM block tile rows   (activation buffers are allocated in multiples)
constexpr int kTileN = 128;      // GEMM block tile cols   (weights are repacked/padded to multiples)
constexpr int kTileK = 32;       // GEMM k-step            (K is padded to multiples)
constexpr int kHeadDim = 128;    // the attention kernels' default head width (Paraformer-large); see head_dim_supported
constexpr int kHeadDimSmall = 80; // the small Paraformer: d_model 320 / 4 heads
inline bool head_dim_supported(int hd) { return hd == kHeadDim || hd == kHeadDimSmall; }      // what a Paraformer may be built with
constexpr int kMelW = 32;        // max taps per mel triangle (80 bins @ 512-pt FFT need <= 19)

// ---- front end (SURVEY §8a rows a2,a3) -------------------------------------------------------
struct FbankTables {
  const float* window;     // [400] hamming, feature-window.cc:33-42
  const double* tw512;     // [256][2] cos/-sin of 2*pi*k/512
  const int* mel_off;      // [n_mels]
  const int* mel_size;     // [n_mels]
  const float* mel_w;      // [n_mels][kMelW]
  const float* cmvn_mean;  // [lfr_m*n_mels]
  const float* cmvn_istd;  // [lfr_m*n_mels]
};
// pcm: utterances back to back; sample_off[b] (int64), frame_off[b] prefix of fbank frame counts
// (B+1 entries), nframes[b], row_off[b] (first LFR row of utterance b in feats).
void launch_fbank_lfr_cmvn(const float* pcm, const int64_t* sample_off, const int* frame_off,
                           const int* nframes, const int* row_off, int B, int total_frames,
                           FbankTables tb, float* feats, hipStream_t s);
// The same three launchers (this one and the two below) from 16-bit PCM: the sample s stands for s / 32768.f, which the float form
// multiplies by 32768 again (paraformer.cpp:312-314), so the kernel loads (float)s and every result is bit for bit that of the float
// form fed s / 32768.f.  sample_off counts samples: an utterance may start at an odd one (2-byte alignment is all that is assumed;
// the compiled kernel may fetch two neighbouring samples with one unaligned 4-byte load, which gfx950 global loads allow).
void launch_fbank_lfr_cmvn(const int16_t* pcm, const int64_t* sample_off, const int* frame_off,
                           const int* nframes, const int* row_off, int B, int total_frames,
                           FbankTables tb, float* feats, hipStream_t s);

// Streaming form (ParaformerOnline::FbankKaldi, paraformer-online.cpp:119-145): one utterance, raw
// log-mel frames [total_frames, 80] out, no LFR/CMVN.  sample_off/frame_off/nframes: 1/2/1 entries.
void launch_fbank_frames(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes,
                         int total_frames, FbankTables tb, float* fb_out, hipStream_t s);
void launch_fbank_frames(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes,
                         int total_frames, FbankTables tb, float* fb_out, hipStream_t s);
// the same for B utterances back to back in `pcm` (frame_off has B + 1 entries); frames land back to back in fb_out
void launch_fbank_frames_batch(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                               int total_frames, FbankTables tb, float* fb_out, hipStream_t s);
// the s16 form serves the packed offline VAD pass (pfhip_vad_forward_sil_batch_s16, vad.cpp), whose staging buffer holds the files'
// shorts as they arrived; both streaming families convert to f32 while the host copies the samples into their staging buffers
void launch_fbank_frames_batch(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B,
                               int total_frames, FbankTables tb, float* fb_out, hipStream_t s);

// x0[row][0..D) = feats*scale + PE(row_pos[row]+1); columns D..ldx are zeroed.
void launch_embed(const float* feats, int D, float* x0, int ldx, const int* row_pos, int M,
                  const float* inv_timescale, float scale, hipStream_t s);

// ---- the fp16 two-plane domain guard ---------------------------------------------------------------------------------------
// The default large-GEMM / attention forms stage their operands as two fp16 planes (gemm_x3.hip header): |a| >= 65504 overflows,
// rows whose magnitude is far below 1 lose relative precision (absolute error 2^-25 per element).  A forward runs with a
// per-thread launch context: `range_flag` (device word) is raised (bit 1) by the LayerNorm-folding kernels when a row's CENTRED
// standard deviation leaves [2^-8, 2^11] (1 / rstd, what the window below is applied to — not the rms: the offset is judged apart)
// or when its offset |mean| / std exceeds kLnOffsetMax; by the LayerNorm kernel and by the head when a row is not finite (bit 0:
// the check sits on the residual stream because ReLU swallows NaN).  Inside both limits |x| <= |mean| + sqrt(512) std <=
// (4 + 22.7) * 2048 < 65504: no element of such a row of <= 512 values overflows a plane.  `exact` routes every split-operand
// launch of the calling thread to the bf16 three-plane kernels (gemm_x6.hip / attention_x6.hip: fp32's exponent range, exact
// split), keeps the encoder off the plane images and — the fold cancels in fp32 accumulation as well — the forward off the
// LayerNorm fold (launch_layernorm + GEMM).  The reference computes in plain fp32 (onnxruntime/src/paraformer.cpp:496-541).
struct LaunchCtx {
  bool exact = false;
  int* range_flag = nullptr;
};
LaunchCtx& launch_ctx();                      // thread-local (gemm.hip)
constexpr float kLnRstdMin = 1.0f / 2048.0f, kLnRstdMax = 256.0f;
// The fold rstd * (x W'^T - mean * colsum) subtracts two terms of size |mean| to leave one of size std: it loses |mean| / std of
// the accumulation's precision on rows the window above cannot see.  Measured against fp64 (DESIGN.md section 2, table "stated
// domain of the fold"; tests/test_gpu_ln_fold.py::test_fold_stated_domain): at |mean| / std = 4 every form is within the GEMM bound
// 3e-5 (1.0e-5 .. 1.4e-5), at 16 none is (3.9e-5 .. 5.3e-5, more than 4 x the unfolded fp32 path).  4 is the largest offset of
// that sweep at which all forms hold, so it is the limit.
constexpr float kLnOffsetMax = 4.0f;
// whether a row with these merged statistics is outside the domain of the fold (NaN / Inf statistics are)
__host__ __device__ inline bool ln_row_out_of_domain(float mean, float rstd) {
  const float off = mean * rstd;
  return !(rstd > kLnRstdMin && rstd < kLnRstdMax) || !(off * off <= kLnOffsetMax * kLnOffsetMax);
}

// ---- dense ops --------------------------------------------------------------------------------
// Operands of C[M,N] = act(LNfold?(A[M,K]) W[N,K]^T + bias[N]) (+R1[M,N]) (+R2[M,N]); an absent field is nullptr / 0 / false / 1.
// A rows must be allocated up to a multiple of 128, K % 32 == 0, W readable for ceil(N/128)*128 rows.  C may alias R1 or R2
// (in-place residual update).
struct GemmOp {
  const float* A = nullptr; int lda = 0;
  const float* W = nullptr; int ldw = 0;
  float* C = nullptr; int ldc = 0;
  int M = 0, N = 0, K = 0;
  const float* bias = nullptr;
  const float* R1 = nullptr; int ldr1 = 0;
  const float* R2 = nullptr; int ldr2 = 0;
  bool relu = false;
  // power of two with max|W| * w_scale < 65504, used by the fp16 two-plane kernels (gemm_x3.hip) to stage W * w_scale
  // (best_w_scale below; 1 is always valid for |W| < 65504 and costs precision only for weights of very small magnitude)
  float w_scale = 1.0f;
  // The two below are served by the split-operand kernels only (gemm_x6.hip / gemm_x3.hip: GemmKernel::SplitBySize or a forced one);
  // launch_gemm aborts when they reach another kernel.
  // ln_stats (with ln_tiles, ln_colsum): LayerNorm folded in — A is the raw residual stream x, W must be W * gamma, bias must be
  // bias + W beta and ln_colsum[n] = sum_k W[n][k] gamma[k]; the epilogue forms rstd_i * (x W'^T - mean_i * colsum) + bias with the
  // statistics merged from the ln_tiles pairs per row the producer left (eps 1e-12).
  const float* ln_stats = nullptr; int ln_tiles = 0; const float* ln_colsum = nullptr;
  // stats_out (N == tiles_n * 128 exactly): the epilogue also leaves per-row LayerNorm statistics of its 128-column tile at
  // stats_out[row][tile column][2] = (mean of the tile's columns, sum of squared deviations from it).
  float* stats_out = nullptr;
};
// Which kernel launch_gemm takes.  BySize: the measured rules of gemm.hip (fp32 MFMA 32x32x2 kernels below 48 tiles of 128 x 128,
// the split-operand kernels from there).  The next nine force one kernel (dev / tests): the 128 x 128 tiled, the weight-streaming
// and the 64 x 128 tiled fp32-MFMA kernels; the bf16 three-plane / six-product kernels (gemm_x6.hip) and the fp16 two-plane /
// three-product kernels (gemm_x3.hip) on their 256 / 128 / 64 x 128 tiles.  SplitBySize — the product path of the LayerNorm fold
// and of the row statistics: always the split-operand kernels, form by context and tile by the rules of BySize.
enum class GemmKernel { BySize, Tiled128, Streaming, Tiled64, Bf16_256, Bf16_128, Bf16_64, F16_256, F16_128, F16_64, SplitBySize };
enum class SplitTile { Rows256, Rows128, Rows64 };      // tile height of the split-operand kernels (128 columns)
enum class SplitForm { ByContext, F16x3, Bf16x6 };      // ByContext: fp16 x3 unless PFHIP_GEMM_X3=0 or the launch context is exact
// guard == false (the product path): C/R1/R2 are allocated for ceil(M/128)*128 rows and ceil(N/128)*128 columns and bias is
// readable to the padded N, so the epilogue has no bounds branches (pad outputs are junk nobody reads).  guard == true
// bounds-checks every element (the streaming and the split-operand kernels always do).
void launch_gemm(const GemmOp& op, GemmKernel kernel, bool guard, hipStream_t s);
float best_w_scale(float max_abs);
// fp32-grade GEMM on the BF16 matrix cores (three-way bf16 split of both operands, six MFMAs per block): gemm_x6.hip.
// gw: column-group width of the tile order.  With ln_stats the 256-row tile becomes the 128-row one.
void launch_gemm_f32_bf16x6(const GemmOp& op, SplitTile tile, int gw, hipStream_t s);
// the same tilings with TWO fp16 planes and THREE products per block (gemm_x3.hip); op.w_scale: the power-of-two weight scale
void launch_gemm_f32_f16x3(const GemmOp& op, SplitTile tile, int gw, hipStream_t s);
// ---- pre-split operands (gemm_p3.hip): the three-product fp16 scheme with the split taken out of the K-loop -------------------
// Plane image of X[rows, K]: two arrays (hi, lo) of plane_image_bytes(rows, K) bytes each, laid out [K / 16][rows padded to 128][16]
// fp16 with the 16-byte halves of a row swapped where row bit 3 is set.  launch_split_planes writes the images of an fp32 matrix
// (times `scale`); launch_gemm_p3 multiplies A images by W images (N % 128 == 0, K % 16 == 0; W pre-multiplied by w_scale) and
// writes fp32 C (bias, LayerNorm-fold finish, residual R1, ReLU, row statistics) and / or the plane images of C (rows_p rows).
size_t plane_image_bytes(int rows, int K);
void launch_split_planes(const float* X, int ld, int rows_valid, int rows, int K, float scale, void* hi, void* lo, hipStream_t s);
struct PlaneGemmOp {
  const void* Ah = nullptr; const void* Al = nullptr; int rows_a = 0;      // A images, rows per K-step
  const void* Wh = nullptr; const void* Wl = nullptr; int rows_w = 0;      // W images
  float w_scale = 1.0f;
  float* C = nullptr; int ldc = 0;
  void* Ph = nullptr; void* Pl = nullptr; int rows_p = 0;                  // images of C
  // row_planes_from = c > 0 (the encoder's QKV projection, C given): columns < c leave as fp32 rows of C, columns >= c as ROW-MAJOR
  // fp16 planes Ph / Pl [M][rows_p] (rows_p = elements per plane row; column n at element n - c) — the K | V operand of
  // attention_p3.hip.  c % 128 == 0; 128- and 64-row tiles only.
  int row_planes_from = 0;
  int M = 0, N = 0, K = 0;
  const float* bias = nullptr;
  const float* R1 = nullptr; int ldr1 = 0;
  bool relu = false;
  const float* ln_stats = nullptr; int ln_tiles = 0; const float* ln_colsum = nullptr;      // as GemmOp's
  float* stats_out = nullptr;
};
// The column-group width of the tile order is 4; PFHIP_P3_GW overrides it on the 128-column kernels only (not on the 256 x 256 tile).
void launch_gemm_p3(const PlaneGemmOp& op, hipStream_t s,
                    int tile_rows = 0,       // 0: 64-row tiles when 128-row tiles would fill less than a round; 64 / 128 / 256 force one
                    int tile_cols = 0);      // 256: the 256 x 256 tile, for the forms gemm_p3_wide_serves() names (tile_rows 0)
// whether the 256 x 256 tile has this form (LayerNorm fold, fp32 C or plane images of C but not both, no residual, no statistics out,
// N % 256 == 0), and how many launches of this process it has served (tests, probes)
bool gemm_p3_wide_serves(bool c, bool planes, bool r1, bool ln, bool stats_out, int row_planes_from, int N, int K);
long gemm_p3_wide_launches();
// Row-major planes of an fp32 matrix (tests, tools): hi / lo [rows][ldp] fp16, cols % 8 == 0.
void launch_split_rows(const float* X, int ld, int rows, int cols, void* hi, void* lo, int ldp, hipStream_t s);
// gemm_x6_ln_ok(M): whether launch_gemm (BySize) would put the N = 512 launches of M rows on the split-operand kernels (both sides
// of a statistics hand-off must).
bool gemm_x6_ln_ok(int M);
bool gemm_f16_planes_form();      // the large GEMMs are on the fp16 two-plane form (not PFHIP_GEMM_X3=0 / PFHIP_GEMM_X6=0)

// y[row][0..D) = LN(x[row][0..D)) * g + b; columns D..Dout zeroed.  D % 4 == 0, Dout <= 2048.
void launch_layernorm(const float* x, int ldx, float* y, int ldy, const float* g, const float* b,
                      int M, int D, int Dout, float eps, hipStream_t s);

// out[t][c] = (res? res[t][c] : 0) + v[t][c] + sum_j w[c][j] * v[t + j - (k-1)/2][c], per utterance
// segment [off[b], off[b]+len[b]) with zero padding outside the segment.  C % 4 == 0, k == 11.
void launch_fsmn(const float* v, int ldv, const float* w, const float* res, int ldres, float* out,
                 int ldo, const int* off, const int* len, int B, int max_len, int C, hipStream_t s);
// Same with the window shifted into the past by `shift` frames (UPSTREAM sanm_shfit): taps cover
// [t - 5 - shift, t + 5 - shift]; shift is 0 or 5 (5 = fully causal, the vad-realtime punctuation model).
void launch_fsmn_shift(const float* v, int ldv, const float* w, const float* res, int ldres, float* out,
                       int ldo, const int* off, const int* len, int B, int max_len, int C, int shift, hipStream_t s);

// Operands of packed multi-head attention: O[q, h*hd:(h+1)*hd] = softmax(scale * Q_h K_h^T) V_h over the utterance's own keys.
// q segments (q_off, q_len), kv segments (kv_off, kv_len), all device arrays.  An absent field is nullptr / 0 / false.
struct AttnOp {
  const float* Q = nullptr; int ldq = 0;
  const float* K = nullptr; int ldk = 0;
  const float* V = nullptr; int ldv = 0;
  float* O = nullptr; int ldo = 0;
  const int* q_off = nullptr; const int* q_len = nullptr;
  const int* kv_off = nullptr; const int* kv_len = nullptr;
  int B = 0, H = 0, max_q_len = 0;
  float scale = 1.0f;
  int head_dim = kHeadDim;
  // With a per-query key limit: query row i (packed index) only sees keys [0, min(kv_len, q_kv_limit[i])) — the
  // prefix mask CTTransformerOnline::VadMask builds (ct-transformer-online.cpp:225-240).  The fp32-MFMA kernel only.
  const int* q_kv_limit = nullptr;
  // fsmn_w != nullptr (self-attention only: q segments == kv segments; the split-operand kernels, launch_attention_fsmn): the kernel
  // also writes the encoder layer's FSMN memory mem = V + depthwise conv k = 11 over time (what launch_fsmn computes, bit for bit)
  // for its rows and its head's channels; mem_accumulate: mem += instead.
  const float* fsmn_w = nullptr; float* mem = nullptr; int ldmem = 0; bool mem_accumulate = false;
  // the context as fp16 plane images (gemm_p3.hip's A operand) instead of fp32 rows; with planes_hi set, O is not written
  // (attention_x3.hip, attention_p3.hip)
  void* planes_hi = nullptr; void* planes_lo = nullptr; int plane_rows = 0;
  // attention_p3.hip: K / V given as row-major planes instead of K / V above (row stride ldkv elements, K at column 0, V at column
  // v_col of each plane; head h in columns 128 h ..)
  const void* kv_hi = nullptr; const void* kv_lo = nullptr; int ldkv = 0, v_col = 0;
};
// Plain attention (the fused memory block and the plane-image fields of op are not honoured on any kernel), kernel by head width: 128, 80 (the small Paraformer: 320 / 4 heads) or
// 32 (CT-Transformer: 256 / 8 heads).  d_k = 128 with more than 64 queries per utterance runs the split-operand kernels, d_k = 80
// with more than 64 attention_h80.hip unless the launch context is exact; q_kv_limit keeps the fp32-MFMA kernel.
void launch_attention(const AttnOp& op, hipStream_t s);
// both attention products on the BF16 matrix cores (exact three-way split, attention_x6.hip); d_k = 128, no per-query limits
void launch_attention_x6(const AttnOp& op, hipStream_t s);
// the same with two fp16 planes and three products per block (attention_x3.hip)
void launch_attention_x3(const AttnOp& op, hipStream_t s);
// attention_x3.hip's fused attention on K / V given as row-major planes (op.kv_hi ..): tiles staged by LDS-DMA, V read through
// gfx950's transposing LDS read.  d_k = 128.
void launch_attention_p3(const AttnOp& op, hipStream_t s);
// d_k = 80 in the same arithmetic class (attention_h80.hip): two fp16 planes, three products per block on v_mfma_f32_32x32x16_f16,
// fp32 accumulation, online softmax; V^T padded to 96 rows in LDS.  fp32 rows out; no fused memory block, no plane images.
void launch_attention_h80(const AttnOp& op, hipStream_t s);
// Plain fp32 attention for any head width 1 <= op.head_dim <= 64 (the exact-width form of attention.hip's kernel; the large CT-Transformer: 516 / 12 = 43):
// the arithmetic of launch_attention's fp32-MFMA kernel, q_kv_limit included, on heads that start at any multiple of 4 bytes.  Reads
// and writes columns [h * head_dim, (h + 1) * head_dim) of a row and nothing else.  launch_attention does not route here.
void launch_attention_dk(const AttnOp& op, hipStream_t s);
// Encoder-layer pair: FSMN memory of V (into mem) + self-attention (into O) over the q segments.  One launch where the BF16
// attention kernel runs (d_k = 128, more than 64 queries per utterance), otherwise launch_fsmn + launch_attention.
void launch_attention_fsmn(const AttnOp& op, hipStream_t s);
// whether launch_attention_fsmn can write the context as fp16 plane images (gemm_p3.hip's A operand) instead of fp32 rows: the
// fused launch on attention_x3.hip only.
bool attention_planes_ok(int max_len, int head_dim = kHeadDim);
// whether launch_attention_fsmn will be the single fused launch (then, and only then, mem_accumulate is honoured: the caller may
// pass the residual stream as `mem` and drop the memory term from the output projection)
bool attention_fsmn_is_fused(int max_len, int head_dim = kHeadDim);      // never at d_k = 80

// ---- timestamp head (SURVEY §8a row a6 producer; blstm.hip) -------------------------------------------------------
// Bidirectional LSTM, hidden 512, over packed sequences (off/len in frames, B <= 32): gx [rows, 4096] = input projections
// + biases (forward i,f,g,o | backward i,f,g,o), whh [2][2048][512], y [rows, 1024]; hx = kBlstmScratchFloats floats of
// scratch, ZEROED ONCE by the caller; its word kBlstmFlagWord is an error flag the kernel sets (1 = step barrier timed
// out, 2 = the blocks of a direction were not all on one XCD) — check it after the stream has drained.
constexpr int kBlstmScratchFloats = 2 * 4 * 32 * 512 + 8;      // exchange ring [2 dir][4][32][512], then 8 state words
constexpr int kBlstmFlagWord = 2 * 4 * 32 * 512 + 2;
hipError_t launch_blstm(const float* gx, const float* whh, float* y, float* hx, const int* off, const int* len, int B, int Lmax,
                        hipStream_t s);
// The same recurrence as one launch per time step (no inter-block exchange inside a launch: works whatever else runs on the
// device); cst = 2 * 32 * 512 floats of cell state.  Same results bit for bit.
hipError_t launch_blstm_stepwise(const float* gx, const float* whh, float* y, float* hx, float* cst, const int* off, const int* len, int B,
                                 int Lmax, hipStream_t s);
void launch_alpha2(const float* y, int ldy, const float* w, float b, float smooth, float noise, float* a2, int rows, int D,
                   hipStream_t s);
void launch_us_cif(const float* a2, const int* off, const int* len, const int* token_num, int B, int max_len, float threshold,
                   float* us_alphas, float* us_peaks, hipStream_t s);

// ---- predictor / CIF (SURVEY §8a rows a4,a12) -------------------------------------------------
// col[row] = [h[t-1] | h[t] | h[t+1]] with zeros outside the utterance.  row_pos/row_len give the
// local index and utterance length of every packed row.
void launch_im2col3(const float* h, int ldh, float* col, int ldc, const int* row_pos,
                    const int* row_len, int M, int D, hipStream_t s);
// alphas[row] = relu(sigmoid(dot(o[row], w) + b) * smooth - noise)
void launch_alpha(const float* o, int ldo, const float* w, const float* b, float smooth,
                  float noise, float* alphas, int M, int D, hipStream_t s);
// CIF integrate-and-fire per utterance (paraformer-online.cpp:301-327) with the tail slot
// (alpha = tail, hidden = 0) appended.  Writes fired frames to stage[(row_off[b]+b+n)][0..D),
// n_fires[b], token_num[b] = floor(sequential fp32 sum of alphas incl. tail).
// fire_frame (optional, [sum len + B] ints): the sibling kernel that also stores the step each token fired in, fire nf of
// utterance b at row_off[b] + b + nf (0..len-1 an LFR row, len the tail slot); NULL launches exactly the default kernel
void launch_cif(const float* hidden, int ldh, const float* alphas, const int* row_off,
                const int* len, int B, int D, float threshold, float tail, float* stage,
                int* n_fires, int* token_num, hipStream_t s, int* fire_frame = nullptr);
// emb[tok_off[b]+n] = stage[row_off[b]+b+n]
void launch_compact(const float* stage, float* emb, const int* tok_row_src, int ML, int D,
                    hipStream_t s);

// ---- hotword embedder ------------------------------------------------------------
// out[r] = table[ids[r]]  (Embedding lookup, D % 4 == 0)
void launch_gather_rows(const int32_t* ids, const float* table, int D, float* out, int R, hipStream_t s);
// One LSTM step on pre-activations G [H, 4D] (torch gate order i,f,g,o): c = sig(f)*c + sig(i)*tanh(g);
// h = sig(o)*tanh(c); rows with lens[j]-1 == t also copy h into sel[j].
void launch_lstm_cell(const float* G, float* c, float* h, const int32_t* lens, int t, float* sel, int H, int D,
                      hipStream_t s);

// ---- CT-Transformer helpers (punc.hip) ---------------------------------------------------------
// out[row][0..D) = table[clamp(ids[row], 0, vocab - 1)] * scale + PE(pos + 1), pos = pos_of_row ? pos_of_row[row] : row; columns
// D..Dout zeroed (Dout <= ldo)
void launch_embed_gather(const int32_t* ids, const float* table, int vocab, int D, int Dout, float* out, int ldo, int N,
                         const float* inv_ts, float scale, const int* pos_of_row, hipStream_t s);
// out[row] = the first maximum over columns [0, ncls) of the row (std::max_element, ct-transformer.cpp:193-196)
void launch_argmax_first(const float* logits, int ldl, int N, int ncls, int32_t* out, hipStream_t s);

// ---- head -----------------------------------------------------------------
// per row: log-softmax over V logits, argmax (first max wins, util.cpp:63-74).  logp may be null.
// range_flag (may be null): bit 0 is raised when a row's log-sum-exp is not finite (NaN / Inf reached the logits).
void launch_logsoftmax_argmax(const float* logits, int ldl, int ML, int V, float* logp, int32_t* ids,
                              hipStream_t s, int* range_flag = nullptr);
// ---- CTC head and collapse (ctc_head.hip) --------------------------------------------------------------------------------------
// The head of a CTC model without its logits matrix: per row of X [M, K] (K % 32 == 0; exactly M rows are read) the arg-max over
// x W^T + bias (W [V, K], exactly V rows; first maximum wins), logp_best = that logit - log-sum-exp of the row, and (lse non-null)
// the log-sum-exp.  Arithmetic of gemm_x3.hip with the given power-of-two w_scale.  workspace: ctc_head_workspace_bytes(M, V) bytes
// of per-tile (max, arg-max, sum exp) partials.  false (nothing launched) for what the kernels do not take.
size_t ctc_head_workspace_bytes(int M, int V);
bool launch_ctc_head(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int32_t* ids,
                     float* logp_best, float* lse, void* workspace, size_t workspace_bytes, hipStream_t s, int* range_flag = nullptr);
// SenseVoice's four prompt rows: rows row_off[b] .. + 3 of feats (row stride ld) = rows prompt[4 b .. 4 b + 3] of E [16][D], for every
// utterance with rows (len[b] >= 4; device arrays).  best[r] = logp[r][ids[r]].
void launch_svs_prompt_rows(const float* E, int D, const int* prompt, const int* row_off, const int* len, int B, float* feats, int ld,
                            hipStream_t s);
void launch_gather_best(const float* logp, int ld, const int32_t* ids, int M, float* best, hipStream_t s);
// lse[r] = log-sum-exp of logits[r][0 .. V): what the unfused head keeps where the fused one's merge kernel writes `lse`
void launch_row_lse(const float* logits, int ld, int M, int V, float* lse, hipStream_t s);
// CTC collapse per utterance b over frames [row_off[b], row_off[b] + len[b]) (device arrays): a frame is kept when its id is not
// `blank` and differs from the previous frame's.  ids / tok_frame / tok_logp [B][max_tokens] (the two last may be null): the kept
// id, its 0-based frame inside the utterance and a copy of frame_logp there; token_num[b] = the number kept, also beyond max_tokens
// (tokens past max_tokens are counted, not stored).  ctc_collapse_chunk(): the frames one trip of the scan covers.
int ctc_collapse_chunk();
bool launch_ctc_collapse(const int32_t* frame_ids, const float* frame_logp, const int* row_off, const int* len, int B, int blank,
                         int max_tokens, int32_t* ids, int32_t* tok_frame, float* tok_logp, int32_t* token_num, hipStream_t s);
// ---- CTC forced alignment (ctc_align.hip) ---------------------------------------------------------------------------------------
// Emissions of the labels asked for: utterance b owns rows [row_off[b], + len[b]) of X and labels[lab_off[b] .. + n_lab[b]) (device
// arrays); E + e_off[b] is E_b [len[b]][n_lab[b] + 1] = x_t . W[id_j] + bias[id_j] - lse[row], column 0 the blank, column j label j.
// fp32 FMA.  K % 32 == 0, row strides % 4 == 0.  Rows are clamped to the utterance, label ids to 0 .. V - 1.  false: nothing launched.
// e_floats >= 0: the floats of E, and an utterance whose E_b does not lie inside them is left unwritten (sizes planned on the device).
bool launch_ctc_emissions(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* lse, const int* row_off,
                          const int* len, const int* lab_off, const int* n_lab, const int32_t* labels, const long long* e_off, int B, int K,
                          int V, int blank, float* E, hipStream_t s, long long e_floats = -1);
// The step between the collapse and the two kernels above, on the device: from token_num [B] (the collapse's) and speech_len [B] (the
// rows N_b the labels are aligned against) n_lab[b] = max(token_num[b] - 4, 0), lab_off[b] = b maxT + 4 (the labels are the collapse's
// id buffer [B][maxT] behind the four tags), e_off[b] = the exclusive int64 prefix sum of N_b (n_lab[b] + 1), *total (may be null) =
// the sum over all b.  n_lab[b] = -1 (both kernels then leave the utterance alone) where E_b would end beyond cap_floats, and — with
// nothing added to the sum — where token_num[b] > maxT or N_b < 0.  One workgroup; B <= 65535.  false: nothing launched.
bool launch_ctc_greedy_plan(const int32_t* token_num, const int* speech_len, int B, int maxT, long long cap_floats, int* n_lab, int* lab_off,
                            long long* e_off, long long* total, hipStream_t s);
// Viterbi over the CTC trellis of each utterance and the token spans (include/pfhip_ops.h states the recurrence).  e_floats: the floats
// of E; workspace: ctc_align_workspace_bytes(e_floats) bytes of back-pointers.  tok_begin / tok_end / tok_logp [B][max_tokens] (tok_logp
// may be null), score [B].  false (nothing launched) for max_tokens above ctc_align_max_tokens() (the two score rows of 2 L + 1 states
// must fit 64 KB of LDS), a short workspace or a null buffer.  An utterance whose n_lab exceeds max_tokens or whose E_b leaves E is
// answered as infeasible.
size_t ctc_align_workspace_bytes(size_t e_floats);
int ctc_align_max_tokens();
bool launch_ctc_align(const float* E, const long long* e_off, size_t e_floats, const int* len, const int* n_lab, const int32_t* labels,
                      const int* lab_off, int B, int max_tokens, int32_t* tok_begin, int32_t* tok_end, float* tok_logp, float* score,
                      void* workspace, size_t workspace_bytes, hipStream_t s);
// The fused CTC head with the k best columns of every row (ctc_head.hip; 1 <= k <= kCtcTopkMax, V >= k): ids / logp_best / lse are
// launch_ctc_head's bit for bit (the same tile arithmetic; the greedy tile kernel is a separate instantiation that does not change);
// topk_ids / topk_logp [M][k], larger logit first, equal logits smaller column first, value = (logit - row maximum) - log(sum): logit - lse, and logp_best at rank 0.
// workspace: ctc_head_topk_workspace_bytes(M, V, k) bytes — per row and tile k (value, column) pairs on top of the greedy triple.
constexpr int kCtcTopkMax = 16;
size_t ctc_head_topk_workspace_bytes(int M, int V, int k);
bool launch_ctc_head_topk(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int k,
                          int32_t* ids, float* logp_best, float* lse, int32_t* topk_ids, float* topk_logp, void* workspace,
                          size_t workspace_bytes, hipStream_t s, int* range_flag = nullptr);
// The k best columns of every row of a log-prob matrix [rows][V] the unfused head formed (the exact re-run of the range guard, a caller
// who wants full rows): topk_ids / topk_logp [rows][k], larger value first, equal values lower column first; 1 <= k <= kCtcTopkMax, V >= k.
bool launch_row_topk(const float* logp, int ld, int rows, int V, int k, int32_t* topk_ids, float* topk_logp, hipStream_t s);
// ---- CTC prefix beam search with hotwords (ctc_beam.hip) ------------------------------------------------------------------------
// The context graph on the device (ctx_graph.h in CSR form; n_states == 0: no graph).  Indices are the host builder's, validated there.
struct CtxGraphDev {
  const int32_t* arc_begin = nullptr;            // [n_states + 1]
  const float* escape = nullptr;                 // [n_states]
  const int32_t* arc_label = nullptr;            // [n_arcs], sorted inside a state
  const int32_t* arc_next = nullptr;
  const float* arc_weight = nullptr;
  int n_states = 0, n_arcs = 0;
};
// One workgroup per utterance walks rows [row_off[b], + len[b]) (device arrays) of topk_ids / topk_logp [rows][k] in order
// (include/pfhip_ops.h states the recurrence and the tie rule).  1 <= first_beam <= k <= kBeamMax, 1 <= nbest <= second_beam <=
// kBeamMax.  Out, per utterance: n_hyp [B]; ids [B][nbest][max_tokens]; n_tokens / score / ctc_score / ctx_score [B][nbest].
// workspace: ctc_prefix_beam_workspace_bytes(rows, B, second_beam) bytes of trie nodes (the utterances' row ranges must not overlap:
// an utterance's nodes live at its rows' positions).  false: nothing launched.
constexpr int kBeamMax = 16;
size_t ctc_prefix_beam_workspace_bytes(long long rows, int B, int second_beam);
bool launch_ctc_prefix_beam(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len, int B,
                            int V, int blank, int first_beam, int second_beam, const CtxGraphDev& graph, int nbest, int max_tokens,
                            int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score, float* ctx_score,
                            void* workspace, size_t workspace_bytes, hipStream_t s);
// The same search with every utterance on its own parameters: workgroup b reads utt[b] (a DEVICE array [B]) — first_beam 0: no search
// for b (n_hyp 0); graph: an index into graphs (a DEVICE table [n_graphs]), -1: none.  The top-k rows have stride k and utterance b
// reads their first first_beam[b] columns; trie nodes sit at the utterance's rows with stride sb_max (workspace:
// ctc_prefix_beam_workspace_bytes(rows, B, sb_max)); outputs are [B][nbest_max]([max_tokens]), slots from nbest[b] on filled as the
// slots behind n_hyp.  A descriptor outside the strides is answered as n_hyp 0 by the kernel; ctc_prefix_beam_multi_check is the
// host's check of a HOST copy of the descriptors (beams 0..16, first_beam <= k, 1 <= nbest <= second_beam where first_beam > 0, graph
// in -1 .. n_graphs - 1) and gives the two maxima (at least 1).
struct BeamUtt { int first_beam, second_beam, nbest, graph; };
bool ctc_prefix_beam_multi_check(const BeamUtt* utt, int B, int k, int n_graphs, int* sb_max, int* nbest_max);
bool launch_ctc_prefix_beam_multi(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                  int B, int V, int blank, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, int sb_max,
                                  int nbest_max, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                                  float* ctc_score, float* ctx_score, void* workspace, size_t workspace_bytes, hipStream_t s);
// ---- hotword-biased beam search over a non-autoregressive head's candidates (nar_beam.hip) --------------------------------------
// One workgroup per utterance walks rows [row_off[b], + len[b]) (device arrays) of cand_ids / cand_logp [rows][k] in order, one token
// per row (include/pfhip_ops.h states the recurrence and the tie rule).  Workgroup b reads utt[b] (a DEVICE array [B]) with
// first_beam as the WIDTH (the row's first `width` columns are its candidates), second_beam as the beam, nbest, and graph an index
// into graphs (a DEVICE table [n_graphs]; -1: none): 1 <= width <= k <= kNarWidthMax, 1 <= nbest <= beam <= kBeamMax.  Trie nodes
// sit at the utterance's rows with stride beam_stride (workspace: nbest_ctx_beam_workspace_bytes(rows, B, beam_stride); the row
// ranges must not overlap); outputs are [B][nbest_stride]([max_tokens]).  A descriptor outside the strides (width 0 included: "no
// search") is answered as n_hyp 0 by the kernel; nbest_ctx_beam_check is the host's check of a HOST copy of the descriptors
// (allow_none: width 0 passes unread) and gives the two maxima (at least 1).  len_cap (a DEVICE array [B], or null): utterance b
// walks min(len[b], len_cap[b]) rows.  false: nothing launched.
constexpr int kNarWidthMax = 8;
size_t nbest_ctx_beam_workspace_bytes(long long rows, int B, int beam_stride);
bool nbest_ctx_beam_check(const BeamUtt* utt, int B, int k, int n_graphs, bool allow_none, int* beam_max, int* nbest_max);
bool launch_nbest_ctx_beam(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len,
                           const int* len_cap, int B, int V, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, int beam_stride, int nbest_stride,
                           int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* am_score, float* ctx_score,
                           void* workspace, size_t workspace_bytes, hipStream_t s);
// ---- token n-gram language model (lm_graph.h on the device; lm_step.h walks it, lm_score.hip scores sentences with it) ------------
// n_states == 0: no model.  Indices are the host builder's, validated there; lm_step clamps them all the same.
constexpr int kLmOrderMax = 6;
struct LmGraphDev {
  const float* uni_w = nullptr;                  // [vocab + 1]
  const int32_t* uni_next = nullptr;             // [vocab + 1]
  const int32_t* arc_begin = nullptr;            // [n_states + 1]
  const float* backoff_w = nullptr;              // [n_states]
  const int32_t* backoff_state = nullptr;        // [n_states]
  const int32_t* arc_label = nullptr;            // [n_arcs], sorted inside a state
  const int32_t* arc_next = nullptr;
  const float* arc_weight = nullptr;
  int n_states = 0, n_arcs = 0, vocab = 0, start = 0, has_eos = 0;
};
// One lane per sentence: sentence b is ids[b * max_len .. + len[b]) (device arrays; len clamped to 0 .. max_len, an id clamped to
// 0 .. vocab - 1).  tok_w [B][max_len]: the weight of every token from the start state on (0 behind the sentence); eos_w [B]: the
// weight of </s> behind the last token (0 without has_eos); total [B]: their fp32 sum, left to right.  false: nothing launched.
bool launch_lm_score(const int32_t* ids, const int* len, int B, int max_len, const LmGraphDev& g, float* tok_w, float* eos_w, float* total,
                     hipStream_t s);
// The nar_beam.hip search with a language model walked beside the context graph (lm.n_states > 0; lm.vocab == V): every hypothesis
// also carries the model's state and its score so far, which joins the total; lm_score [B][nbest_stride] is that share (0 behind
// n_hyp).  Its own kernel instantiation: launch_nbest_ctx_beam runs what it ran before.
bool launch_nbest_ctx_beam_lm(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len,
                              const int* len_cap, int B, int V, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm,
                              int beam_stride, int nbest_stride, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                              float* am_score, float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, hipStream_t s);
// ... and launch_ctc_prefix_beam_multi the same way (ctc_beam.hip): a hypothesis's model state and score belong to its prefix.
bool launch_ctc_prefix_beam_multi_lm(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                     int B, int V, int blank, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm,
                                     int sb_max, int nbest_max, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                                     float* ctc_score, float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, hipStream_t s);
// The same head with the k best columns of every row (topk.hip; 1 <= k <= kTopkMax <= V): topk_ids / topk_logp [ML][k], larger logit
// first, equal logits smaller column first, so topk_ids[.., 0] == ids; a value equals the logp entry of its column bit for bit.  The
// log-sum-exp is formed with logp null as well.  false (nothing launched) when the arguments are outside that.
constexpr int kTopkMax = 8;
bool launch_logsoftmax_topk(const float* logits, int ldl, int ML, int V, int k, float* logp, int32_t* ids, int32_t* topk_ids,
                            float* topk_logp, hipStream_t s, int* range_flag = nullptr);

// ---- chunk-streaming pieces ----------------------------------------------
// Per-connection operations of a streaming batch, many in one launch: one descriptor per operation (arrays in HBM).
// rows_copy: dst[r][0..ncols) = src[r][0..ncols) (or 0 when src == nullptr), columns ncols..ldd zeroed.
// stream_lfr: OnlineLfrCmvn + x*sqrt(d) + GetPosEmb (paraformer-online.cpp:196-238, 549-555, 240-268) for `n_rows` LFR rows: row i =
// frames [6i, 6i+7) of fb (T frames incl. the splice cache), the tail replicated with the last frame;
// out[i] = ((x + mean) * istd) * scale + PE(pos0 + i + 1).  out has row stride ldo.
struct RowsCopyOp { float* dst; const float* src; int ldd, lds, nrows, ncols; };      // src == nullptr: zeros; lds == 0: row 0 repeated
struct StreamLfrOp { const float* fb; float* out; int T, n_rows, pos0, pad_; };
void launch_rows_copy_batch(const RowsCopyOp* ops, int n_ops, int max_rows, hipStream_t s);
void launch_stream_lfr_batch(const StreamLfrOp* ops, int n_ops, int max_rows, const float* mean, const float* istd, float scale,
                             const float* inv_ts, int ldo, hipStream_t s);
// One connection of a streaming batch (device-side descriptor): its window in the packed encoder matrices, its tokens in
// the packed decoder matrices (filled in after the CIF counts are known), and its persistent state.
struct StreamSeg {
  float* carry;        // CIF hidden_cache_ [D] followed by alphas_cache_ [1]
  float* dcache;       // decoder FSMN caches [layers][10][D]
  int row_off, n;      // window rows
  int is_last, pre, suf;       // CifSearch: last chunk flag, alphas outside [pre, suf) are zeroed (paraformer-online.cpp:279-286)
  int tok_off, n_tok;  // fired tokens
  int pad_;
};
// CifSearch (paraformer-online.cpp:270-345) for B connections at once; stream b's fires land in emb_all[b * emb_rows ..],
// their count in n_fire[b] (counts above emb_rows are reported but not stored: the caller checks).  fire_step (may be null: the
// kernel and launch as ever) [B * emb_rows]: the scan step in which stored token j of stream b fired, at [b * emb_rows + j]
// (0 = the carry slot, 1..n = window rows 0..n-1, n + 1 = the tail slot); slots of tokens that did not fire are left alone.
void launch_cif_stream(const float* enc, int lde, const float* alphas, const StreamSeg* segs, int B, float threshold, float tail,
                       float* emb_all, int emb_rows, int* n_fire, int D, hipStream_t s, int* fire_step = nullptr);
// Decoder FSMN with the 10-frame cache (paraformer-online.cpp:374, 500) for the packed tokens of B connections.
void launch_fsmn_cached(const float* t2, const float* w, const float* res, float* out, const StreamSeg* segs, int B, int layer,
                        int C, hipStream_t s);

// ---- fused kernels for ONE streaming window (stream_fused.hip): M <= 32 rows ---------------------------------------------
// Operands of C[M,N] = act(LN?(X) W^T + bias) (+R1) (+R2) (+ FSMN memory of fsmn_v) over the rows of one window; an absent field
// is nullptr / 0 / false.  A launcher whose kernel has no parameter for a field that is set refuses the op (see each).
struct WindowGemmOp {
  const float* X = nullptr; int ldx = 0;
  const float* W = nullptr; int ldw = 0;
  float* C = nullptr; int ldc = 0;
  int M = 0, N = 0, K = 0;
  const float* bias = nullptr;
  const float* R1 = nullptr; int ldr1 = 0;
  const float* R2 = nullptr; int ldr2 = 0;
  bool relu = false;
  float eps = 1e-12f;
  // the SAN-M memory term: + fsmn_v + depthwise conv k = 11 (taps fsmn_w) of fsmn_v over the M rows
  const float* fsmn_v = nullptr; int ldv = 0; const float* fsmn_w = nullptr;
  // LayerNorm of X in front, one form at most.  Explicit (launch_fused_ln_gemm): gamma ln_g, beta ln_b over columns [0, D), D <= K
  // (columns D..K of the normalised operand are 0).  Algebraic (launch_fused_gemv_1trip): ln_colsum, the column sums of W, with W /
  // bias the gamma/beta-folded ones; the LayerNorm is over exactly the K operand columns (D is 0 or K).
  const float* ln_g = nullptr; const float* ln_b = nullptr; int D = 0;
  const float* ln_colsum = nullptr;
};
// One workgroup per 32 columns or fewer (fused_ln_gemm_route).  Serves every field but ln_colsum: an op that carries it is a
// programming error and aborts, as launch_gemm does for a fold that reaches the wrong kernel.
void launch_fused_ln_gemm(const WindowGemmOp& op, hipStream_t s);
// The same operator with every operand requested in one trip (fused_gemv_1trip_route).  Returns false, launching nothing, for the
// shapes it does not take and for an op with R2 or ln_g (or a LayerNorm width D other than K): the caller falls back to
// launch_fused_ln_gemm with the plain weights.
bool launch_fused_gemv_1trip(const WindowGemmOp& op, hipStream_t s);
// Attention of windows of at most 32 queries and 32 keys, d_k = 128 or 80: one small workgroup per head and window, operands
// requested at kernel start.  max_kv_len: the host-side maximum of the key counts, as op.max_q_len is of the query counts.
// op.q_off == nullptr: ONE window — max_q_len queries and max_kv_len keys starting at the pointers, grid (H), no segment array is
// read (none may be set, nor fsmn_w / mem).  Otherwise B windows by the four segment arrays, grid (H, B); with fsmn_w
// (self-attention: q segments == kv segments) the launch also writes the FSMN memory of V into mem, what launch_fsmn computes.
// Returns false, launching nothing, for shapes it does not take and for an op with a field it does not serve (q_kv_limit,
// mem_accumulate, plane images, K / V planes): the caller uses launch_attention.
bool launch_window_attention(const AttnOp& op, int max_kv_len, hipStream_t s);
// ONE window's attention (att, the one-window form above: 4 heads of 128, max_q_len <= 20, max_kv_len <= 32; att.O is not written)
// AND the projection of its context by proj.W [N, 512] (+bias, +R1, + the FSMN memory) in one launch: every workgroup redoes the
// attention and keeps the context in LDS, so proj.X and proj.M are unused (the rows are att.max_q_len).  False, launching nothing,
// outside that and for a proj with R2, relu or a LayerNorm.
bool launch_fused_att_out(const AttnOp& att, int max_kv_len, const WindowGemmOp& proj, hipStream_t s);
// Which instantiation and launch geometry the two GEMM launchers above take for a shape: host arithmetic only (nothing is launched, no
// device is needed), the environment knobs of this process included.  The launchers launch exactly what these return — the one
// place the choice is made.
struct Gemv1tRoute {        // fused_gemv1t_kernel<LN, FS, CW, CPL, 4, RPL, NF> on `waves` waves; ok == false: refused (all else 0)
  bool ok, ln, fs;
  int cw, cpl, rpl, nf, waves;
};
Gemv1tRoute fused_gemv_1trip_route(int M, int N, int K, bool has_ln, bool has_fsmn);
enum LnGemmKernel { kLnGemmNone = 0, kLnGemmVector = 1, kLnGemmMatrix = 2 };      // none: M <= 0 or N <= 0, nothing to launch
struct LnGemmRoute {        // fused_ln_gemv_kernel<LN, CW, MR> (vector) or fused_ln_gemm_kernel<LN, CW> (matrix: MR = 32, 16 waves)
  LnGemmKernel kernel;      // k_blocks: the k-blocks the waves share (K / (256 / CW) in the vector form, K / 8 in the matrix form)
  bool ln;
  int cw, mr, waves, k_blocks;
};
LnGemmRoute fused_ln_gemm_route(int M, int N, int K, bool has_ln);

// ---- FSMN-VAD pieces --------------------------------------------------------------
// Generic LfrCmvn over raw fbank frames fb [F, n_mels] -> out [T = ceil(F/n), ldo] (columns >= m*n_mels zeroed).
void launch_lfr_cmvn(const float* fb, int F, int T, int m, int n, int n_mels, const float* mean, const float* istd,
                     float* out, int ldo, hipStream_t s);
// Memory block with left order 20: out = p + causal depthwise conv over [cache(19 rows); p]; cache_out (may be
// null) receives the last 19 rows of [cache_in; p] and must not alias cache_in.
// One connection's share of a packed FSMN-VAD forward: rows [row_off, row_off + T), network caches [layers][19][C]
// (cache_out == nullptr: do not advance, the final call of fsmn-vad.cpp:129-134).
struct VadSeg { const float* cache_in; float* cache_out; int row_off, T; };
struct VadLfrOp { const float* fb; int Tin, n_out, row_off, pad_; };
void launch_fsmn_causal20(const float* p, int ldp, const float* w, const VadSeg* segs, int B, int max_T, int layer, float* out,
                          int ldo, int C, hipStream_t s);
// OnlineLfrCmvn (fsmn-vad-online.cpp:90-133) for many connections: row i of operation k = frames [i*n, i*n + m) of its fb (which starts
// with the splice cache; Tin frames), the tail replicated with the last frame, no left padding; rows row_off .. + n_out of out.
void launch_lfr_cmvn_online_batch(const VadLfrOp* ops, int n_ops, int max_rows, int m, int n, int n_mels, const float* mean,
                                  const float* istd, float* out, int ldo, hipStream_t s);
void launch_softmax_rows(const float* x, int ldx, int M, int N, float* y, float* col0, hipStream_t s);
// The offline LfrCmvn (fsmn-vad.cpp:198-238) for B files whose fbank frames lie back to back in fb (frame_off[b], nframes[b]): every
// file is padded at its own edges, its T_b = ceil(nframes[b] / n) rows go to rows row_off[b].. of out; max_T = the largest T_b.  Row
// for row what launch_lfr_cmvn writes for the file alone.
void launch_lfr_cmvn_packed(const float* fb, const int* frame_off, const int* nframes, const int* row_off, int B, int max_T, int m, int n,
                            int n_mels, const float* mean, const float* istd, float* out, int ldo, hipStream_t s);
// Frame energies of the end-point detector's decibel track (vad_energy.hip): B utterances packed in pcm as for
// launch_fbank_frames_batch (sample_off int64, frame_off [B + 1], nframes [B], device arrays; nframes[b] = n < flen ? 0 :
// 1 + (n - flen) / fshift); e[frame_off[b] + f] = sum_{i < flen} x[f * fshift + i]^2 in one fp32 accumulator, i ascending, products
// rounded before they are added: bit for bit VadSegmenter::AppendDecibel's sum.  s16: x = (float)s * (1 / 32768), exact; an utterance
// may start at an odd sample.  false (nothing launched) when 63 * fshift + flen samples do not fit 64 KB of LDS.
bool launch_frame_energy(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                         int flen, int fshift, float* e, hipStream_t s);
bool launch_frame_energy(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                         int flen, int fshift, float* e, hipStream_t s);

// ---- resampling ahead of the front end (resample.hip; plan: resample.cpp) ----------------------
// The device image of one rate pair's polyphase plan (Kaldi LinearResample, onnxruntime/src/resample.cpp:104-153):
// per output phase ph < Q its first input index first[ph], its tap count ntap[ph] <= K and its weight row w[ph * K ..].
// Output sample s of an utterance reads inputs first[s % Q] + (s / Q) * P + j, j < ntap[s % Q].
struct ResampleTable { const int* first; const int* ntap; const float* w; int P, Q, K; };
// Packed batch: utterance b reads n_in[b] samples at in + in_off[b] and writes n_out[b] samples at out + out_off[b]
// (host arrays; n_out from the flush-mode count).  Bitwise the reference's serial fp32 dot product per output.
void launch_resample(const float* in, const int64_t* in_off, const int* n_in, float* out, const int64_t* out_off, const int* n_out,
                     int B, const ResampleTable& t, hipStream_t s);
// 16-bit PCM in (offsets in samples, 2-byte alignment assumed): every sample is converted (float)s * (1.f / 32768.f) on load, the tap
// loop and its order are the same, the output stays f32 — bit for bit launch_resample of s / 32768.f.
void launch_resample(const int16_t* in, const int64_t* in_off, const int* n_in, float* out, const int64_t* out_off, const int* n_out,
                     int B, const ResampleTable& t, hipStream_t s);

// ---- the DNSMOS networks (conv3x3.hip, dnsmos.hip) ---------------------------------------------
// 3x3 / pad 1 / stride 1 convolution + bias + ReLU on NHWC fp32 activations, x [N][H][W][Cin] -> y [N][H][W][Cout], or with `pool`
// the 2x2 / stride 2 floor max-pool of that, y [N][H / 2][W / 2][Cout].  Every launcher returns false, having launched nothing, for
// what its kernel does not take.
// Cin 32 or a multiple of 64, Cout 32 or 64: implicit GEMM on two fp16 planes.  The weights are packed once (launch_conv3x3_pack: ONNX
// [Cout][Cin][3][3] fp32 -> two plane images of conv3x3_plane_bytes(Cin, Cout) bytes each, times the power of two `scale` =
// best_w_scale(max |w|)) and the same scale is passed to the convolution as w_scale.  N <= 65535.
size_t conv3x3_plane_bytes(int Cin, int Cout);
bool launch_conv3x3_pack(const float* w, int Cin, int Cout, float scale, void* hi, void* lo, hipStream_t s);
bool launch_conv3x3_relu(const float* x, const void* whi, const void* wlo, float w_scale, const float* bias, float* y, int N, int H, int W,
                         int Cin, int Cout, bool pool, hipStream_t s);
// Cin == 1: x [N][H][W], w the ONNX [Cout][1][3][3]; nine FMAs in the order ky, kx ascending.
bool launch_conv3x3_c1_relu(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout, bool pool,
                            hipStream_t s);
// The primary net's front end: window i = the (n_frames + 1) * 160 samples at pcm + win_off[i] (device int64 array; n_win <= 65535),
// frame f = samples [160 f, 160 f + 320); out [n_win][n_frames][161] = log(max(floor_v, sqrt(re^2 + im^2)^2)) / denom with re / im
// against tab [320][2][kDnsmosBinStride], which dnsmos_stft_table builds on the host from the graph's two [161][320] STFT kernels.
// s16: x = (float)s * (1 / 32768), bit for bit the f32 call.
constexpr int kDnsmosBinStride = 168;
constexpr int kDnsmosMelFrames = 900, kDnsmosMels = 120, kDnsmosFft = 321;
void dnsmos_stft_table(const float* wr, const float* wi, float* tab);
bool launch_dnsmos_logpow(const float* pcm, const int64_t* win_off, int n_win, const float* tab, int n_frames, float floor_v, float denom,
                          float* out, hipStream_t s);
bool launch_dnsmos_logpow(const int16_t* pcm, const int64_t* win_off, int n_win, const float* tab, int n_frames, float floor_v, float denom,
                          float* out, hipStream_t s);
// The P.808 net's input: out [n_win][900][120] = (power_to_db(melspectrogram(first 144000 samples of window i), ref = max) + 40) / 40,
// transposed (dnsmos.hip's head says which settings are recalled).  dnsmos_mel_tables fills (host) tab [321][2][kDnsmosBinStride] and
// melT [161][120]; wmax = n_win device words of scratch.
void dnsmos_mel_tables(float* tab, float* melT);
bool launch_dnsmos_melspec(const float* pcm, const int64_t* win_off, int n_win, const float* tab, const float* melT, float* out,
                           unsigned* wmax, hipStream_t s);
bool launch_dnsmos_melspec(const int16_t* pcm, const int64_t* win_off, int n_win, const float* tab, const float* melT, float* out,
                           unsigned* wmax, hipStream_t s);
// The head: max over the HW pixels of x [N][HW][C], then three dense layers y = x W + b with W [in][out] as the graph's MatMul holds
// it, ReLU after the first two; out [N][D3].  C, D1, D2, D3 <= 256.
bool launch_globalmax_mlp(const float* x, int N, int HW, int C, const float* w1, const float* b1, int D1, const float* w2, const float* b2,
                          int D2, const float* w3, const float* b3, int D3, float* out, hipStream_t s);

}  // namespace pfhip
