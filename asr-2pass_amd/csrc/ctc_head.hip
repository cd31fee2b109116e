// CTC head without the logits matrix, and the CTC collapse.
//
// A CTC model projects EVERY encoder row onto the vocabulary (SenseVoiceSmall: ~25 000 columns; widths recalled from upstream
// FunASR, no SenseVoice file was at hand) and the greedy search (CTCSearch, onnxruntime/src/sensevoice-small.cpp:323-377) then
// keeps one arg-max per row.  Written out, the bench batch's logits are 16 128 x 25 055 fp32 = 1.62 GB per forward.  Here the
// projection's epilogue reduces each 128-column tile of a row to (max, lowest column holding it, sum of exp(x - max)) and a
// second small kernel merges a row's tiles in ascending column order: 12 bytes per row and tile leave the GEMM (38 MB).
//
// Arithmetic: that of gemm_x3.hip — two fp16 planes per operand (split_common.h), W staged times the power-of-two w_scale (undone
// in the epilogue), three v_mfma_f32_32x32x16_f16 products per block in the order hi*lo, lo*hi, hi*hi, fp32 accumulation.
// Tile 128 x 128, K-step 16, 256 threads = 4 waves as 2 x 2 of 64 x 64 (2 x 2 MFMA tiles each); operands split while staged into
// a double-buffered LDS stage (2 x 24 576 B, static: 3 workgroups a CU), global loads of step k + 1 issued before the MFMAs of
// step k, one barrier per step.  A plain pipeline: the hand-placed schedule of gemm_f32_f16x3_128_kernel is not reproduced.
// Operand rows are clamped to M - 1 / V - 1, so X needs exactly M rows and W exactly V; what the clamped rows produce is masked
// (columns) or not stored (rows).
#include "kernels.h"
#include "launch_common.h"
#include "split_common.h"

#include <math.h>

#include <algorithm>

namespace pfhip {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kHT = 128;                         // tile rows = tile columns
constexpr int kHK = 16;                          // K-step: one MFMA deep
constexpr int kRowB = 48;                        // bytes per operand row in LDS (16 fp16 + pad: conflict-free 16-byte fragment reads)
constexpr int kPlane = kHT * kRowB;              // 6 144 B
constexpr int kStage = 4 * kPlane;               // X hi, X lo, W hi, W lo
constexpr int kCs = kHT + 4;                     // padded row stride of the C half tile (floats)
constexpr int kHeadLds = 2 * kStage;             // 49 152 B
static_assert(64 * kCs * 4 <= kHeadLds, "a 64-row half of the C tile must fit the operand stages");

template <bool SC>
__device__ __forceinline__ void stage4(const float4& v, float scale, unsigned char* hi, unsigned char* lo) {
  const float x0 = SC ? v.x * scale : v.x, x1 = SC ? v.y * scale : v.y, x2 = SC ? v.z * scale : v.z, x3 = SC ? v.w * scale : v.w;
  const unsigned h01 = hi_pair(x0, x1), h23 = hi_pair(x2, x3);
  *reinterpret_cast<uint2*>(hi) = make_uint2(h01, h23);
  *reinterpret_cast<uint2*>(lo) = make_uint2(lo_pair(sub_lo(x0, h01), sub_hi(x1, h01)), lo_pair(sub_lo(x2, h23), sub_hi(x3, h23)));
}

// partials: [column tile][row] so that the merge kernel's threads (one per row) read consecutive words.  The body of both tile
// kernels below: TOPK = false is the greedy head; TOPK = true also leaves the tile's k best (value, column) pairs of every row in
// pkv / pki [column tile][rank][row] (best first, equal values lower column first; a tile with fewer than k finite logits ends in
// (-inf, INT_MAX) pairs).
template <bool TOPK>
__device__ __forceinline__ void ctc_head_tile(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                              const float* __restrict__ bias, float sw, int M, int V, int K, int tiles_n, int n_tiles, int gw,
                                              float* __restrict__ pmax, int* __restrict__ pidx, float* __restrict__ psum, int k,
                                              float* __restrict__ pkv, int* __restrict__ pki) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kHeadLds];

  int tm, tn;
  tile_of_block(blockIdx.x, n_tiles, tiles_n, gw, tm, tn);
  const int m0 = tm * kHT, n0 = tn * kHT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  // staging map: thread t holds 4 consecutive k of X rows t/4, t/4 + 64 and of W rows t/4, t/4 + 64
  const int srow = tid >> 2, sq = tid & 3;
  const float* Xg0 = X + (size_t)min(m0 + srow, M - 1) * ldx + 4 * sq;
  const float* Xg1 = X + (size_t)min(m0 + srow + 64, M - 1) * ldx + 4 * sq;
  const float* Wg0 = W + (size_t)min(n0 + srow, V - 1) * ldw + 4 * sq;
  const float* Wg1 = W + (size_t)min(n0 + srow + 64, V - 1) * ldw + 4 * sq;
  const int st = srow * kRowB + 8 * sq;                              // byte offset inside a plane (second row: + 64 rows)
  const int x_fr = (wr * 64 + r) * kRowB + 16 * h;                   // fragment: row r of the MFMA tile, k = 8 h .. 8 h + 7
  const int w_fr = 2 * kPlane + (wc * 64 + r) * kRowB + 16 * h;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  float4 x0, x1, w0, w1;
  auto load_raw = [&](int k0) {
    x0 = *reinterpret_cast<const float4*>(Xg0 + k0);
    x1 = *reinterpret_cast<const float4*>(Xg1 + k0);
    w0 = *reinterpret_cast<const float4*>(Wg0 + k0);
    w1 = *reinterpret_cast<const float4*>(Wg1 + k0);
  };
  auto split_store = [&](int stage) {
    unsigned char* const s = lds + stage * kStage;
    stage4<false>(x0, 1.0f, s + st, s + kPlane + st);
    stage4<false>(x1, 1.0f, s + st + 64 * kRowB, s + kPlane + st + 64 * kRowB);
    stage4<true>(w0, sw, s + 2 * kPlane + st, s + 3 * kPlane + st);
    stage4<true>(w1, sw, s + 2 * kPlane + st + 64 * kRowB, s + 3 * kPlane + st + 64 * kRowB);
  };

  const int nk = K / kHK;
  load_raw(0);
  split_store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_raw((kt + 1) * kHK);                              // in flight under this step's MFMAs
    half8 fa[2][2], fb[2][2];                                        // [plane][tile]
    const unsigned char* const s = lds + cur * kStage;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[p][i] = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(s + p * kPlane + x_fr + i * 32 * kRowB));
        fb[p][i] = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(s + p * kPlane + w_fr + i * 32 * kRowB));
      }
    // a b = a1 b2 + a2 b1 + a1 b1 (small terms first, as gemm_x3.hip); a2 b2 ~ 2^-22 |a b| is dropped
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[1][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][i], fb[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
    if (more) split_store(cur ^ 1);                                  // last read in step kt - 1, before the barrier that ended it
    __syncthreads();
  }

  // ---- epilogue: two 64-row halves through LDS (C/D map: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)); 32 lanes hold
  // one row's 128 columns as float4 and reduce it to the tile's (max, lowest column holding it, sum of exp(x - max))
  float* const Cs = reinterpret_cast<float*>(lds);
  const float inv = 1.0f / sw;                                       // a power of two: exact
  const int c4 = tid & 31, rsub = tid >> 5;
  const int gcol = n0 + 4 * c4;
  float bv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bv[q] = gcol + q < V ? bias[gcol + q] : 0.f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (wr == half) {
      float* cw = Cs + (4 * h) * kCs + wc * 64 + r;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) cw[(i * 32 + (e & 3) + 8 * (e >> 2)) * kCs + j * 32] = acc[i][j][e];
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
      const int row = pass * 8 + rsub;
      const int grow = m0 + half * 64 + row;
      const float4 c = *reinterpret_cast<const float4*>(Cs + row * kCs + 4 * c4);
      float v[4] = {c.x * inv + bv[0], c.y * inv + bv[1], c.z * inv + bv[2], c.w * inv + bv[3]};
      float best = -INFINITY;
      int bidx = 0x7fffffff;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (gcol + q >= V) v[q] = -INFINITY;                         // a pad column never wins and adds exp(-inf) = 0
        if (v[q] > best) { best = v[q]; bidx = gcol + q; }           // strict '>' in column order: the first maximum
      }
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {                      // stays inside the 32 lanes of the row
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bidx, off);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
      }
      float e = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) e += v[q] == -INFINITY ? 0.f : expf(v[q] - best);
      e = half_wave_sum(e);
      if (c4 == 0 && grow < M) {
        const size_t o = (size_t)tn * M + grow;
        pmax[o] = best; pidx[o] = bidx; psum[o] = e;
      }
      if constexpr (TOPK) {
        // k rounds of the same (max, lowest column) pass: each round stores the winner and strikes it from the lane that holds it
        for (int rank = 0; rank < k; ++rank) {                        // k is uniform: every lane reaches the shuffles
          if (c4 == 0 && grow < M) {
            const size_t o = ((size_t)tn * k + rank) * M + grow;
            pkv[o] = best; pki[o] = bidx;
          }
          if (rank + 1 == k) break;
          const int struck = bidx;
          best = -INFINITY;
          bidx = 0x7fffffff;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (gcol + q == struck) v[q] = -INFINITY;
            if (v[q] > best) { best = v[q]; bidx = gcol + q; }
          }
#pragma unroll
          for (int off = 16; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bidx, off);
            if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256, 3) void ctc_head_tile_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                                               const float* __restrict__ bias, float sw, int M, int V, int K, int tiles_n,
                                                               int n_tiles, int gw, float* __restrict__ pmax, int* __restrict__ pidx,
                                                               float* __restrict__ psum) {
  ctc_head_tile<false>(X, ldx, W, ldw, bias, sw, M, V, K, tiles_n, n_tiles, gw, pmax, pidx, psum, 0, nullptr, nullptr);
}

__global__ __launch_bounds__(256, 3) void ctc_head_tile_topk_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                                                    const float* __restrict__ bias, float sw, int M, int V, int K,
                                                                    int tiles_n, int n_tiles, int gw, float* __restrict__ pmax,
                                                                    int* __restrict__ pidx, float* __restrict__ psum, int k,
                                                                    float* __restrict__ pkv, int* __restrict__ pki) {
  ctc_head_tile<true>(X, ldx, W, ldw, bias, sw, M, V, K, tiles_n, n_tiles, gw, pmax, pidx, psum, k, pkv, pki);
}

// a row's column tiles in ascending order with the running triple: a later tile replaces the maximum
// only when strictly larger (so among equal maxima the lowest column wins) and the sum is rescaled to the maximum it then has
__device__ __forceinline__ void merge_row_triples(const float* __restrict__ pmax, const int* __restrict__ pidx, const float* __restrict__ psum,
                                                  int M, int tiles_n, int row, int32_t* __restrict__ ids, float* __restrict__ logp_best,
                                                  float* __restrict__ lse, int* range_flag, float* m_out, float* ls_out) {
  float m = -INFINITY, s = 0.f;
  int idx = 0x7fffffff;
  for (int t = 0; t < tiles_n; ++t) {
    const size_t o = (size_t)t * M + row;
    const float mt = pmax[o], st = psum[o];
    if (mt > m) {
      s = s * expf(m - mt) + st;                                     // m = -inf: 0 * 0 + st
      m = mt; idx = pidx[o];
    } else if (mt != -INFINITY) {
      s += st * expf(mt - m);
    }
  }
  const float ls = logf(s);
  ids[row] = idx;
  logp_best[row] = -ls;                                              // best logit - (m + log s)
  if (lse) lse[row] = m + ls;
  if (range_flag && !(fabsf(m + ls) < INFINITY)) atomicOr(range_flag, 1);      // NaN / Inf reached the logits (as logsoftmax_argmax_kernel)
  *m_out = m; *ls_out = ls;
}

// one thread per row
__global__ __launch_bounds__(256) void ctc_head_merge_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                                             const float* __restrict__ psum, int M, int tiles_n, int32_t* __restrict__ ids,
                                                             float* __restrict__ logp_best, float* __restrict__ lse, int* range_flag) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  float m, ls;
  merge_row_triples(pmax, pidx, psum, M, tiles_n, row, ids, logp_best, lse, range_flag, &m, &ls);
}

// The merge of the top-k head: the greedy outputs by the same walk, then the k best of the row's tiles x k pairs.  The running list
// is 16 (value, column) pairs in registers of which the first k are used, kept sorted by an unrolled bubble insert (static indices
// only: no scratch).  A tile's pairs are sorted, so the tile is left at its first pair that does not beat slot k - 1.
__global__ __launch_bounds__(256) void ctc_head_merge_topk_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx,
                                                                  const float* __restrict__ psum, const float* __restrict__ pkv,
                                                                  const int* __restrict__ pki, int M, int tiles_n, int k,
                                                                  int32_t* __restrict__ ids, float* __restrict__ logp_best,
                                                                  float* __restrict__ lse, int32_t* __restrict__ topk_ids,
                                                                  float* __restrict__ topk_logp, int* range_flag) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  float m, ls;
  merge_row_triples(pmax, pidx, psum, M, tiles_n, row, ids, logp_best, lse, range_flag, &m, &ls);
  float val[kCtcTopkMax];
  int col[kCtcTopkMax];
#pragma unroll
  for (int j = 0; j < kCtcTopkMax; ++j) { val[j] = -INFINITY; col[j] = 0x7fffffff; }
  for (int t = 0; t < tiles_n; ++t)
    for (int rank = 0; rank < k; ++rank) {
      const size_t o = ((size_t)t * k + rank) * M + row;
      float cv = pkv[o];
      int ci = pki[o];
      float lv = val[0];                                             // the list's slot k - 1, picked with static indices
      int lc = col[0];
#pragma unroll
      for (int j = 1; j < kCtcTopkMax; ++j)
        if (j == k - 1) { lv = val[j]; lc = col[j]; }
      if (!(cv > lv || (cv == lv && ci < lc))) break;                // it cannot be among the k best: nor can the tile's later pairs
#pragma unroll
      for (int j = 0; j < kCtcTopkMax; ++j) {
        if (j >= k) break;                                           // slots from k on are never returned
        const bool in = cv > val[j] || (cv == val[j] && ci < col[j]);
        const float tv = in ? val[j] : cv;
        const int ti = in ? col[j] : ci;
        val[j] = in ? cv : val[j];
        col[j] = in ? ci : col[j];
        cv = tv; ci = ti;
      }
    }
#pragma unroll
  for (int j = 0; j < kCtcTopkMax; ++j)
    if (j < k) {
      const bool none = col[j] == 0x7fffffff;                        // fewer than k finite logits in the row
      topk_ids[(size_t)row * k + j] = none ? -1 : col[j];
      // (value - maximum) - log(sum) never increases along the row; rank 0 is logp_best's own -ls (0 - ls would lose the sign of -0)
      topk_logp[(size_t)row * k + j] = none ? -INFINITY : (j == 0 ? -ls : (val[j] - m) - ls);
    }
}

// ---- CTC collapse ---------------------------------------------------------------------------------------------------------------
// CTCSearch's loop (sensevoice-small.cpp:340-347) per utterance: keep frame t when id[t] != blank and id[t] != id[t - 1]
// (id[-1] = -1), compacted by a prefix sum.  One workgroup per utterance scans kCollapseChunk frames a trip; what crosses a chunk
// is the running count (every thread holds the same copy) and the previous chunk's last id (read back from the frame ids).
constexpr int kCollapseChunk = 256;

__global__ __launch_bounds__(kCollapseChunk) void ctc_collapse_kernel(const int32_t* __restrict__ frame_ids, const float* __restrict__ frame_logp,
                                                                      const int* __restrict__ row_off, const int* __restrict__ len, int blank,
                                                                      int max_tokens, int32_t* __restrict__ ids, int32_t* __restrict__ tok_frame,
                                                                      float* __restrict__ tok_logp, int32_t* __restrict__ token_num) {
  __shared__ int s_wave[kCollapseChunk / 64];
  const int b = blockIdx.x;
  const int T = len[b];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* fid = frame_ids + row_off[b];
  const float* flp = frame_logp ? frame_logp + row_off[b] : nullptr;
  const size_t out0 = (size_t)b * max_tokens;
  int count = 0;
  for (int c0 = 0; c0 < T; c0 += kCollapseChunk) {                   // T and c0 are uniform: every thread reaches the barriers
    const int t = c0 + tid;
    int id = blank, prev = -1;
    if (t < T) {
      id = fid[t];
      if (t > 0) prev = fid[t - 1];
    }
    const bool keep = t < T && id != blank && id != prev;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kCollapseChunk / 64; ++w) {
      const int n = s_wave[w];
      if (w < wave) before += n;
      total += n;
    }
    const int pos = count + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos < max_tokens) {
      ids[out0 + pos] = id;
      if (tok_frame) tok_frame[out0 + pos] = t;
      if (tok_logp) tok_logp[out0 + pos] = flp[t];
    }
    count += total;
    __syncthreads();                                                 // s_wave is rewritten by the next chunk
  }
  if (tid == 0) token_num[b] = count;                                // the true count, also when it exceeds max_tokens
}

// SenseVoice's prompt rows (sensevoice-small.cpp:597-640): rows row_off[b] .. + 3 of feats = rows prompt[4 b ..] of E [16][D]
__global__ __launch_bounds__(128) void svs_prompt_rows_kernel(const float* __restrict__ E, int D, const int* __restrict__ prompt,
                                                              const int* __restrict__ row_off, const int* __restrict__ len,
                                                              float* __restrict__ feats, int ld) {
  const int b = blockIdx.x >> 2, j = blockIdx.x & 3;
  if (len[b] < 4) return;
  const float* src = E + (size_t)prompt[4 * b + j] * D;
  float* dst = feats + (size_t)(row_off[b] + j) * ld;
  for (int c = threadIdx.x; c < D; c += 128) dst[c] = src[c];
}

// best[r] = logp[r][ids[r]]: the unfused head's log-prob of the arg-max
__global__ __launch_bounds__(256) void gather_best_kernel(const float* __restrict__ logp, int ld, const int32_t* __restrict__ ids, int M,
                                                          float* __restrict__ best) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < M) best[r] = logp[(size_t)r * ld + ids[r]];
}

// lse[r] = log sum_c exp(logits[r][c]) of the unfused head's logits, one wave per row (max first, then the sum): what the fused head's
// merge kernel writes as `lse`, kept for the aligner (ctc_align.hip).  A second pass over the chunk's logits, on the unfused route only.
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ logits, int ld, int M, int V, float* __restrict__ lse) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* x = logits + (size_t)row * ld;
  float m = -INFINITY;
  for (int c = lane; c < V; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  float sum = 0.f;
  for (int c = lane; c < V; c += 64) sum += x[c] == -INFINITY ? 0.f : expf(x[c] - m);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) lse[row] = m + logf(sum);
}

// The k best columns of a row of the unfused head's log-probs, one wave per row: round r takes the largest value that ranks behind
// round r - 1's pick (smaller, or equal with a higher column), lowest column first — k passes over a row that sits in L2.
__global__ __launch_bounds__(256) void row_topk_kernel(const float* __restrict__ logp, int ld, int rows, int V, int k,
                                                       int32_t* __restrict__ topk_ids, float* __restrict__ topk_logp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                                           // whole waves leave: the shuffles below stay inside a wave
  const float* x = logp + (size_t)row * ld;
  float pv = INFINITY;
  int pc = -1;
  for (int r = 0; r < k; ++r) {
    float best = -INFINITY;
    int bc = 0x7fffffff;
    for (int c = lane; c < V; c += 64) {
      const float v = x[c];
      const bool behind = v < pv || (v == pv && c > pc);
      if (behind && (v > best || (v == best && c < bc))) { best = v; bc = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oc = __shfl_xor(bc, off);
      if (ob > best || (ob == best && oc < bc)) { best = ob; bc = oc; }
    }
    if (lane == 0) {
      topk_ids[(size_t)row * k + r] = bc == 0x7fffffff ? -1 : bc;
      topk_logp[(size_t)row * k + r] = bc == 0x7fffffff ? -INFINITY : best;
    }
    pv = best; pc = bc;
  }
}

}  // namespace

bool launch_row_topk(const float* logp, int ld, int rows, int V, int k, int32_t* topk_ids, float* topk_logp, hipStream_t s) {
  if (k < 1 || k > kCtcTopkMax || V < k || ld < V || rows < 0) return false;
  if (rows == 0) return true;
  if (!logp || !topk_ids || !topk_logp) return false;
  hipLaunchKernelGGL(row_topk_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logp, ld, rows, V, k, topk_ids, topk_logp);
  return true;
}

void launch_svs_prompt_rows(const float* E, int D, const int* prompt, const int* row_off, const int* len, int B, float* feats, int ld,
                            hipStream_t s) {
  if (B > 0) hipLaunchKernelGGL(svs_prompt_rows_kernel, dim3(4 * B), dim3(128), 0, s, E, D, prompt, row_off, len, feats, ld);
}
void launch_gather_best(const float* logp, int ld, const int32_t* ids, int M, float* best, hipStream_t s) {
  if (M > 0) hipLaunchKernelGGL(gather_best_kernel, dim3((M + 255) / 256), dim3(256), 0, s, logp, ld, ids, M, best);
}

void launch_row_lse(const float* logits, int ld, int M, int V, float* lse, hipStream_t s) {
  if (M > 0) hipLaunchKernelGGL(row_lse_kernel, dim3((M + 3) / 4), dim3(256), 0, s, logits, ld, M, V, lse);
}

size_t ctc_head_workspace_bytes(int M, int V) {
  const size_t tiles_n = (size_t)(V + kHT - 1) / kHT;
  return 3 * tiles_n * (size_t)M * 4;
}

bool launch_ctc_head(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int32_t* ids,
                     float* logp_best, float* lse, void* workspace, size_t workspace_bytes, hipStream_t s, int* range_flag) {
  if (M < 0 || V <= 0 || K < 32 || K % 32 || !W || !bias || ldw < K || ldw % 4 || !(w_scale > 0.f)) return false;
  if (M == 0) return true;
  if (!X || ldx < K || ldx % 4 || !ids || !logp_best || !workspace || workspace_bytes < ctc_head_workspace_bytes(M, V)) return false;
  const int tiles_m = (M + kHT - 1) / kHT, tiles_n = (V + kHT - 1) / kHT;
  if ((long long)tiles_m * tiles_n > 0x7fffffffLL) return false;
  const int n_tiles = tiles_m * tiles_n;
  // column groups of <= 2 MiB of weights stay in an XCD's L2 while the row panels stream through (split_common.h tile_of_block)
  const int gw = std::max(1, std::min(tiles_n, (int)(2.0 * 1024 * 1024 / ((double)kHT * K * 4))));
  float* pmax = static_cast<float*>(workspace);
  int* pidx = reinterpret_cast<int*>(pmax + (size_t)tiles_n * M);
  float* psum = pmax + 2 * (size_t)tiles_n * M;
  hipLaunchKernelGGL(ctc_head_tile_kernel, dim3(n_tiles), dim3(256), 0, s, X, ldx, W, ldw, bias, w_scale, M, V, K, tiles_n, n_tiles, gw, pmax,
                     pidx, psum);
  hipLaunchKernelGGL(ctc_head_merge_kernel, dim3((M + 255) / 256), dim3(256), 0, s, pmax, pidx, psum, M, tiles_n, ids, logp_best, lse, range_flag);
  return true;
}

size_t ctc_head_topk_workspace_bytes(int M, int V, int k) {
  const size_t tiles_n = (size_t)(V + kHT - 1) / kHT;
  return ctc_head_workspace_bytes(M, V) + 2 * tiles_n * (size_t)k * (size_t)M * 4;
}

bool launch_ctc_head_topk(const float* X, int ldx, const float* W, int ldw, const float* bias, float w_scale, int M, int V, int K, int k,
                          int32_t* ids, float* logp_best, float* lse, int32_t* topk_ids, float* topk_logp, void* workspace,
                          size_t workspace_bytes, hipStream_t s, int* range_flag) {
  if (k < 1 || k > kCtcTopkMax || V < k) return false;
  if (M < 0 || V <= 0 || K < 32 || K % 32 || !W || !bias || ldw < K || ldw % 4 || !(w_scale > 0.f)) return false;
  if (M == 0) return true;
  if (!X || ldx < K || ldx % 4 || !ids || !logp_best || !topk_ids || !topk_logp || !workspace ||
      workspace_bytes < ctc_head_topk_workspace_bytes(M, V, k))
    return false;
  const int tiles_m = (M + kHT - 1) / kHT, tiles_n = (V + kHT - 1) / kHT;
  if ((long long)tiles_m * tiles_n > 0x7fffffffLL) return false;
  const int n_tiles = tiles_m * tiles_n;
  const int gw = std::max(1, std::min(tiles_n, (int)(2.0 * 1024 * 1024 / ((double)kHT * K * 4))));      // as launch_ctc_head
  float* pmax = static_cast<float*>(workspace);
  int* pidx = reinterpret_cast<int*>(pmax + (size_t)tiles_n * M);
  float* psum = pmax + 2 * (size_t)tiles_n * M;
  float* pkv = pmax + 3 * (size_t)tiles_n * M;
  int* pki = reinterpret_cast<int*>(pkv + (size_t)tiles_n * k * M);
  hipLaunchKernelGGL(ctc_head_tile_topk_kernel, dim3(n_tiles), dim3(256), 0, s, X, ldx, W, ldw, bias, w_scale, M, V, K, tiles_n, n_tiles, gw,
                     pmax, pidx, psum, k, pkv, pki);
  hipLaunchKernelGGL(ctc_head_merge_topk_kernel, dim3((M + 255) / 256), dim3(256), 0, s, pmax, pidx, psum, pkv, pki, M, tiles_n, k, ids,
                     logp_best, lse, topk_ids, topk_logp, range_flag);
  return true;
}

int ctc_collapse_chunk() { return kCollapseChunk; }

bool launch_ctc_collapse(const int32_t* frame_ids, const float* frame_logp, const int* row_off, const int* len, int B, int blank,
                         int max_tokens, int32_t* ids, int32_t* tok_frame, float* tok_logp, int32_t* token_num, hipStream_t s) {
  if (B < 0 || max_tokens < 0 || !row_off || !len || !token_num || (max_tokens > 0 && !ids) || (tok_logp && !frame_logp)) return false;
  if (B == 0) return true;
  if (!frame_ids) return false;
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(kCollapseChunk), 0, s, frame_ids, frame_logp, row_off, len, blank, max_tokens, ids,
                     tok_frame, tok_logp, token_num);
  return true;
}

}  // namespace pfhip
