// Head with N-best candidates: the sibling of logsoftmax_argmax_kernel (rowops.hip) that, per token row, also selects the k best
// columns (1 <= k <= 8) and their log-probabilities.  The reference's GreedySearch keeps only the arg-max
// (onnxruntime/src/paraformer.cpp:386-395); this is an extension for callers that want token confidences and runners-up without the
// [rows, vocab] log-probability matrix.  Launched only when candidates are asked for: k = 0 keeps the rowops.hip kernel and its launch.
//
// Order: larger logit first, equal logits smaller column first (FindMax, util.cpp:63-74, and the arg-max kernel's reductions), so
// candidate 0 is the arg-max id and any prefix of the list is the answer for a smaller k.
// Values: (logit - m) - lse with m and lse formed by the arg-max kernel's own statements in its order (thread-strided expf sum,
// wave_sum, (s0 + s1) + (s2 + s3)), so a candidate's value equals the logp entry of its column bit for bit.
#include "kernels.h"

#include <math.h>

namespace pfhip {
namespace {

__device__ __forceinline__ float wave_sum(float v) {      // rowops.hip's: the sum order is part of the bit-for-bit statement above
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

constexpr int kNoCol = 0x7fffffff;      // the arg-max kernel's "no column yet"

// Every thread keeps the K best (logit, column) pairs of the columns it reads, sorted, in registers: the insertion is an unrolled
// compare-and-swap chain over named elements (an array indexed at run time would live in scratch).  A thread visits its columns in
// increasing order, so an equal logit arrives with the larger column and strict '>' keeps the earlier one ahead.
template <int K>
struct TopList {
  float v[K];
  int c[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = -INFINITY; c[j] = kNoCol; }
  }
  __device__ __forceinline__ void insert(float x, int col) {
    if (x > v[K - 1]) {
      v[K - 1] = x; c[K - 1] = col;
#pragma unroll
      for (int j = K - 1; j >= 1; --j) {
        const bool up = v[j] > v[j - 1];
        const float hv = up ? v[j] : v[j - 1], lv = up ? v[j - 1] : v[j];
        const int hc = up ? c[j] : c[j - 1], lc = up ? c[j - 1] : c[j];
        v[j - 1] = hv; v[j] = lv; c[j - 1] = hc; c[j] = lc;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) { v[j] = v[j + 1]; c[j] = c[j + 1]; }
    v[K - 1] = -INFINITY; c[K - 1] = kNoCol;
  }
};

template <int K>
__global__ __launch_bounds__(256) void logsoftmax_topk_kernel(const float* __restrict__ logits, int ldl, int ML, int V, int k,
                                                              float* __restrict__ logp, int32_t* __restrict__ ids,
                                                              int32_t* __restrict__ topk_ids, float* __restrict__ topk_logp,
                                                              int* range_flag) {
  __shared__ float s_max[2][4];
  __shared__ int s_idx[2][4];
  __shared__ float s_sum[4];
  const int row = blockIdx.x;
  if (row >= ML) return;
  const float* lr = logits + (size_t)row * ldl;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  TopList<K> top;
  top.clear();
  int bad = 0;                                  // a NaN never wins a comparison: non-finite logits are looked for element by element
  if ((V & 3) == 0 && (ldl & 3) == 0) {         // 16-byte loads (every vocabulary of the model: 8404 = 4 x 2101 columns, padded rows)
    for (int c4 = threadIdx.x; 4 * c4 < V; c4 += 256) {
      const float4 x = *reinterpret_cast<const float4*>(lr + 4 * c4);
      const int c = 4 * c4;
      top.insert(x.x, c);
      top.insert(x.y, c + 1);
      top.insert(x.z, c + 2);
      top.insert(x.w, c + 3);
      bad |= (int)!(fabsf(x.x) < INFINITY) | (int)!(fabsf(x.y) < INFINITY) | (int)!(fabsf(x.z) < INFINITY) | (int)!(fabsf(x.w) < INFINITY);
    }
  } else {
    for (int c = threadIdx.x; c < V; c += 256) {
      const float x = lr[c];
      top.insert(x, c);
      bad |= (int)!(fabsf(x) < INFINITY);
    }
  }
  // k rounds of a block-wide arg-max over the threads' list heads (ties -> smaller column, as in the arg-max kernel); the thread that
  // holds the winner pops it.  Every thread ends a round with the same winner, so thread 0 has all k in registers.  The LDS slots
  // alternate between rounds: a wave can be at most one barrier ahead of the slowest reader.
  float win_v[K];
  int win_c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    win_v[j] = -INFINITY; win_c[j] = kNoCol;
    if (j < k) {                                // uniform
      float best = top.v[0];
      int bidx = top.c[0];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bidx, off);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
      }
      if (lane == 0) { s_max[j & 1][wave] = best; s_idx[j & 1][wave] = bidx; }
      __syncthreads();
      float m = s_max[j & 1][0];
      int mi = s_idx[j & 1][0];
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (s_max[j & 1][i] > m || (s_max[j & 1][i] == m && s_idx[j & 1][i] < mi)) { m = s_max[j & 1][i]; mi = s_idx[j & 1][i]; }
      win_v[j] = m; win_c[j] = mi;
      if (top.c[0] == mi) top.pop();
    }
  }
  const float m = win_v[0];
  const int mi = win_c[0];
  // the log-sum-exp pass runs with logp null as well: the candidates' values are the point of this kernel
  float sum = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) sum += expf(lr[c] - m);
  sum = wave_sum(sum);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  const float lse = logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
  // the range flag is raised where the arg-max kernel raises it: without logp by a non-finite logit, in both forms by a non-finite lse
  if (range_flag && !logp && __any(bad)) { if (lane == 0) atomicOr(range_flag, 1); }
  if (threadIdx.x == 0) {
    ids[row] = mi;
    if (range_flag && !(fabsf(lse) < INFINITY)) atomicOr(range_flag, 1);      // NaN / Inf reached the logits
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < k) {
        topk_ids[(size_t)row * k + j] = win_c[j];
        topk_logp[(size_t)row * k + j] = (win_v[j] - m) - lse;
      }
  }
  if (logp) {
    float* pr = logp + (size_t)row * V;
    for (int c = threadIdx.x; c < V; c += 256) pr[c] = (lr[c] - m) - lse;
  }
}

}  // namespace

bool launch_logsoftmax_topk(const float* logits, int ldl, int ML, int V, int k, float* logp, int32_t* ids, int32_t* topk_ids,
                            float* topk_logp, hipStream_t s, int* range_flag) {
  if (k < 1 || k > kTopkMax || V < k || ML < 0 || ldl < V || !logits || !ids || !topk_ids || !topk_logp) return false;
  if (ML == 0) return true;
  const dim3 grid(ML), block(256);
  if (k == 1)
    hipLaunchKernelGGL(logsoftmax_topk_kernel<1>, grid, block, 0, s, logits, ldl, ML, V, k, logp, ids, topk_ids, topk_logp, range_flag);
  else if (k == 2)
    hipLaunchKernelGGL(logsoftmax_topk_kernel<2>, grid, block, 0, s, logits, ldl, ML, V, k, logp, ids, topk_ids, topk_logp, range_flag);
  else if (k <= 4)
    hipLaunchKernelGGL(logsoftmax_topk_kernel<4>, grid, block, 0, s, logits, ldl, ML, V, k, logp, ids, topk_ids, topk_logp, range_flag);
  else
    hipLaunchKernelGGL(logsoftmax_topk_kernel<8>, grid, block, 0, s, logits, ldl, ML, V, k, logp, ids, topk_ids, topk_logp, range_flag);
  return true;
}

}  // namespace pfhip
