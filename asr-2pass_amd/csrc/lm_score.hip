// Sentences scored by the token n-gram language model (pfhip_op_lm_score, include/pfhip_ops.h): the rescoring and perplexity
// primitive beside the searches that walk the same model, and lm_step.h on its own.
//
// One lane per sentence: a sentence is a chain of dependent steps (the state behind token i is the state before token i + 1), so there
// is nothing to share inside one, and sentences share nothing with each other.  A step is a binary search over a state's arcs: a few
// dependent loads the L2 answers.  No LDS, no barrier, no atomics; every store goes to the lane's own row of the outputs.
#include "kernels.h"
#include "launch_common.h"
#include "lm_step.h"

namespace pfhip {
namespace {

constexpr int kNT = 64;

__global__ __launch_bounds__(kNT) void lm_score_kernel(const int32_t* __restrict__ ids, const int* __restrict__ len, int B, int max_len,
                                                       LmGraphDev g, float* __restrict__ tok_w, float* __restrict__ eos_w,
                                                       float* __restrict__ total) {
  const int b = blockIdx.x * kNT + threadIdx.x;
  if (b >= B) return;
  const int n = min(max(len[b], 0), max_len);
  const int32_t* const row = ids + (size_t)b * max_len;
  float* const out = tok_w + (size_t)b * max_len;
  int state = g.start;
  float sum = 0.f;
  for (int i = 0; i < n; ++i) {
    float w;
    state = lm_step(g, state, min(max(row[i], 0), g.vocab - 1), &w);
    out[i] = w;
    sum = sum + w;
  }
  for (int i = n; i < max_len; ++i) out[i] = 0.f;
  float e = 0.f;
  if (g.has_eos) {
    lm_step(g, state, g.vocab, &e);
    sum = sum + e;
  }
  eos_w[b] = e;
  total[b] = sum;
}

}  // namespace

bool launch_lm_score(const int32_t* ids, const int* len, int B, int max_len, const LmGraphDev& g, float* tok_w, float* eos_w, float* total,
                     hipStream_t s) {
  if (B < 0 || max_len < 0 || g.n_states < 1 || g.n_arcs < 0 || g.vocab < 1 || g.start < 0 || g.start >= g.n_states ||
      (long long)B * max_len > 0x7fffffffLL)
    return false;
  if (B == 0) return true;
  if (!len || !eos_w || !total || (max_len > 0 && (!ids || !tok_w)) || !g.uni_w || !g.uni_next || !g.arc_begin || !g.backoff_w || !g.backoff_state ||
      (g.n_arcs > 0 && (!g.arc_label || !g.arc_next || !g.arc_weight)))
    return false;
  hipLaunchKernelGGL(lm_score_kernel, dim3((B + kNT - 1) / kNT), dim3(kNT), 0, s, ids, len, B, max_len, g, tok_w, eos_w, total);
  return true;
}

}  // namespace pfhip
