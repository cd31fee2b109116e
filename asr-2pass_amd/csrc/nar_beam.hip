// Hotword-biased beam search over the candidates of a non-autoregressive head: the rows of a Paraformer are independent token
// positions, each with its k best columns as topk.hip leaves them, so a hypothesis is one candidate per row and the search replaces
// tokens position by position without ever changing the token count.  include/pfhip_ops.h (pfhip_op_nbest_ctx_beam) states the
// recurrence and the tie rule.  An extension: the reference biases a Paraformer only inside its WFST search (BiasLm).
//
// One workgroup of 128 threads per utterance walks its len[b] rows in order, built like ctc_prefix_beam_kernel<true> (ctc_beam.hip).
// The beam (<= 16 hypotheses: am score, context score and state, trie node) is a double buffer in LDS: row t reads buffer t & 1 and
// writes the other.  A row is two phases and two barriers.
//   A  thread p < nh * width forms the extension of hypothesis p / width by candidate p % width into candidate slot p: slots are
//      hypothesis-major and candidate-minor.  Two extensions differ in the parent or in the token, so they never name the same
//      sequence: there is no merge.
//   B  every candidate counts the candidates that beat it (greater total; equal total and lower slot): its rank.  Ranks are unique,
//      so ranks 0 .. beam - 1 write the next beam without a race.  A surviving extension at rank r of row t owns trie node
//      1 + t * beam_stride + r of the utterance: no allocation counter, no atomics.  Threads < width fetch the next row meanwhile.
// Trip counts depend on len[b] and the utterance's descriptor alone, all uniform in the workgroup; barriers sit in uniform control
// flow only; no spin-wait, no dependency between workgroups, no atomics.  Ids of a row are clamped to 0 .. V - 1, a log-probability
// that is NaN or below -FLT_MAX counts as -FLT_MAX, a NaN total ranks as -inf: whatever the rows hold, ranks stay unique, every beam
// slot that is read was written, and every index stays inside its buffer.  Graph indices are the host builder's (ctx_graph.cpp).
// The final walk from each surviving node to the root writes the ids; it reads nodes other threads wrote, behind a barrier.
//
// kLm = true is the same search with a token n-gram language model (lm_step.h) walked beside the context graph: a hypothesis also
// carries the model's state and its score so far, an extension adds the weight of its token to it, the total takes it as one more
// fp32 add behind am + ctx, and at the end, where the model has </s>, every live hypothesis takes the weight of </s> (after the context
// back-off, before the final order).  The model's state and score are a function of the token sequence alone.  kLm = false compiles to
// what the kernel was before: the model's LDS arrays exist in the kLm = true instantiation alone, the extra arguments are not read.
#include "ctx_step.h"
#include "kernels.h"
#include "launch_common.h"
#include "lm_step.h"

#include <float.h>
#include <math.h>

#include <algorithm>

namespace pfhip {
namespace {

constexpr int kNT = 128;                         // threads of the workgroup
constexpr int kBM = kBeamMax;                    // 16 hypotheses
constexpr int kWM = kNarWidthMax;                // 8 candidates of a row
static_assert(kBM * kWM <= kNT, "one thread per (hypothesis, candidate) pair");

struct NarBeam {                                 // one buffer of the beam
  float am[kBM], ctx[kBM];
  int state[kBM], node[kBM];
};
struct BeamLm {                                  // the model's share of one buffer of the beam (kLm)
  float lm[kBM];
  int lm_state[kBM];
};
// The LDS of the model's state and score exists in the kLm = true instantiation alone: the arrays are function-local statics of the
// specialisation that is only called there, so kLm = false keeps the LDS layout, and with it the code, it had before.
template <bool kLm> struct LmLds;
template <> struct LmLds<false> {
  __device__ static __forceinline__ BeamLm* beam() { return nullptr; }
  __device__ static __forceinline__ float* cand_lm() { return nullptr; }
  __device__ static __forceinline__ int* cand_state() { return nullptr; }
};
template <> struct LmLds<true> {
  __device__ static __forceinline__ BeamLm* beam() { __shared__ BeamLm b[2]; return b; }
  __device__ static __forceinline__ float* cand_lm() { __shared__ float a[kNT]; return a; }
  __device__ static __forceinline__ int* cand_state() { __shared__ int a[kNT]; return a; }
};

template <bool kLm>
__global__ __launch_bounds__(kNT) void nbest_ctx_beam_kernel(const int32_t* __restrict__ cand_ids, const float* __restrict__ cand_logp, int k,
                                                             long long rows, const int* __restrict__ row_off, const int* __restrict__ len,
                                                             const int* __restrict__ len_cap, int V, int beam_stride, int nbest_stride, int max_tokens,
                                                             int32_t* __restrict__ n_hyp, int32_t* __restrict__ out_ids,
                                                             int32_t* __restrict__ n_tokens, float* __restrict__ score,
                                                             float* __restrict__ am_score, float* __restrict__ ctx_score,
                                                             int32_t* __restrict__ node_parent, int32_t* __restrict__ node_token,
                                                             const BeamUtt* __restrict__ utt, const CtxGraphDev* __restrict__ graphs,
                                                             int n_graphs, LmGraphDev lm, float* __restrict__ lm_score) {
  __shared__ NarBeam beam[2];
  __shared__ int fr_id[2][kWM];
  __shared__ float fr_lp[2][kWM];
  __shared__ float c_tot[kNT], c_am[kNT], c_ctx[kNT];
  __shared__ int c_state[kNT];
  BeamLm* const blm = LmLds<kLm>::beam();                            // null without a model, and then never read
  float* const c_lm = LmLds<kLm>::cand_lm();
  int* const c_lm_state = LmLds<kLm>::cand_state();

  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = len_cap ? min(len[b], len_cap[b]) : len[b];          // (the model's token rows: fires capped by the token count)
  const long long r0 = row_off[b];
  // what this utterance may write: [b][nbest_stride]...; emptied first, so that a refused or rowless utterance reads as "no hypothesis"
  const size_t o_h = (size_t)b * nbest_stride;
  for (int j = tid; j < nbest_stride; j += kNT) {
    n_tokens[o_h + j] = 0;
    score[o_h + j] = -INFINITY; am_score[o_h + j] = -INFINITY; ctx_score[o_h + j] = 0.f;
    if constexpr (kLm) lm_score[o_h + j] = 0.f;
  }
  for (size_t j = tid; j < (size_t)nbest_stride * max_tokens; j += kNT) out_ids[o_h * max_tokens + j] = -1;
  // the rows must lie inside the arrays (row_off and len are device data the launcher could not see), and the descriptor inside the
  // launch's strides; T * beam_stride + 1 stays below 2^31 (the launcher's check on rows).  first_beam is the width here.
  const BeamUtt u = utt[b];
  const bool refused = T < 0 || r0 < 0 || r0 + T > rows || u.first_beam < 1 || u.first_beam > min(k, kWM) || u.second_beam < 1 ||
                       u.second_beam > min(beam_stride, kBM) || u.nbest < 1 || u.nbest > min(u.second_beam, nbest_stride) || u.graph < -1 ||
                       u.graph >= n_graphs;
  if (refused || T == 0) {                                           // uniform
    if (tid == 0) n_hyp[b] = 0;
    return;
  }
  const int width = u.first_beam, bw = u.second_beam, nbest = u.nbest;
  CtxGraphDev g;
  if (u.graph >= 0) g = graphs[u.graph];
  // utterance b's nodes 1 .. T * beam_stride are stored from r0 * beam_stride on: node n at n - 1 (the root, node 0, is never read)
  int32_t* const npar = node_parent + (size_t)r0 * beam_stride;
  int32_t* const ntok = node_token + (size_t)r0 * beam_stride;
  const int32_t* const rid = cand_ids + (size_t)r0 * k;
  const float* const rlp = cand_logp + (size_t)r0 * k;

  auto fetch = [&](int t) {                                          // threads < width: row t's candidates, sanitised
    if (tid < width) {
      const int id = rid[(size_t)t * k + tid];
      float lp = rlp[(size_t)t * k + tid];
      if (!(lp >= -FLT_MAX)) lp = -FLT_MAX;                          // NaN, -inf
      fr_id[t & 1][tid] = min(max(id, 0), V - 1);
      fr_lp[t & 1][tid] = fminf(lp, FLT_MAX);
    }
  };
  if (tid == 0) {
    NarBeam& h = beam[0];
    h.am[0] = 0.f; h.ctx[0] = 0.f; h.state[0] = 0; h.node[0] = 0;
    if constexpr (kLm) { blm[0].lm[0] = 0.f; blm[0].lm_state[0] = lm.start; }
  }
  fetch(0);
  __syncthreads();

  int nh = 1;                                                        // every thread keeps the same count
  for (int t = 0; t < T; ++t) {                                      // T, nh, width uniform: every thread reaches every barrier
    const NarBeam& cur = beam[t & 1];
    NarBeam& nxt = beam[(t + 1) & 1];
    const int* const fid = fr_id[t & 1];
    const float* const flp = fr_lp[t & 1];
    const int n = nh * width;                                        // <= 128
    const int h = tid / width, c = tid - h * width;
    // ---- phase A
    if (tid < n) {
      const float am = cur.am[h] + flp[c];
      int st = cur.state[h];
      float cx = cur.ctx[h];
      if (g.n_states > 0) {
        float w;
        st = ctx_step(g, st, fid[c], &w);
        cx = cx + w;
      }
      float tot = am + cx;
      if constexpr (kLm) {
        float w;
        c_lm_state[tid] = lm_step(lm, blm[t & 1].lm_state[h], fid[c], &w);
        const float l = blm[t & 1].lm[h] + w;
        c_lm[tid] = l;
        tot = tot + l;
      }
      if (tot != tot) tot = -INFINITY;
      c_am[tid] = am; c_ctx[tid] = cx; c_state[tid] = st; c_tot[tid] = tot;
    }
    __syncthreads();
    // ---- phase B
    if (tid < n) {
      const float mine = c_tot[tid];
      int rk = 0;
      for (int j = 0; j < n; ++j) {
        const float tj = c_tot[j];
        rk += (tj > mine || (tj == mine && j < tid)) ? 1 : 0;
      }
      if (rk < bw) {
        const int node = 1 + t * beam_stride + rk;                   // <= T * beam_stride
        npar[node - 1] = cur.node[h]; ntok[node - 1] = fid[c];
        nxt.am[rk] = c_am[tid]; nxt.ctx[rk] = c_ctx[tid]; nxt.state[rk] = c_state[tid]; nxt.node[rk] = node;
        if constexpr (kLm) { blm[(t + 1) & 1].lm[rk] = c_lm[tid]; blm[(t + 1) & 1].lm_state[rk] = c_lm_state[tid]; }
      }
    }
    if (t + 1 < T) fetch(t + 1);                                     // buffer (t + 1) & 1: not the one this row reads
    nh = min(n, bw);
    __syncthreads();
  }

  // ---- the end: back-off of an unfinished match (UpdateFinalContext), then the order by total, equal totals in beam order
  const NarBeam& fin = beam[T & 1];
  if (tid < nh) {
    float cx = fin.ctx[tid];
    const int st = fin.state[tid];
    if (g.n_states > 0 && st != 0) cx = cx + g.escape[min(max(st, 0), g.n_states - 1)];
    float tot = fin.am[tid] + cx;
    if constexpr (kLm) {
      float l = blm[T & 1].lm[tid];
      if (lm.has_eos) {
        float w;
        lm_step(lm, blm[T & 1].lm_state[tid], lm.vocab, &w);
        l = l + w;
      }
      c_lm[tid] = l;
      tot = tot + l;
    }
    if (tot != tot) tot = -INFINITY;
    c_tot[tid] = tot; c_ctx[tid] = cx;
  }
  __syncthreads();
  if (tid == 0) n_hyp[b] = min(nh, nbest);
  if (tid >= nh) return;                                             // no barrier follows
  int rk = 0;
  for (int j = 0; j < nh; ++j) rk += (c_tot[j] > c_tot[tid] || (c_tot[j] == c_tot[tid] && j < tid)) ? 1 : 0;
  if (rk >= nbest) return;
  n_tokens[o_h + rk] = T;                                            // every row gave one token; the true count, also above max_tokens
  score[o_h + rk] = c_tot[tid]; am_score[o_h + rk] = fin.am[tid]; ctx_score[o_h + rk] = c_ctx[tid];
  if constexpr (kLm) lm_score[o_h + rk] = c_lm[tid];
  int32_t* const dst = out_ids + (o_h + rk) * max_tokens;
  int node = fin.node[tid];
  const int cap = T * beam_stride;                                   // the last node of this utterance
  for (int pos = T - 1; pos >= 0; --pos) {
    node = min(max(node, 1), cap);
    if (pos < max_tokens) dst[pos] = ntok[node - 1];
    node = npar[node - 1];
  }
}

}  // namespace

size_t nbest_ctx_beam_workspace_bytes(long long rows, int B, int beam_stride) {
  if (rows < 0 || B < 0 || beam_stride < 1) return 0;
  return 2 * sizeof(int32_t) * std::max<size_t>((size_t)rows * beam_stride, 1);
}

bool nbest_ctx_beam_check(const BeamUtt* utt, int B, int k, int n_graphs, bool allow_none, int* beam_max, int* nbest_max) {
  if (B < 0 || B > 65535 || k < 1 || k > kNarWidthMax || n_graphs < 0 || (B > 0 && !utt)) return false;
  int bm = 1, nm = 1;
  for (int b = 0; b < B; ++b) {
    const BeamUtt& u = utt[b];
    if (u.first_beam == 0 && allow_none) continue;                   // no search: the rest is not read
    if (u.first_beam < 1 || u.first_beam > k || u.second_beam < 1 || u.second_beam > kBeamMax || u.nbest < 1 || u.nbest > u.second_beam ||
        u.graph < -1 || u.graph >= n_graphs)
      return false;
    bm = std::max(bm, u.second_beam); nm = std::max(nm, u.nbest);
  }
  if (beam_max) *beam_max = bm;
  if (nbest_max) *nbest_max = nm;
  return true;
}

namespace {

template <bool kLm>
bool launch_nar(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len, const int* len_cap, int B,
                int V, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm, int beam_stride, int nbest_stride,
                int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* am_score, float* ctx_score, float* lm_score,
                void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (kLm && (lm.n_states < 1 || lm.n_arcs < 0 || lm.vocab != V || lm.start < 0 || lm.start >= lm.n_states)) return false;
  if (B < 0 || B > 65535 || rows < 0 || k < 1 || k > kNarWidthMax || beam_stride < 1 || beam_stride > kBeamMax || nbest_stride < 1 ||
      nbest_stride > beam_stride || n_graphs < 0 || V < 1 || max_tokens < 0 || rows * beam_stride + 1 > 0x7fffffffLL)
    return false;
  if (B == 0) return true;
  if (!utt || (n_graphs > 0 && !graphs) || !row_off || !len || !n_hyp || !n_tokens || !score || !am_score || !ctx_score ||
      (max_tokens > 0 && !ids) || (rows > 0 && (!cand_ids || !cand_logp)) || !workspace ||
      workspace_bytes < nbest_ctx_beam_workspace_bytes(rows, B, beam_stride))
    return false;
  if (kLm && (!lm_score || !lm.uni_w || !lm.uni_next || !lm.arc_begin || !lm.backoff_w || !lm.backoff_state ||
              (lm.n_arcs > 0 && (!lm.arc_label || !lm.arc_next || !lm.arc_weight))))
    return false;
  int32_t* const node_parent = static_cast<int32_t*>(workspace);
  int32_t* const node_token = node_parent + std::max<size_t>((size_t)rows * beam_stride, 1);
  hipLaunchKernelGGL(nbest_ctx_beam_kernel<kLm>, dim3(B), dim3(kNT), 0, s, cand_ids, cand_logp, k, rows, row_off, len, len_cap, V, beam_stride,
                     nbest_stride, max_tokens, n_hyp, ids, n_tokens, score, am_score, ctx_score, node_parent, node_token, utt, graphs, n_graphs, lm,
                     lm_score);
  return true;
}

}  // namespace

bool launch_nbest_ctx_beam(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len,
                           const int* len_cap, int B, int V, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, int beam_stride, int nbest_stride,
                           int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* am_score, float* ctx_score,
                           void* workspace, size_t workspace_bytes, hipStream_t s) {
  return launch_nar<false>(cand_ids, cand_logp, k, rows, row_off, len, len_cap, B, V, utt, graphs, n_graphs, LmGraphDev(), beam_stride, nbest_stride,
                           max_tokens, n_hyp, ids, n_tokens, score, am_score, ctx_score, nullptr, workspace, workspace_bytes, s);
}

bool launch_nbest_ctx_beam_lm(const int32_t* cand_ids, const float* cand_logp, int k, long long rows, const int* row_off, const int* len,
                              const int* len_cap, int B, int V, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm,
                              int beam_stride, int nbest_stride, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                              float* am_score, float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, hipStream_t s) {
  return launch_nar<true>(cand_ids, cand_logp, k, rows, row_off, len, len_cap, B, V, utt, graphs, n_graphs, lm, beam_stride, nbest_stride, max_tokens,
                          n_hyp, ids, n_tokens, score, am_score, ctx_score, lm_score, workspace, workspace_bytes, s);
}

}  // namespace pfhip
