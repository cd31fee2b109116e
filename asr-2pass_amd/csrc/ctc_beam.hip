// CTC prefix beam search with hotwords on the device: CtcPrefixDecoder::CtcSearch (onnxruntime/src/ctc-prefix-decoder.cpp:157-263,
// PrefixScore of ctc-prefix-decoder.h:64-110) over the k best columns of every row, as the fused head's top-k form leaves them
// (ctc_head.hip).  No logits matrix is read.  include/pfhip_ops.h (pfhip_op_ctc_prefix_beam) states the recurrence and the tie rule.
//
// One workgroup of 256 threads per utterance walks its len[b] rows in order, as ctc_viterbi_kernel (ctc_align.hip) does.  The beam
// (<= 16 hypotheses: blank-ending score s, non-blank-ending score ns, context score and state, trie node, its parent and token,
// length) is a double buffer in LDS: frame t reads buffer t & 1 and writes the other.  A frame is two phases and two barriers.
//   A  thread p < nh * first_beam forms the extension of hypothesis p / first_beam by candidate p % first_beam (new token, or a
//      repeat after a blank), unless the candidate is the blank or the extension names a live hypothesis; thread h < nh forms the
//      unchanged hypothesis h (blank, repeat) and takes in the extension that names it (the merge).  Candidates land in 16 + 256
//      slots of LDS: unchanged ones at their beam position, extensions behind them, hypothesis-major and candidate-minor.
//   B  every present candidate counts the candidates that beat it (greater total; equal total and lower slot): its rank.  Ranks are
//      unique, so ranks 0 .. second_beam - 1 write the next beam without a race.  A surviving extension at rank r of frame t owns
//      trie node 1 + t * second_beam + r of the utterance: no allocation counter, no atomics.  Threads < first_beam fetch the
//      next row's candidates meanwhile.
// A prefix is its trie node (parent, token); node 0 is the empty prefix.  Two candidates of a frame name the same prefix only when
// an extension (h, tok) equals a live hypothesis h': parent(node_h') == node_h and token(node_h') == tok, tested over the beam.
// Trip counts depend on len[b], the beam sizes and k alone, all uniform in the workgroup; barriers sit in uniform control flow only;
// no spin-wait, no dependency between workgroups, no atomics.  Ids of a row are clamped to 0 .. V - 1, a log-probability that is
// NaN or below -FLT_MAX counts as -FLT_MAX, a NaN total ranks as -inf: whatever the rows hold, ranks stay unique, every beam slot
// that is read was written, and every index stays inside its buffer.  Graph indices are the host builder's (ctx_graph.cpp).
// The final walk from each surviving node to the root writes the ids; it reads nodes other threads wrote, behind a barrier.
//
// kLm = true is the same search with a token n-gram language model (lm_step.h) walked beside the context graph.  The model's state and
// score are a function of the prefix alone: an unchanged hypothesis keeps both, an extension h + tok takes lm_h + the weight of tok
// after lm_state_h (a merged extension is the live hypothesis and keeps that one's, which are the same), every total takes lm as one
// more fp32 add behind the sum it was, and at the end, where the model has </s>, every live hypothesis takes the weight of </s> (after
// the context back-off, before the final order).  kLm = false compiles to what the kernel was before: the model's LDS arrays exist in
// the kLm = true instantiation alone and the extra arguments are not read.
#include "ctx_step.h"
#include "kernels.h"
#include "launch_common.h"
#include "lm_step.h"

#include <float.h>
#include <math.h>

#include <algorithm>

namespace pfhip {
namespace {

constexpr int kBT = 256;                         // threads of the workgroup
constexpr int kBM = kBeamMax;                    // 16
constexpr int kSlots = kBM + kBM * kBM;          // 272 candidate slots
static_assert(kBM * kBM <= kBT, "one thread per (hypothesis, candidate) pair");

// LogAdd of ctc-prefix-decoder.h:31-37: an operand at or below -FLT_MAX is "no path" and the other is returned
__device__ __forceinline__ float log_add(float x, float y) {
  if (x <= -FLT_MAX) return y;
  if (y <= -FLT_MAX) return x;
  const float m = fmaxf(x, y);
  return logf(expf(x - m) + expf(y - m)) + m;
}

struct BeamState {                               // one buffer of the beam
  float s[kBM], ns[kBM], ctx[kBM];
  int state[kBM], node[kBM], par[kBM], tok[kBM], len[kBM];
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
  __device__ static __forceinline__ float* cand_lm() { __shared__ float a[kSlots]; return a; }
  __device__ static __forceinline__ int* cand_state() { __shared__ int a[kSlots]; return a; }
};

// kPerUtt: workgroup b takes first_beam, second_beam, nbest and its graph from utt[b] (launch_ctc_prefix_beam_multi); the arguments
// fb / sb / nbest are then the launch's strides only: sb the node stride of a row, nbest the hypothesis slots of an utterance (fb is
// not read).  Everything read from utt[b] is uniform in the workgroup, so every barrier below still sits in uniform control flow.
template <bool kPerUtt, bool kLm>
__global__ __launch_bounds__(kBT) void ctc_prefix_beam_kernel(const int32_t* __restrict__ topk_ids, const float* __restrict__ topk_logp, int k,
                                                              long long rows, const int* __restrict__ row_off, const int* __restrict__ len,
                                                              int V, int blank, int fb, int sb, CtxGraphDev g, int nbest, int max_tokens,
                                                              int32_t* __restrict__ n_hyp, int32_t* __restrict__ out_ids,
                                                              int32_t* __restrict__ n_tokens, float* __restrict__ score,
                                                              float* __restrict__ ctc_score, float* __restrict__ ctx_score,
                                                              int32_t* __restrict__ node_parent, int32_t* __restrict__ node_token,
                                                              const BeamUtt* __restrict__ utt, const CtxGraphDev* __restrict__ graphs,
                                                              int n_graphs, LmGraphDev lm, float* __restrict__ lm_score) {
  __shared__ BeamState beam[2];
  __shared__ int fr_id[2][kBM];
  __shared__ float fr_lp[2][kBM];
  __shared__ float c_tot[kSlots], c_s[kSlots], c_ns[kSlots], c_ctx[kSlots];
  __shared__ int c_state[kSlots], c_ok[kSlots];
  BeamLm* const blm = LmLds<kLm>::beam();                            // null without a model, and then never read
  float* const c_lm = LmLds<kLm>::cand_lm();
  int* const c_lm_state = LmLds<kLm>::cand_state();

  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = len[b];
  const long long r0 = row_off[b];
  // what this utterance may write: [b][nbest]...; emptied first, so that a refused or rowless utterance reads as "no hypothesis"
  const size_t o_h = (size_t)b * nbest;
  for (int j = tid; j < nbest; j += kBT) {
    n_tokens[o_h + j] = 0;
    score[o_h + j] = -INFINITY; ctc_score[o_h + j] = -INFINITY; ctx_score[o_h + j] = 0.f;
    if constexpr (kLm) lm_score[o_h + j] = 0.f;
  }
  for (size_t j = tid; j < (size_t)nbest * max_tokens; j += kBT) out_ids[o_h * max_tokens + j] = -1;
  // the rows must lie inside the arrays (row_off and len are device data the launcher could not see); T * sb + 1 stays below 2^31
  bool refused = T < 0 || r0 < 0 || r0 + T > rows;
  const int node_stride = sb;
  if constexpr (kPerUtt) {
    // the utterance's own beams: first_beam 0 is "no search"; one outside the launch's strides (k, sb, nbest) or naming no graph of
    // the table has no hypothesis either.  Slots nbest[b] .. of the utterance keep the fill above.
    const BeamUtt u = utt[b];
    refused = refused || u.first_beam < 1 || u.first_beam > min(k, kBM) || u.second_beam < 1 || u.second_beam > min(sb, kBM) || u.nbest < 1 ||
              u.nbest > min(u.second_beam, nbest) || u.graph < -1 || u.graph >= n_graphs;
    if (!refused) {
      fb = u.first_beam; sb = u.second_beam; nbest = u.nbest;
      g = CtxGraphDev();
      if (u.graph >= 0) g = graphs[u.graph];
    }
  }
  if (refused || T == 0) {                                           // uniform
    if (tid == 0) n_hyp[b] = 0;
    return;
  }
  // utterance b's nodes 1 .. T * sb are stored from r0 * node_stride on, inside [r0, r0 + T) * node_stride (sb <= node_stride): node n
  // at n - 1 (the root, node 0, is never read)
  int32_t* const npar = node_parent + (size_t)r0 * node_stride;
  int32_t* const ntok = node_token + (size_t)r0 * node_stride;
  const int32_t* const rid = topk_ids + (size_t)r0 * k;
  const float* const rlp = topk_logp + (size_t)r0 * k;

  auto fetch = [&](int t) {                                          // threads < fb: row t's candidates, sanitised
    if (tid < fb) {
      const int id = rid[(size_t)t * k + tid];
      float lp = rlp[(size_t)t * k + tid];
      if (!(lp >= -FLT_MAX)) lp = -FLT_MAX;                          // NaN, -inf
      fr_id[t & 1][tid] = min(max(id, 0), V - 1);
      fr_lp[t & 1][tid] = fminf(lp, FLT_MAX);
    }
  };
  if (tid == 0) {
    BeamState& h = beam[0];
    h.s[0] = 0.f; h.ns[0] = -FLT_MAX; h.ctx[0] = 0.f;
    h.state[0] = 0; h.node[0] = 0; h.par[0] = -1; h.tok[0] = -1; h.len[0] = 0;
    if constexpr (kLm) { blm[0].lm[0] = 0.f; blm[0].lm_state[0] = lm.start; }
  }
  fetch(0);
  __syncthreads();

  int nh = 1;                                                        // every thread keeps the same count
  for (int t = 0; t < T; ++t) {                                      // T, nh, fb uniform: every thread reaches every barrier
    const BeamState& cur = beam[t & 1];
    BeamState& nxt = beam[(t + 1) & 1];
    const int* const fid = fr_id[t & 1];
    const float* const flp = fr_lp[t & 1];
    // ---- phase A
    if (tid < nh * fb) {
      const int h = tid / fb, c = tid - h * fb;
      const int tok = fid[c];
      bool ok = tok != blank;
      if (ok) {
        const int node_h = cur.node[h];
        for (int h2 = 0; h2 < nh; ++h2)
          if (cur.par[h2] == node_h && cur.tok[h2] == tok) ok = false;       // it IS hypothesis h2: that thread takes the term in
      }
      const int slot = kBM + tid;
      c_ok[slot] = ok;
      if (ok) {
        const float base = tok == cur.tok[h] ? cur.s[h] : log_add(cur.s[h], cur.ns[h]);
        const float ens = base + flp[c];
        int st = cur.state[h];
        float cx = cur.ctx[h];
        if (g.n_states > 0) {
          float w;
          st = ctx_step(g, st, tok, &w);
          cx = cx + w;
        }
        float tot = ens + cx;                                        // LogAdd(-FLT_MAX, ns) = ns
        if constexpr (kLm) {
          float w;
          c_lm_state[slot] = lm_step(lm, blm[t & 1].lm_state[h], tok, &w);
          const float l = blm[t & 1].lm[h] + w;
          c_lm[slot] = l;
          tot = tot + l;
        }
        if (tot != tot) tot = -INFINITY;
        c_s[slot] = -FLT_MAX; c_ns[slot] = ens; c_ctx[slot] = cx; c_state[slot] = st; c_tot[slot] = tot;
      }
    }
    if (tid < kBM) {
      const int h = tid;
      bool ok = false;
      if (h < nh) {
        const int last = cur.tok[h];
        const float sc = log_add(cur.s[h], cur.ns[h]);
        float us = -FLT_MAX, uns = -FLT_MAX;
        for (int c = 0; c < fb; ++c) {
          const int tok = fid[c];
          if (tok == blank) { us = log_add(us, sc + flp[c]); ok = true; }
          else if (tok == last) { uns = log_add(uns, cur.ns[h] + flp[c]); ok = true; }
        }
        const int par = cur.par[h];
        if (par >= 0 && last != blank)
          for (int h2 = 0; h2 < nh; ++h2) {
            if (cur.node[h2] != par) continue;
            const float base = last == cur.tok[h2] ? cur.s[h2] : log_add(cur.s[h2], cur.ns[h2]);
            for (int c = 0; c < fb; ++c)
              if (fid[c] == last) { uns = log_add(uns, base + flp[c]); ok = true; }
          }
        if (ok) {
          float tot = log_add(us, uns) + cur.ctx[h];
          if constexpr (kLm) tot = tot + blm[t & 1].lm[h];
          if (tot != tot) tot = -INFINITY;
          c_s[h] = us; c_ns[h] = uns; c_tot[h] = tot;
        }
      }
      c_ok[h] = ok;
    }
    __syncthreads();
    // ---- phase B
    const int n_slots = kBM + nh * fb;
    int cnt = 0;
    {
      const int i0 = tid, i1 = tid + kBT;
      const bool m0 = i0 < n_slots && c_ok[i0], m1 = i1 < n_slots && c_ok[i1];
      const float t0 = m0 ? c_tot[i0] : 0.f, t1 = m1 ? c_tot[i1] : 0.f;
      int rk0 = 0, rk1 = 0;
      for (int j = 0; j < n_slots; ++j) {
        if (!c_ok[j]) continue;
        const float tj = c_tot[j];
        ++cnt;
        rk0 += (tj > t0 || (tj == t0 && j < i0)) ? 1 : 0;
        rk1 += (tj > t1 || (tj == t1 && j < i1)) ? 1 : 0;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = q ? i1 : i0, rk = q ? rk1 : rk0;
        if (!(q ? m1 : m0) || rk >= sb) continue;
        if (i < kBM) {                                               // an unchanged hypothesis keeps its node
          nxt.s[rk] = c_s[i]; nxt.ns[rk] = c_ns[i]; nxt.ctx[rk] = cur.ctx[i];
          nxt.state[rk] = cur.state[i]; nxt.node[rk] = cur.node[i]; nxt.par[rk] = cur.par[i]; nxt.tok[rk] = cur.tok[i];
          nxt.len[rk] = cur.len[i];
          if constexpr (kLm) { blm[(t + 1) & 1].lm[rk] = blm[t & 1].lm[i]; blm[(t + 1) & 1].lm_state[rk] = blm[t & 1].lm_state[i]; }
        } else {
          const int p = i - kBM, h = p / fb, c = p - h * fb;
          const int node = 1 + t * sb + rk;                          // <= T * sb
          npar[node - 1] = cur.node[h]; ntok[node - 1] = fid[c];
          nxt.s[rk] = c_s[i]; nxt.ns[rk] = c_ns[i]; nxt.ctx[rk] = c_ctx[i];
          nxt.state[rk] = c_state[i]; nxt.node[rk] = node; nxt.par[rk] = cur.node[h]; nxt.tok[rk] = fid[c];
          nxt.len[rk] = cur.len[h] + 1;
          if constexpr (kLm) { blm[(t + 1) & 1].lm[rk] = c_lm[i]; blm[(t + 1) & 1].lm_state[rk] = c_lm_state[i]; }
        }
      }
    }
    if (t + 1 < T) fetch(t + 1);                                     // buffer (t + 1) & 1: not the one this frame reads
    nh = min(cnt, sb);
    __syncthreads();
  }

  // ---- the end: back-off of an unfinished match (UpdateFinalContext, :280-299), then the order by total
  const BeamState& fin = beam[T & 1];
  if (tid < kBM) {
    bool ok = tid < nh;
    if (ok) {
      float cx = fin.ctx[tid];
      const int st = fin.state[tid];
      if (g.n_states > 0 && st != 0) cx = cx + g.escape[min(max(st, 0), g.n_states - 1)];
      const float ctc = log_add(fin.s[tid], fin.ns[tid]);
      float tot = ctc + cx;
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
      c_tot[tid] = tot; c_s[tid] = ctc; c_ctx[tid] = cx;
    }
    c_ok[tid] = ok;
  }
  __syncthreads();
  if (tid == 0) n_hyp[b] = min(nh, nbest);
  if (tid >= nh) return;                                             // no barrier follows
  int rk = 0;
  for (int j = 0; j < nh; ++j) rk += (c_tot[j] > c_tot[tid] || (c_tot[j] == c_tot[tid] && j < tid)) ? 1 : 0;
  if (rk >= nbest) return;
  const int L = fin.len[tid];
  n_tokens[o_h + rk] = L;                                            // the true length, also above max_tokens
  score[o_h + rk] = c_tot[tid]; ctc_score[o_h + rk] = c_s[tid]; ctx_score[o_h + rk] = c_ctx[tid];
  if constexpr (kLm) lm_score[o_h + rk] = c_lm[tid];
  int32_t* const dst = out_ids + (o_h + rk) * max_tokens;
  int node = fin.node[tid];
  const int cap = T * sb;                                            // the last node of this utterance
  for (int pos = L - 1; pos >= 0; --pos) {
    node = min(max(node, 1), cap);
    if (pos < max_tokens) dst[pos] = ntok[node - 1];
    node = npar[node - 1];
  }
}

}  // namespace

size_t ctc_prefix_beam_workspace_bytes(long long rows, int B, int second_beam) {
  if (rows < 0 || B < 0 || second_beam < 1) return 0;
  return 2 * sizeof(int32_t) * std::max<size_t>((size_t)rows * second_beam, 1);
}

bool launch_ctc_prefix_beam(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len, int B,
                            int V, int blank, int first_beam, int second_beam, const CtxGraphDev& graph, int nbest, int max_tokens,
                            int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score, float* ctx_score,
                            void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (B < 0 || B > 65535 || rows < 0 || k < 1 || k > kBeamMax || first_beam < 1 || first_beam > k || second_beam < 1 ||
      second_beam > kBeamMax || nbest < 1 || nbest > second_beam || V < 1 || blank < 0 || blank >= V || max_tokens < 0 ||
      rows * second_beam + 1 > 0x7fffffffLL)
    return false;
  if (graph.n_states < 0 || graph.n_arcs < 0 ||
      (graph.n_states > 0 && (!graph.arc_begin || !graph.escape || (graph.n_arcs > 0 && (!graph.arc_label || !graph.arc_next || !graph.arc_weight)))))
    return false;
  if (B == 0) return true;
  if (!row_off || !len || !n_hyp || !n_tokens || !score || !ctc_score || !ctx_score || (max_tokens > 0 && !ids) ||
      (rows > 0 && (!topk_ids || !topk_logp)) || !workspace || workspace_bytes < ctc_prefix_beam_workspace_bytes(rows, B, second_beam))
    return false;
  int32_t* const node_parent = static_cast<int32_t*>(workspace);
  int32_t* const node_token = node_parent + std::max<size_t>((size_t)rows * second_beam, 1);
  hipLaunchKernelGGL((ctc_prefix_beam_kernel<false, false>), dim3(B), dim3(kBT), 0, s, topk_ids, topk_logp, k, rows, row_off, len, V, blank,
                     first_beam, second_beam, graph, nbest, max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, node_parent, node_token,
                     static_cast<const BeamUtt*>(nullptr), static_cast<const CtxGraphDev*>(nullptr), 0, LmGraphDev(), static_cast<float*>(nullptr));
  return true;
}

bool ctc_prefix_beam_multi_check(const BeamUtt* utt, int B, int k, int n_graphs, int* sb_max, int* nbest_max) {
  if (B < 0 || B > 65535 || k < 1 || k > kBeamMax || n_graphs < 0 || (B > 0 && !utt)) return false;
  int sm = 1, nm = 1;
  for (int b = 0; b < B; ++b) {
    const BeamUtt& u = utt[b];
    if (u.first_beam < 0 || u.first_beam > k || u.second_beam < 0 || u.second_beam > kBeamMax || u.graph < -1 || u.graph >= n_graphs) return false;
    if (u.first_beam == 0) continue;                                 // no search: second_beam and nbest are not read
    if (u.nbest < 1 || u.nbest > u.second_beam) return false;
    sm = std::max(sm, u.second_beam); nm = std::max(nm, u.nbest);
  }
  if (sb_max) *sb_max = sm;
  if (nbest_max) *nbest_max = nm;
  return true;
}

namespace {

template <bool kLm>
bool launch_multi(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len, int B, int V, int blank,
                  const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm, int sb_max, int nbest_max, int max_tokens,
                  int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score, float* ctc_score, float* ctx_score, float* lm_score, void* workspace,
                  size_t workspace_bytes, hipStream_t s) {
  if (kLm && (lm.n_states < 1 || lm.n_arcs < 0 || lm.vocab != V || lm.start < 0 || lm.start >= lm.n_states)) return false;
  if (B < 0 || B > 65535 || rows < 0 || k < 1 || k > kBeamMax || sb_max < 1 || sb_max > kBeamMax || nbest_max < 1 || nbest_max > sb_max ||
      n_graphs < 0 || V < 1 || blank < 0 || blank >= V || max_tokens < 0 || rows * sb_max + 1 > 0x7fffffffLL)
    return false;
  if (B == 0) return true;
  if (!utt || (n_graphs > 0 && !graphs) || !row_off || !len || !n_hyp || !n_tokens || !score || !ctc_score || !ctx_score ||
      (max_tokens > 0 && !ids) || (rows > 0 && (!topk_ids || !topk_logp)) || !workspace ||
      workspace_bytes < ctc_prefix_beam_workspace_bytes(rows, B, sb_max))
    return false;
  if (kLm && (!lm_score || !lm.uni_w || !lm.uni_next || !lm.arc_begin || !lm.backoff_w || !lm.backoff_state ||
              (lm.n_arcs > 0 && (!lm.arc_label || !lm.arc_next || !lm.arc_weight))))
    return false;
  int32_t* const node_parent = static_cast<int32_t*>(workspace);
  int32_t* const node_token = node_parent + std::max<size_t>((size_t)rows * sb_max, 1);
  hipLaunchKernelGGL((ctc_prefix_beam_kernel<true, kLm>), dim3(B), dim3(kBT), 0, s, topk_ids, topk_logp, k, rows, row_off, len, V, blank, 0, sb_max,
                     CtxGraphDev(), nbest_max, max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, node_parent, node_token, utt,
                     graphs, n_graphs, lm, lm_score);
  return true;
}

}  // namespace

bool launch_ctc_prefix_beam_multi(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                  int B, int V, int blank, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, int sb_max,
                                  int nbest_max, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                                  float* ctc_score, float* ctx_score, void* workspace, size_t workspace_bytes, hipStream_t s) {
  return launch_multi<false>(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, utt, graphs, n_graphs, LmGraphDev(), sb_max, nbest_max,
                             max_tokens, n_hyp, ids, n_tokens, score, ctc_score, ctx_score, nullptr, workspace, workspace_bytes, s);
}

bool launch_ctc_prefix_beam_multi_lm(const int32_t* topk_ids, const float* topk_logp, int k, long long rows, const int* row_off, const int* len,
                                     int B, int V, int blank, const BeamUtt* utt, const CtxGraphDev* graphs, int n_graphs, const LmGraphDev& lm,
                                     int sb_max, int nbest_max, int max_tokens, int32_t* n_hyp, int32_t* ids, int32_t* n_tokens, float* score,
                                     float* ctc_score, float* ctx_score, float* lm_score, void* workspace, size_t workspace_bytes, hipStream_t s) {
  return launch_multi<true>(topk_ids, topk_logp, k, rows, row_off, len, B, V, blank, utt, graphs, n_graphs, lm, sb_max, nbest_max, max_tokens,
                            n_hyp, ids, n_tokens, score, ctc_score, ctx_score, lm_score, workspace, workspace_bytes, s);
}

}  // namespace pfhip
