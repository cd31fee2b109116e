// CTC forced alignment: the emissions of the labels asked for, the Viterbi pass over the CTC trellis and the token spans.
//
// A transcript is aligned against a CTC model's log-probabilities without the logits matrix (ctc_head.hip says why there is none):
// of the ~25 000 columns of a row only the blank and the utterance's own labels are needed, ~150 columns.
//
// (a) ctc_emissions_kernel.  Utterance b owns rows [row_off[b], row_off[b] + len[b]) of X [., K] and the labels
//     labels[lab_off[b] .. + n_lab[b]); E_b [len[b]][n_lab[b] + 1] = x_t . W[id_j] + bias[id_j] - lse[row], column 0 the blank, column j
//     label j.  A grouped GEMM whose B operand is a gather of rows of W [V, K].
//     Arithmetic: plain fp32 FMA (fmaf), no MFMA and no fp16 planes.  A K-step of 32 is summed into a fresh partial which is then added
//     to the running sum, so the rounding of a 512-long dot product grows with 32 + 16 terms, not with 512.
//     Tile 64 x 64, K-step 32, 256 threads with 4 x 4 outputs each; operands staged k-major in LDS (2 x 32 x 68 floats = 17 408 B), the
//     next step's global loads issued before this step's FMAs, two barriers a step.  Sizes are on the device, so the grid is fixed
//     (kEmitBlocks workgroups per utterance) and a workgroup strides over its utterance's tiles: every trip count is uniform in the
//     workgroup.  Rows are clamped to the utterance's last row, label slots to its last label, ids to 0 .. V - 1: nothing outside X, W,
//     bias or E_b is touched.  ~2.5 GFLOP for 32 utterances of 30 s: nothing here is tuned further.
//
// (b) ctc_viterbi_kernel.  One workgroup per utterance, states s = 0 .. 2 L strided over its 256 threads (any S = 2 L + 1).  The two
//     score rows are a double buffer in dynamic LDS (8 S bytes), one barrier per frame: frame t reads row (t - 1) & 1 and writes row
//     t & 1, and the barrier that ends frame t orders both against frame t + 1.  Trip counts depend on N and S alone, which are uniform
//     in the workgroup; there is no spin-wait and no dependency between workgroups.  Back-pointers (0 stay, 1, 2) are bytes in a global
//     workspace, utterance b's at byte 2 e_off[b]: its N S <= 2 N (L + 1) bytes fit there because the E_b do not overlap.  Thread 0
//     walks back over the N frames and writes the spans.  The recurrence (pfhip_ops.h states it in full): the largest of stay / step 1 /
//     step 2 (step 2 only into a label state whose label differs from the previous label), a later candidate winning only when strictly
//     greater, then ONE fp32 add of the emission (the file is built with -ffp-contract=off; __fadd_rn says it again).
//
// (c) ctc_greedy_plan_kernel.  What lets (a) and (b) run behind the collapse with no host round trip: from the collapse's token_num
//     [B] (device) and the speech rows N_b (host-known, uploaded with the forward's metadata) it writes n_lab, lab_off — the labels are
//     the collapse's own id buffer [B][maxT] behind the four tags, nothing is copied — and e_off, the exclusive int64 prefix sum of
//     N_b (n_lab + 1).  ONE workgroup of 256 threads, b strided over it in chunks of 256: a Hillis-Steele scan of the chunk in LDS
//     (8 steps, two barriers each) and a running carry every thread keeps in a register.  The trip counts depend on B alone: no
//     spin-wait, no other workgroup, no atomics.  An utterance whose E_b would end beyond cap_floats (what the host allocated from the
//     bound n_lab <= N_b) gets n_lab = -1, which (a) and (b) leave untouched and (b) answers as infeasible.
#include "kernels.h"
#include "launch_common.h"

#include <math.h>

namespace pfhip {
namespace {

constexpr int kET = 64;                          // tile rows = tile columns
constexpr int kEK = 32;                          // K-step
constexpr int kEs = kET + 4;                     // padded LDS row (floats): 16-byte aligned float4 reads
constexpr int kEmitBlocks = 16;                  // workgroups per utterance (32 x 30 s: 24 tiles each)
constexpr int kVitThreads = 256;
constexpr int kPlanThreads = 256;

__device__ __forceinline__ int label_id(const int32_t* __restrict__ lab, int col, int L, int blank, int V) {
  // column 0: the blank; column j: label j.  Columns past the last are clamped onto it (their results are not stored).
  int id = blank;
  if (col > 0 && L > 0) id = lab[min(col, L) - 1];
  return min(max(id, 0), V - 1);
}

__global__ __launch_bounds__(256) void ctc_emissions_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias, const float* __restrict__ lse,
                                                            const int* __restrict__ row_off, const int* __restrict__ len,
                                                            const int* __restrict__ lab_off, const int* __restrict__ n_lab,
                                                            const int32_t* __restrict__ labels, const long long* __restrict__ e_off, int K, int V,
                                                            int blank, float* __restrict__ E, long long e_floats) {
  __shared__ __attribute__((aligned(16))) float Xs[kEK][kEs];
  __shared__ __attribute__((aligned(16))) float Ws[kEK][kEs];
  const int b = blockIdx.y;
  const int N = len[b], L = n_lab[b];
  if (N <= 0 || L < 0) return;                                       // uniform: the whole workgroup leaves
  const int C = L + 1;
  const long long eo = e_off[b];
  // e_floats >= 0 (sizes planned on the device, ctc_greedy_plan_kernel): an E_b that does not lie inside E is not written
  if (e_floats >= 0 && (eo < 0 || eo + (long long)N * C > e_floats)) return;      // uniform
  const int32_t* lab = labels + lab_off[b];
  const int r0 = row_off[b];
  float* Eb = E + eo;
  const int tiles_n = (C + kET - 1) / kET, n_tiles = (N + kET - 1) / kET * tiles_n;
  const int tid = threadIdx.x;
  const int srow = tid >> 2, sq = tid & 3;                           // staging: operand row srow, k = 4 sq .. + 3 and 16 + 4 sq .. + 3
  const int ty = tid >> 4, tx = tid & 15;                            // outputs: rows 4 ty .. + 3, columns 4 tx .. + 3

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // uniform trip count
    const int m0 = tile / tiles_n * kET, n0 = tile % tiles_n * kET;
    const float* Xg = X + (size_t)(r0 + min(m0 + srow, N - 1)) * ldx + 4 * sq;
    const float* Wg = W + (size_t)label_id(lab, n0 + srow, L, blank, V) * ldw + 4 * sq;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    float4 xa = *reinterpret_cast<const float4*>(Xg), xb = *reinterpret_cast<const float4*>(Xg + 16);
    float4 wa = *reinterpret_cast<const float4*>(Wg), wb = *reinterpret_cast<const float4*>(Wg + 16);
    for (int k0 = 0; k0 < K; k0 += kEK) {
      __syncthreads();                                               // the previous step (or tile) has read the stage
      Xs[4 * sq][srow] = xa.x; Xs[4 * sq + 1][srow] = xa.y; Xs[4 * sq + 2][srow] = xa.z; Xs[4 * sq + 3][srow] = xa.w;
      Xs[16 + 4 * sq][srow] = xb.x; Xs[17 + 4 * sq][srow] = xb.y; Xs[18 + 4 * sq][srow] = xb.z; Xs[19 + 4 * sq][srow] = xb.w;
      Ws[4 * sq][srow] = wa.x; Ws[4 * sq + 1][srow] = wa.y; Ws[4 * sq + 2][srow] = wa.z; Ws[4 * sq + 3][srow] = wa.w;
      Ws[16 + 4 * sq][srow] = wb.x; Ws[17 + 4 * sq][srow] = wb.y; Ws[18 + 4 * sq][srow] = wb.z; Ws[19 + 4 * sq][srow] = wb.w;
      __syncthreads();
      if (k0 + kEK < K) {                                            // in flight under this step's FMAs
        xa = *reinterpret_cast<const float4*>(Xg + k0 + kEK); xb = *reinterpret_cast<const float4*>(Xg + k0 + kEK + 16);
        wa = *reinterpret_cast<const float4*>(Wg + k0 + kEK); wb = *reinterpret_cast<const float4*>(Wg + k0 + kEK + 16);
      }
      float part[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[i][j] = 0.f;
#pragma unroll
      for (int k = 0; k < kEK; ++k) {
        const float4 a4 = *reinterpret_cast<const float4*>(&Xs[k][4 * ty]);
        const float4 b4 = *reinterpret_cast<const float4*>(&Ws[k][4 * tx]);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, w[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) part[i][j] = fmaf(a[i], w[j], part[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + 4 * tx + j;
      if (col >= C) continue;
      const float bj = bias[label_id(lab, col, L, blank, V)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = m0 + 4 * ty + i;
        if (t < N) Eb[(size_t)t * C + col] = (acc[i][j] + bj) - lse[r0 + t];
      }
    }
  }
}

__global__ __launch_bounds__(kVitThreads) void ctc_viterbi_kernel(const float* __restrict__ E, const long long* __restrict__ e_off,
                                                                  const int* __restrict__ len, const int* __restrict__ n_lab,
                                                                  const int32_t* __restrict__ labels, const int* __restrict__ lab_off,
                                                                  int max_tokens, long long e_floats, int32_t* __restrict__ tok_begin,
                                                                  int32_t* __restrict__ tok_end, float* __restrict__ tok_logp,
                                                                  float* __restrict__ score, unsigned char* __restrict__ bp_all) {
  extern __shared__ float v[];                                       // [2][S]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = len[b], L = n_lab[b];
  const size_t out0 = (size_t)b * max_tokens;
  for (int j = tid; j < max_tokens; j += kVitThreads) {
    tok_begin[out0 + j] = -1; tok_end[out0 + j] = -1;
    if (tok_logp) tok_logp[out0 + j] = -INFINITY;
  }
  // what the launcher could not see (sizes live on the device): an utterance whose labels exceed max_tokens (the LDS rows and the
  // outputs are sized by it) or whose E_b does not lie inside E is answered as infeasible, never read or written
  const long long eo = e_off[b];
  const bool refused = L < 0 || L > max_tokens || N < 0 || eo < 0 || eo + (long long)N * (L + 1) > e_floats;
  if (refused || N == 0) {                                           // uniform
    if (tid == 0) score[b] = (!refused && L == 0) ? 0.f : -INFINITY;
    return;
  }
  const int S = 2 * L + 1, C = L + 1;
  const float* Eb = E + eo;
  const int32_t* lab = labels + lab_off[b];
  unsigned char* bp = bp_all + 2 * (size_t)eo;
  for (int s = tid; s < S; s += kVitThreads) v[s] = s == 0 ? Eb[0] : (s == 1 ? Eb[1] : -INFINITY);
  __syncthreads();
  for (int t = 1; t < N; ++t) {                                      // N, S uniform: every thread reaches every barrier
    const float* vp = v + ((t - 1) & 1) * S;
    float* vc = v + (t & 1) * S;
    const float* Et = Eb + (size_t)t * C;
    for (int s = tid; s < S; s += kVitThreads) {
      const int j = (s + 1) >> 1;                                    // label state: label j (1-based), column j
      float best = vp[s];
      int step = 0;
      if (s >= 1) {
        const float c1 = vp[s - 1];
        if (c1 > best) { best = c1; step = 1; }
        if ((s & 1) && s >= 3 && lab[j - 1] != lab[j - 2]) {
          const float c2 = vp[s - 2];
          if (c2 > best) { best = c2; step = 2; }
        }
      }
      vc[s] = __fadd_rn(best, Et[(s & 1) ? j : 0]);
      bp[(size_t)t * S + s] = (unsigned char)step;
    }
    __syncthreads();                                                 // also makes the back-pointers visible to thread 0
  }
  if (tid != 0) return;
  const float* vl = v + ((N - 1) & 1) * S;
  int s = 0;
  if (L > 0) s = vl[2 * L] >= vl[2 * L - 1] ? 2 * L : 2 * L - 1;
  const float sc = vl[s];
  score[b] = sc;
  if (!(sc > -INFINITY)) return;                                     // infeasible: the spans stay -1
  int cur = -1, first = 0;                                           // the token whose frames are being walked, and its earliest frame so far
  auto close = [&]() {
    if (cur < 0) return;
    tok_begin[out0 + cur] = first;
    if (tok_logp) tok_logp[out0 + cur] = Eb[(size_t)first * C + cur + 1];
  };
  for (int t = N - 1; t >= 0; --t) {
    if (s & 1) {
      const int j = s >> 1;
      if (j != cur) { close(); cur = j; tok_end[out0 + j] = t + 1; }
      first = t;
    }
    if (t > 0) s -= bp[(size_t)t * S + s];
  }
  close();
}


__global__ __launch_bounds__(kPlanThreads) void ctc_greedy_plan_kernel(const int32_t* __restrict__ token_num, const int* __restrict__ speech_len,
                                                                       int B, int maxT, long long cap_floats, int* __restrict__ n_lab,
                                                                       int* __restrict__ lab_off, long long* __restrict__ e_off,
                                                                       long long* __restrict__ total) {
  __shared__ long long sh[kPlanThreads];
  const int tid = threadIdx.x;
  long long carry = 0;                                               // the floats of every utterance before this chunk
  for (int b0 = 0; b0 < B; b0 += kPlanThreads) {                     // uniform trip count
    const int b = b0 + tid;
    int L = 0;
    long long size = 0;
    if (b < B) {
      const int tn = token_num[b], N = speech_len[b];
      L = tn > 4 ? tn - 4 : 0;
      if (tn > maxT || N < 0) L = -1;                                // counts no collapse over maxT rows leaves: labels would lie outside ids[b]
      else size = (long long)N * (L + 1);
    }
    sh[tid] = size;
    __syncthreads();
    for (int off = 1; off < kPlanThreads; off <<= 1) {               // inclusive scan of the chunk
      const long long add = tid >= off ? sh[tid - off] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    const long long incl = sh[tid], chunk = sh[kPlanThreads - 1];
    if (b < B) {
      const long long eo = carry + incl - size;
      if (L >= 0 && (eo < 0 || eo + size < eo || eo + size > cap_floats)) L = -1;      // E_b would end beyond what is allocated
      n_lab[b] = L;
      lab_off[b] = b * maxT + 4;
      e_off[b] = eo;
    }
    carry += chunk;
    __syncthreads();                                                 // sh is rewritten by the next chunk
  }
  if (tid == 0 && total) *total = carry;
}

}  // namespace

bool launch_ctc_emissions(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* lse, const int* row_off,
                          const int* len, const int* lab_off, const int* n_lab, const int32_t* labels, const long long* e_off, int B, int K,
                          int V, int blank, float* E, hipStream_t s, long long e_floats) {
  if (B < 0 || B > 65535 || V <= 0 || K < 32 || K % 32 || ldx < K || ldx % 4 || ldw < K || ldw % 4 || blank < 0 || blank >= V) return false;
  if (B == 0) return true;
  if (!X || !W || !bias || !lse || !row_off || !len || !lab_off || !n_lab || !labels || !e_off || !E) return false;
  hipLaunchKernelGGL(ctc_emissions_kernel, dim3(kEmitBlocks, B), dim3(256), 0, s, X, ldx, W, ldw, bias, lse, row_off, len, lab_off, n_lab,
                     labels, e_off, K, V, blank, E, e_floats);
  return true;
}

bool launch_ctc_greedy_plan(const int32_t* token_num, const int* speech_len, int B, int maxT, long long cap_floats, int* n_lab, int* lab_off,
                            long long* e_off, long long* total, hipStream_t s) {
  // lab_off[b] = b maxT + 4 is an int: the id buffer [B][maxT] must be indexable by one
  if (B < 0 || B > 65535 || maxT < 0 || cap_floats < 0 || (long long)B * maxT + 4 > 0x7fffffffLL) return false;
  if (B == 0) return true;
  if (!token_num || !speech_len || !n_lab || !lab_off || !e_off) return false;
  hipLaunchKernelGGL(ctc_greedy_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, token_num, speech_len, B, maxT, cap_floats, n_lab, lab_off,
                     e_off, total);
  return true;
}

size_t ctc_align_workspace_bytes(size_t e_floats) { return 2 * e_floats; }
int ctc_align_max_tokens() { return (64 * 1024 / 8 - 1) / 2; }       // 8 (2 L + 1) <= 65 536: L <= 4095

bool launch_ctc_align(const float* E, const long long* e_off, size_t e_floats, const int* len, const int* n_lab, const int32_t* labels,
                      const int* lab_off, int B, int max_tokens, int32_t* tok_begin, int32_t* tok_end, float* tok_logp, float* score,
                      void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (B < 0 || max_tokens < 0 || max_tokens > ctc_align_max_tokens() || e_floats > ((size_t)1 << 61)) return false;
  if (B == 0) return true;
  if (!E || !e_off || !len || !n_lab || !labels || !lab_off || !tok_begin || !tok_end || !score || !workspace ||
      workspace_bytes < ctc_align_workspace_bytes(e_floats))
    return false;
  const int lds = 8 * (2 * max_tokens + 1);
  hipLaunchKernelGGL(ctc_viterbi_kernel, dim3(B), dim3(kVitThreads), lds, s, E, e_off, len, n_lab, labels, lab_off, max_tokens,
                     (long long)e_floats, tok_begin, tok_end, tok_logp, score, static_cast<unsigned char*>(workspace));
  return true;
}

}  // namespace pfhip
