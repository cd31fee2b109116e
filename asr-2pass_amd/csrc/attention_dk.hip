// Fused multi-head attention for head widths that attention.hip is not instantiated for: any 1 <= d_k <= 64, fp32 on
// v_mfma_f32_32x32x2_f32 (the large CT-Transformer: 516 / 12 heads = 43).  The arithmetic is attention.hip's attention_kernel<HD>
// — one workgroup = 4 waves = 128 query rows of one (sequence, head), key/value tiles of 32 keys double buffered in LDS, swapped
// QK^T (key on the MFMA row, query on the lane), online softmax in the base-2 domain, per-query key limits — with the width split
// in two: HDP, the template parameter, is the padded width the tiles and the MFMA loops are laid out for (32, 48 or 64); d_k, a
// runtime argument, is what memory holds.
//
// What differs from attention_kernel:
//   * head h starts at column h * d_k, which is aligned to 4 bytes only (43 floats): every global access is a dword.  Q, the K / V
//     staging and the output store move single floats; a thread still owns the four columns 4 c .. 4 c + 3 of a staged row.
//   * no access touches a column at or beyond d_k of its head: in Q and K a neighbour head's values would enter the scores, and
//     the last head of the last row would leave the buffer.  Pad columns [d_k, HDP) are staged as zeros (Q, K and V alike), so
//     the pad rows of O^T are zeros that are never stored.
//   * where HDP is no multiple of 32 (48) the lanes of the last d-tile past HDP re-read the tile's last column in LDS, as the
//     HD = 80 form of attention_kernel does; their accumulator rows are dropped.
//   * the store writes d_k floats per (row, head) and nothing else.
#include "kernels.h"
#include "launch_common.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

namespace pfhip {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kQW = 32;            // query rows per wave
constexpr int kQB = 128;           // query rows per block
constexpr int kKT = 32;            // keys per tile

template <int HDP>
__global__ __launch_bounds__(256, 2) void attention_dk_kernel(
    const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
    const float* __restrict__ V, int ldv, float* __restrict__ O, int ldo,
    const int* __restrict__ q_off, const int* __restrict__ q_len, const int* __restrict__ kv_off,
    const int* __restrict__ kv_len, const int* __restrict__ q_kv_limit, float scale, int d_k) {
  constexpr int kKS = HDP + 4;                       // padded K-tile row stride: conflict-free ds_read_b128
  constexpr int kKVBuf = kKT * kKS + kKT * HDP;      // floats per (K,V) buffer
  constexpr int kLdsFloats = (2 * kKVBuf > 4 * kQW * kKS) ? 2 * kKVBuf : 4 * kQW * kKS;
  constexpr int NKB = HDP / 8;                       // MFMA k-blocks of the QK^T product
  constexpr int ND = (HDP + 31) / 32;                // 32-wide d tiles of the output (the last one partly live when HDP % 32)
  constexpr int C4 = HDP / 4;                        // four-column chunks per row
  constexpr int RPP = 256 / C4;                      // rows per staging pass (RPP * C4 of the 256 threads move a chunk each)
  constexpr int NP = (kKT + RPP - 1) / RPP;          // staging passes
  constexpr bool kRagged = (256 % C4) != 0 || (kKT % RPP) != 0;      // some (thread, pass) pairs have no row (HDP = 48)
  static_assert(HDP % 8 == 0 && HDP <= 64 && ND <= 2 && NP <= 2 && NKB >= 2 * NP, "staging / tiling slots");
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];

  // grid = (head, sequence, query block), as attention_kernel: the query blocks of one (sequence, head) share an XCD's L2
  const int b = blockIdx.y, head = blockIdx.x;
  const int Lq = q_len[b];
  const int q0 = blockIdx.z * kQB;
  const int Lk = kv_len[b];
  if (q0 >= Lq || Lk <= 0) return;
  const size_t qbase = (size_t)q_off[b], kbase = (size_t)kv_off[b];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- Q slice of this lane: row q0 + wave*32 + r, d = 8*kb + 4*h + kk; zero at d >= d_k ----------
  float4 qreg[NKB];
  int klim = Lk;              // keys this lane's query may see: all, or a per-query prefix (CT-Transformer VadMask)
  {
    int qrow = q0 + wave * kQW + r;
    if (qrow >= Lq) qrow = Lq - 1;
    if (q_kv_limit) { const int l = q_kv_limit[qbase + qrow]; klim = l < Lk ? l : Lk; }
    const float* qp = Q + (qbase + qrow) * ldq + (size_t)head * d_k;
    // Q is pre-multiplied by scale * log2(e): the scores come out of the MFMAs in the base-2 softmax domain
    const float qs = scale * 1.44269504088896340736f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int c = kb * 8 + 4 * h;
      float4 qv;
      qv.x = c + 0 < d_k ? qp[c + 0] * qs : 0.f;
      qv.y = c + 1 < d_k ? qp[c + 1] * qs : 0.f;
      qv.z = c + 2 < d_k ? qp[c + 2] * qs : 0.f;
      qv.w = c + 3 < d_k ? qp[c + 3] * qs : 0.f;
      qreg[kb] = qv;
    }
  }
  const bool limited = q_kv_limit != nullptr;      // per-query key limits: every tile takes the masked path

  // ---- K/V tile staging (named registers + sched_barriers, as attention_kernel) --------------------
  const int lrow = tid / C4, lc4 = tid % C4;   // RPP rows x C4 chunks per pass, NP passes
  float4 rk0, rk1, rv0, rv1;
  rk0 = rv0 = rk1 = rv1 = make_float4(0.f, 0.f, 0.f, 0.f);
  // which of this thread's four columns the head has (the others stay zero in the tile)
  const bool c0 = 4 * lc4 + 0 < d_k, c1 = 4 * lc4 + 1 < d_k, c2 = 4 * lc4 + 2 < d_k, c3 = 4 * lc4 + 3 < d_k;
  // whether this thread has a row in staging pass i
#define PFHIP_STAGE_LIVE(i) (!kRagged || (lrow < RPP && lrow + RPP * (i) < kKT))
  const float* Kh = K + kbase * ldk + (size_t)head * d_k + 4 * lc4;
  const float* Vh = V + kbase * ldv + (size_t)head * d_k + 4 * lc4;
  // one row group (RPP keys) of the next K or V tile -> staging registers / staging registers -> LDS
#define PFHIP_ROW_LOAD(R, P, ld, i, kt)                                                 \
  do {                                                                                  \
    int key_ = (kt) * kKT + lrow + RPP * (i);                                           \
    key_ = key_ < Lk ? key_ : Lk - 1;                                                   \
    if (PFHIP_STAGE_LIVE(i)) {                                                          \
      const float* p_ = (P) + (size_t)key_ * (ld);                                      \
      R.x = c0 ? p_[0] : 0.f; R.y = c1 ? p_[1] : 0.f;                                   \
      R.z = c2 ? p_[2] : 0.f; R.w = c3 ? p_[3] : 0.f;                                   \
    }                                                                                   \
  } while (0)
#define PFHIP_K_LOAD(RK, i, kt) PFHIP_ROW_LOAD(RK, Kh, ldk, i, kt)
#define PFHIP_V_LOAD(RV, i, kt) PFHIP_ROW_LOAD(RV, Vh, ldv, i, kt)
#define PFHIP_K_STORE(RK, i, buf) \
  do { if (PFHIP_STAGE_LIVE(i)) *reinterpret_cast<float4*>(lds + (buf) * kKVBuf + (lrow + RPP * (i)) * kKS + 4 * lc4) = RK; } while (0)
#define PFHIP_V_STORE(RV, i, buf) \
  do { if (PFHIP_STAGE_LIVE(i)) *reinterpret_cast<float4*>(lds + (buf) * kKVBuf + kKT * kKS + (lrow + RPP * (i)) * HDP + 4 * lc4) = RV; } while (0)

  f32x16 oacc0, oacc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { oacc0[e] = 0.f; oacc1[e] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  const int nkt = (Lk + kKT - 1) / kKT;
  PFHIP_K_LOAD(rk0, 0, 0); PFHIP_V_LOAD(rv0, 0, 0);
  if (NP > 1) { PFHIP_K_LOAD(rk1, 1, 0); PFHIP_V_LOAD(rv1, 1, 0); }
  PFHIP_K_STORE(rk0, 0, 0); PFHIP_V_STORE(rv0, 0, 0);
  if (NP > 1) { PFHIP_K_STORE(rk1, 1, 0); PFHIP_V_STORE(rv1, 1, 0); }
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    // unconditional prefetch of the next tile (the last iteration re-fetches its own): straight-line body
    const int ktn = kt + 1 < nkt ? kt + 1 : kt;
    const float* ks = lds + cur * kKVBuf;
    const float* vs = ks + kKT * kKS;

    // S^T[key][q] = sum_d K[key][d] * Q[q][d]; the K fragment of k-block kb+1 is read under the 4 MFMAs of kb.
    // Two accumulators, alternated, so consecutive MFMAs never wait for each other's result.
    f32x16 sacc, sacb;
#pragma unroll
    for (int e = 0; e < 16; ++e) { sacc[e] = 0.f; sacb[e] = 0.f; }
    const float* kp = ks + r * kKS + 4 * h;
    float4 ka = *reinterpret_cast<const float4*>(kp);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const float4 kn = *reinterpret_cast<const float4*>(kp + (kb < NKB - 1 ? kb + 1 : kb) * 8);
      if (kb == 0) PFHIP_K_LOAD(rk0, 0, ktn);
      if (kb == 1) PFHIP_V_LOAD(rv0, 0, ktn);
      if (NP > 1) {
        if (kb == 2) PFHIP_K_LOAD(rk1, 1, ktn);
        if (kb == 3) PFHIP_V_LOAD(rv1, 1, ktn);
      }
      __builtin_amdgcn_sched_barrier(0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.x, qreg[kb].x, sacc, 0, 0, 0);
      sacb = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.y, qreg[kb].y, sacb, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.z, qreg[kb].z, sacc, 0, 0, 0);
      sacb = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.w, qreg[kb].w, sacb, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      ka = kn;
    }

    // online softmax (base 2) for query column r; this lane holds keys (e&3) + 8*(e>>2) + 4*h of the tile.
    // Tiles that lie wholly inside the key range skip the masking (wave-uniform branch).
    float tmax = -INFINITY;
    if (!limited && (kt + 1) * kKT <= Lk) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float sv = sacc[e] + sacb[e];
        sacc[e] = sv;
        tmax = fmaxf(tmax, sv);
      }
    } else {
      const int key0 = kt * kKT + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = key0 + (e & 3) + 8 * (e >> 2);
        const float sv = (key < klim) ? sacc[e] + sacb[e] : -INFINITY;
        sacc[e] = sv;
        tmax = fmaxf(tmax, sv);
      }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pv = __builtin_amdgcn_exp2f(sacc[e] - m_new);
      sacc[e] = pv;
      psum += pv;
    }
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    if (__any(alpha != 1.0f)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        oacc0[e] *= alpha;
        if (ND > 1) oacc1[e] *= alpha;
      }
    }

    // O^T[d][q] += sum_key V[key][d] * P^T[key][q]; V values of step e+1 are read under the MFMAs of e
    const float* vp = vs + (4 * h) * HDP + r;
    // column of this lane in d-tile 1, relative to r: lanes past the padded width re-read its last column (their rows of O^T are dropped)
    const int c1v = HDP % 32 == 0 ? 32 : (32 + r < HDP ? 32 + r : HDP - 1) - r;
    float va0 = vp[0], va1 = 0.f;
    if (ND > 1) va1 = vp[c1v];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int en = e < 15 ? e + 1 : e;
      const float* vrow = vp + ((en & 3) + 8 * (en >> 2)) * HDP;
      const float vn0 = vrow[0];
      float vn1 = 0.f;
      if (ND > 1) vn1 = vrow[c1v];
      if (e == 0) PFHIP_K_STORE(rk0, 0, cur ^ 1);
      if (e == 1) PFHIP_V_STORE(rv0, 0, cur ^ 1);
      if (NP > 1) {
        if (e == 2) PFHIP_K_STORE(rk1, 1, cur ^ 1);
        if (e == 3) PFHIP_V_STORE(rv1, 1, cur ^ 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      const float pb = sacc[e];
      oacc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0, pb, oacc0, 0, 0, 0);
      if (ND > 1) oacc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1, pb, oacc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      va0 = vn0; va1 = vn1;
    }
    __syncthreads();
  }
#undef PFHIP_K_LOAD
#undef PFHIP_V_LOAD
#undef PFHIP_ROW_LOAD
#undef PFHIP_K_STORE
#undef PFHIP_V_STORE
#undef PFHIP_STAGE_LIVE

  // ---- normalise, transpose through LDS, store d_k floats per row ------------------------------------
  const float inv_l = 1.0f / l_run;
  float* os = lds + wave * (kQW * kKS);
#define PFHIP_O_STORE(OACC, dt)                                                          \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                        \
    float4 o4;                                                                           \
    o4.x = OACC[4 * g + 0] * inv_l; o4.y = OACC[4 * g + 1] * inv_l;                      \
    o4.z = OACC[4 * g + 2] * inv_l; o4.w = OACC[4 * g + 3] * inv_l;                      \
    /* registers 4g..4g+3 are d = dt*32 + 8g + 4h + (0..3) of query column r */          \
    if ((dt) * 32 + 8 * g + 8 <= HDP)                                                    \
      *reinterpret_cast<float4*>(os + r * kKS + (dt) * 32 + 8 * g + 4 * h) = o4;         \
  }
  PFHIP_O_STORE(oacc0, 0)
  if (ND > 1) { PFHIP_O_STORE(oacc1, 1) }
#undef PFHIP_O_STORE
  __syncthreads();
  // each wave stores its own 32 x d_k tile row by row: lane c of a row writes column c (d_k <= 64 lanes, one dword each)
  if (lane < d_k) {
    float* op = O + (qbase + q0 + wave * kQW) * ldo + (size_t)head * d_k + lane;
    const int rows = Lq - (q0 + wave * kQW) < kQW ? Lq - (q0 + wave * kQW) : kQW;      // <= 0: the wave has no live row
#pragma unroll 4
    for (int row = 0; row < rows; ++row) op[(size_t)row * ldo] = os[row * kKS + lane];
  }
}

}  // namespace

// The caller (pfhip_punc_*, pfhip_op_attention_dk) has checked 1 <= head_dim <= 64 and the leading dimensions; a width outside the
// range here is a programming error, as a wrong head width is in attention.hip.
void launch_attention_dk(const AttnOp& o, hipStream_t s) {
  if (o.B <= 0 || o.max_q_len <= 0 || o.H <= 0) return;
  if (o.head_dim < 1 || o.head_dim > 64) { fprintf(stderr, "pfhip: no attention_dk kernel for head width %d\n", o.head_dim); abort(); }
  const dim3 grid(o.H, o.B, (o.max_q_len + kQB - 1) / kQB), block(256);
#define PFHIP_ATT(HDP_)                                                                                                                \
  hipLaunchKernelGGL(attention_dk_kernel<HDP_>, grid, block, 0, s, o.Q, o.ldq, o.K, o.ldk, o.V, o.ldv, o.O, o.ldo, o.q_off, o.q_len, o.kv_off, \
                     o.kv_len, o.q_kv_limit, o.scale, o.head_dim)
  if (o.head_dim <= 32) PFHIP_ATT(32);
  else if (o.head_dim <= 48) PFHIP_ATT(48);
  else PFHIP_ATT(64);
#undef PFHIP_ATT
}

}  // namespace pfhip
