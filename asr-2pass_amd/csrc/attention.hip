// Fused multi-head attention (SAN-M self-attention and decoder cross-attention), fp32 on
// v_mfma_f32_32x32x2_f32, flash-style online softmax.  Stands in for the MatMul/Softmax/MatMul nodes
// of every attention block inside the reference's `m_session_->Run` (onnxruntime/src/paraformer.cpp:541).
//
// One workgroup = 4 waves = 128 query rows of one (utterance, head); each wave owns 32 query rows and
// keeps its Q slice in registers.  Key/value tiles of 32 keys are staged global -> registers -> LDS,
// double buffered.  Per tile a wave computes S^T = K * Q^T (key on the MFMA row, query on the lane:
// "swapped QK^T"), so that
//   * a query's 32 scores live in one lane pair (l, l^32): row max / row sum = 16 register ops + one
//     cross-half shuffle, no LDS;
//   * P^T is already laid out as the B operand of O^T += V^T * P^T — the probabilities never leave
//     their registers; V^T fragments are read from the row-major V tile with conflict-free
//     ds_read_b32 (32 consecutive d per lane half);
//   * O^T keeps the query on the lane too, so the online-softmax rescale is a per-lane scalar multiply.
// The output tile is transposed through LDS once at the end and stored as full 512-B rows.
// Keys >= kv_len are masked to -inf; tile rows past the segment end are clamped to the last valid
// row, so no out-of-segment memory is read.
//
// The kernel has two forms.  The aligned form (d_k = 32, 80, 128: the template width is the head width) moves float4s: head h
// starts at column h * HD, and the caller guarantees 16-byte alignment.  The exact-width form serves any 1 <= d_k <= 64 (the large
// CT-Transformer: 516 / 12 heads = 43) with the width split in two: HD, the template parameter, is the padded width the tiles and
// the MFMA loops are laid out for (32, 48 or 64); d_k, a runtime argument, is what memory holds.  What it does differently:
//   1. head h starts at column h * d_k, which is aligned to 4 bytes only (43 floats): every global access is a dword;
//   2. Q is loaded as four bounds-checked dwords: no access touches a column at or beyond d_k of its head (a neighbour head's
//      values would enter the scores, and the last head of the last row would leave the buffer);
//   3. K and V rows are staged as four bounds-checked dwords, a thread still owning the columns 4 c .. 4 c + 3 of a row; the pad
//      columns [d_k, HD) are staged as zeros (Q, K and V alike), so the pad rows of O^T are zeros that are never stored;
//   4. it returns before any load where the key segment is empty (kv_len <= 0);
//   5. the store writes d_k floats per (row, head) and nothing else: one dword per lane per row for lane < d_k.
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

// HD = head dimension: 128 (Paraformer SAN-M / cross-attention), 80 (the small Paraformer: 320 / 4 heads) or 32 (CT-Transformer,
// 256 / 8 heads).  80 is no multiple of the 32-wide tiles: the K/V tile is staged by 240 of the 256 threads (12 rows x 20 float4 per
// pass, three passes), the output has two full d-tiles and one of 16 live rows (the V column of its dead lanes is clamped to the
// head's last one and their accumulator rows are never stored), and a wave stores three 320-B rows per pass.  The exact-width form
// at HD = 48 is ragged in the same way (192 threads, 16 rows x 12 chunks per pass, two passes, a second d-tile of 16 live rows).
template <int HD, bool kExact>
__global__ __launch_bounds__(256, 2) void attention_kernel(
    const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
    const float* __restrict__ V, int ldv, float* __restrict__ O, int ldo,
    const int* __restrict__ q_off, const int* __restrict__ q_len, const int* __restrict__ kv_off,
    const int* __restrict__ kv_len, const int* __restrict__ q_kv_limit, float scale, int d_k) {
  constexpr int kKS = HD + 4;                        // padded K-tile row stride: conflict-free ds_read_b128
  constexpr int kKVBuf = kKT * kKS + kKT * HD;       // floats per (K,V) buffer
  constexpr int kLdsFloats = (2 * kKVBuf > 4 * kQW * kKS) ? 2 * kKVBuf : 4 * kQW * kKS;
  constexpr int NKB = HD / 8;                        // MFMA k-blocks of the QK^T product
  constexpr int ND = (HD + 31) / 32;                 // 32-wide d tiles of the output (the last one partly live when HD % 32)
  constexpr int C4 = HD / 4;                         // float4 chunks per row
  constexpr int RPP = 256 / C4;                      // rows per staging pass (RPP * C4 of the 256 threads move a float4 each)
  constexpr int NP = (kKT + RPP - 1) / RPP;          // staging passes
  constexpr bool kRagged = (256 % C4) != 0 || (kKT % RPP) != 0;      // some (thread, pass) pairs have no row (HD = 80)
  static_assert(HD % 8 == 0 && ND <= 4 && NP <= 4 && NKB >= 2 * NP, "staging / tiling slots");
  static_assert(!kExact || HD <= 64, "the exact-width store has one lane per column");
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];

  // grid = (head, utterance, query block): consecutive workgroups go to consecutive XCDs, so with the query block as the
  // SLOWEST index all query blocks of one (utterance, head) land on the same XCD and share its K/V tiles in that L2
  const int b = blockIdx.y, head = blockIdx.x;
  const int Lq = q_len[b];
  const int q0 = blockIdx.z * kQB;
  const int Lk = kv_len[b];
  if (q0 >= Lq || (kExact && Lk <= 0)) return;      // (the aligned forms have no guard for an empty key segment)
  const size_t qbase = (size_t)q_off[b], kbase = (size_t)kv_off[b];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // first column of this head: a 64-bit product where d_k is a run-time value
#define PFHIP_HCOL (kExact ? (size_t)head * d_k : (size_t)(head * HD))
  // ---- Q slice of this lane: row q0 + wave*32 + r, d = 8*kb + 4*h + kk; zero at d >= d_k ---------
  float4 qreg[NKB];
  int klim = Lk;              // keys this lane's query may see: all, or a per-query prefix (CT-Transformer VadMask)
  {
    int qrow = q0 + wave * kQW + r;
    if (qrow >= Lq) qrow = Lq - 1;
    if (q_kv_limit) { const int l = q_kv_limit[qbase + qrow]; klim = l < Lk ? l : Lk; }
    const float* qp = Q + (qbase + qrow) * ldq + PFHIP_HCOL + (kExact ? 0 : 4 * h);      // (exact width: 4 h is in the column below)
    // Q is pre-multiplied by scale * log2(e): the scores come out of the MFMAs in the base-2 softmax domain, which
    // saves a multiply per score per tile (the softmax below is exp2(s - m); its ratios are those of exp)
    const float qs = scale * 1.44269504088896340736f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      float4 qv;
      if constexpr (kExact) {
        const int c = kb * 8 + 4 * h;
        qv.x = c + 0 < d_k ? qp[c + 0] * qs : 0.f;
        qv.y = c + 1 < d_k ? qp[c + 1] * qs : 0.f;
        qv.z = c + 2 < d_k ? qp[c + 2] * qs : 0.f;
        qv.w = c + 3 < d_k ? qp[c + 3] * qs : 0.f;
      } else {
        qv = *reinterpret_cast<const float4*>(qp + kb * 8);
        qv.x *= qs; qv.y *= qs; qv.z *= qs; qv.w *= qs;
      }
      qreg[kb] = qv;
    }
  }
  const bool limited = q_kv_limit != nullptr;      // per-query key limits: every tile takes the masked path

  // ---- K/V tile staging (named registers + sched_barriers: hipcc otherwise spills the staging
  //      arrays to scratch and waits for the loads right where they are issued) -------------------------
  const int lrow = tid / C4, lc4 = tid % C4;   // RPP rows x C4 four-column chunks per pass, NP passes
  float4 rk0, rk1, rk2, rk3, rv0, rv1, rv2, rv3;
  rk0 = rv0 = rk1 = rk2 = rk3 = rv1 = rv2 = rv3 = make_float4(0.f, 0.f, 0.f, 0.f);
  // exact width: which of this thread's four columns the head has (the others stay zero in the tile)
  const bool has0 = 4 * lc4 + 0 < d_k, has1 = 4 * lc4 + 1 < d_k, has2 = 4 * lc4 + 2 < d_k, has3 = 4 * lc4 + 3 < d_k;
  // whether this thread has a row in staging pass i
#define PFHIP_STAGE_LIVE(i) (!kRagged || (lrow < RPP && lrow + RPP * (i) < kKT))
  const float* Kh = K + kbase * ldk + PFHIP_HCOL + 4 * lc4;
  const float* Vh = V + kbase * ldv + PFHIP_HCOL + 4 * lc4;
  // one row group (RPP keys) of the next K or V tile -> staging registers / staging registers -> LDS
#define PFHIP_ROW_LOAD(R, P, ld, i, kt)                                                 \
  do {                                                                                  \
    int key_ = (kt) * kKT + lrow + RPP * (i);                                           \
    key_ = key_ < Lk ? key_ : Lk - 1;                                                   \
    if (PFHIP_STAGE_LIVE(i)) {                                                          \
      const float* p_ = (P) + (size_t)key_ * (ld);                                      \
      if constexpr (kExact) {                                                           \
        R.x = has0 ? p_[0] : 0.f; R.y = has1 ? p_[1] : 0.f;                             \
        R.z = has2 ? p_[2] : 0.f; R.w = has3 ? p_[3] : 0.f;                             \
      } else {                                                                          \
        R = *reinterpret_cast<const float4*>(p_);                                       \
      }                                                                                 \
    }                                                                                   \
  } while (0)
#define PFHIP_K_LOAD(RK, i, kt) PFHIP_ROW_LOAD(RK, Kh, ldk, i, kt)
#define PFHIP_V_LOAD(RV, i, kt) PFHIP_ROW_LOAD(RV, Vh, ldv, i, kt)
#define PFHIP_K_STORE(RK, i, buf) \
  do { if (PFHIP_STAGE_LIVE(i)) *reinterpret_cast<float4*>(lds + (buf) * kKVBuf + (lrow + RPP * (i)) * kKS + 4 * lc4) = RK; } while (0)
#define PFHIP_V_STORE(RV, i, buf) \
  do { if (PFHIP_STAGE_LIVE(i)) *reinterpret_cast<float4*>(lds + (buf) * kKVBuf + kKT * kKS + (lrow + RPP * (i)) * HD + 4 * lc4) = RV; } while (0)

  f32x16 oacc0, oacc1, oacc2, oacc3;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    oacc0[e] = 0.f; oacc1[e] = 0.f;
    // d-tiles 2 and 3 are cleared together, and only in a form that has them: cleared where they are dead, or one by one, some
    // instantiation's score adds come out packed differently
    if (ND > 2) { oacc2[e] = 0.f; oacc3[e] = 0.f; }
  }
  float m_run = -1e30f, l_run = 0.f;

  const int nkt = (Lk + kKT - 1) / kKT;
  PFHIP_K_LOAD(rk0, 0, 0); PFHIP_V_LOAD(rv0, 0, 0);
  if (NP > 1) { PFHIP_K_LOAD(rk1, 1, 0); PFHIP_V_LOAD(rv1, 1, 0); }
  if (NP > 2) { PFHIP_K_LOAD(rk2, 2, 0); PFHIP_V_LOAD(rv2, 2, 0); }
  if (NP > 3) { PFHIP_K_LOAD(rk3, 3, 0); PFHIP_V_LOAD(rv3, 3, 0); }
  PFHIP_K_STORE(rk0, 0, 0); PFHIP_V_STORE(rv0, 0, 0);
  if (NP > 1) { PFHIP_K_STORE(rk1, 1, 0); PFHIP_V_STORE(rv1, 1, 0); }
  if (NP > 2) { PFHIP_K_STORE(rk2, 2, 0); PFHIP_V_STORE(rv2, 2, 0); }
  if (NP > 3) { PFHIP_K_STORE(rk3, 3, 0); PFHIP_V_STORE(rv3, 3, 0); }
  __syncthreads();

  // Memory instructions are issued singly between MFMA groups (the next tile's 2*NP global loads under the QK^T
  // MFMAs, its 2*NP LDS writes under the PV MFMAs): in bursts they starve the matrix pipe (see gemm.hip).
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
      if (NP > 2) {
        if (kb == 4) PFHIP_K_LOAD(rk2, 2, ktn);
        if (kb == 5) PFHIP_V_LOAD(rv2, 2, ktn);
      }
      if (NP > 3) {
        if (kb == 6) PFHIP_K_LOAD(rk3, 3, ktn);
        if (kb == 7) PFHIP_V_LOAD(rv3, 3, ktn);
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
        if (ND > 2) oacc2[e] *= alpha;
        if (ND > 3) oacc3[e] *= alpha;
      }
    }

    // O^T[d][q] += sum_key V[key][d] * P^T[key][q]; V values of step e+1 are read under the 4 MFMAs of e
    const float* vp = vs + (4 * h) * HD + r;
    // column of this lane in d-tile t, relative to r: 32 t in a full tile; in the partly live last one the lanes past the
    // (padded) width re-read its last column (their rows of O^T are dropped)
#define PFHIP_DCOL(t) (32 * (t) + 32 <= HD ? 32 * (t) : (32 * (t) + r < HD ? 32 * (t) + r : HD - 1) - r)
    const int c1 = PFHIP_DCOL(1), c2 = PFHIP_DCOL(2), c3 = PFHIP_DCOL(3);
#undef PFHIP_DCOL
    float va0 = vp[0], va1 = 0.f, va2 = 0.f, va3 = 0.f;
    if (ND > 1) va1 = vp[c1];
    if (ND > 2) va2 = vp[c2];
    if (ND > 3) va3 = vp[c3];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int en = e < 15 ? e + 1 : e;
      const float* vrow = vp + ((en & 3) + 8 * (en >> 2)) * HD;
      const float vn0 = vrow[0];
      float vn1 = 0.f, vn2 = 0.f, vn3 = 0.f;
      if (ND > 1) vn1 = vrow[c1];
      if (ND > 2) vn2 = vrow[c2];
      if (ND > 3) vn3 = vrow[c3];
      if (e == 0) PFHIP_K_STORE(rk0, 0, cur ^ 1);
      if (e == 1) PFHIP_V_STORE(rv0, 0, cur ^ 1);
      if (NP > 1) {
        if (e == 2) PFHIP_K_STORE(rk1, 1, cur ^ 1);
        if (e == 3) PFHIP_V_STORE(rv1, 1, cur ^ 1);
      }
      if (NP > 2) {
        if (e == 4) PFHIP_K_STORE(rk2, 2, cur ^ 1);
        if (e == 5) PFHIP_V_STORE(rv2, 2, cur ^ 1);
      }
      if (NP > 3) {
        if (e == 6) PFHIP_K_STORE(rk3, 3, cur ^ 1);
        if (e == 7) PFHIP_V_STORE(rv3, 3, cur ^ 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      const float pb = sacc[e];
      oacc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0, pb, oacc0, 0, 0, 0);
      if (ND > 1) oacc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1, pb, oacc1, 0, 0, 0);
      if (ND > 2) oacc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(va2, pb, oacc2, 0, 0, 0);
      if (ND > 3) oacc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(va3, pb, oacc3, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      va0 = vn0; va1 = vn1; va2 = vn2; va3 = vn3;
    }
    __syncthreads();
  }
#undef PFHIP_K_LOAD
#undef PFHIP_V_LOAD
#undef PFHIP_ROW_LOAD
#undef PFHIP_K_STORE
#undef PFHIP_V_STORE
#undef PFHIP_STAGE_LIVE

  // ---- normalise, transpose through LDS, store full rows (exact width: d_k floats per row) --------
  const float inv_l = 1.0f / l_run;
  float* os = lds + wave * (kQW * kKS);
#define PFHIP_O_STORE(OACC, dt)                                                          \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                        \
    float4 o4;                                                                           \
    o4.x = OACC[4 * g + 0] * inv_l; o4.y = OACC[4 * g + 1] * inv_l;                      \
    o4.z = OACC[4 * g + 2] * inv_l; o4.w = OACC[4 * g + 3] * inv_l;                      \
    /* registers 4g..4g+3 are d = dt*32 + 8g + 4h + (0..3) of query column r */          \
    if ((dt) * 32 + 8 * g + 8 <= HD)                                                     \
      *reinterpret_cast<float4*>(os + r * kKS + (dt) * 32 + 8 * g + 4 * h) = o4;         \
  }
  PFHIP_O_STORE(oacc0, 0)
  if (ND > 1) { PFHIP_O_STORE(oacc1, 1) }
  if (ND > 2) { PFHIP_O_STORE(oacc2, 2) }
  if (ND > 3) { PFHIP_O_STORE(oacc3, 3) }
#undef PFHIP_O_STORE
  __syncthreads();
  if constexpr (kExact) {
    // each wave stores its own 32 x d_k tile row by row: lane c of a row writes column c (d_k <= 64 lanes, one dword each)
    if (lane < d_k) {
      float* op = O + (qbase + q0 + wave * kQW) * ldo + PFHIP_HCOL + lane;
      const int rows = Lq - (q0 + wave * kQW) < kQW ? Lq - (q0 + wave * kQW) : kQW;      // <= 0: the wave has no live row
#pragma unroll 4
      for (int row = 0; row < rows; ++row) op[(size_t)row * ldo] = os[row * kKS + lane];
    }
  } else {
    // each wave stores its own 32 x HD tile as full rows: C4 lanes x float4 per row, 64/C4 rows per pass
    constexpr int RW = 64 / C4;
#pragma unroll
    for (int pass = 0; pass < (kQW + RW - 1) / RW; ++pass) {
      const int row = pass * RW + lane / C4, cc = lane % C4;
      const int qrow = q0 + wave * kQW + row;
      if (lane < RW * C4 && row < kQW && qrow < Lq) {
        const float4 o4 = *reinterpret_cast<const float4*>(os + row * kKS + 4 * cc);
        *reinterpret_cast<float4*>(O + (qbase + qrow) * ldo + PFHIP_HCOL + 4 * cc) = o4;
      }
    }
  }
#undef PFHIP_HCOL
}

}  // namespace

#define PFHIP_ATT(HD_, EXACT_)                                                                                                      \
  hipLaunchKernelGGL((attention_kernel<HD_, EXACT_>), grid, block, 0, s, o.Q, o.ldq, o.K, o.ldk, o.V, o.ldv, o.O, o.ldo, o.q_off, o.q_len, \
                     o.kv_off, o.kv_len, o.q_kv_limit, o.scale, o.head_dim)
// One launch of the fp32-MFMA kernel for the head widths it is built for; any other width is a programming error (the ABI and
// pfhip_create refuse it before a launch is reached)
static void launch_attention_f32(const AttnOp& o, hipStream_t s) {
  const dim3 grid(o.H, o.B, (o.max_q_len + kQB - 1) / kQB), block(256);
  if (o.head_dim == 32) PFHIP_ATT(32, false);
  else if (o.head_dim == 80) PFHIP_ATT(80, false);
  else if (o.head_dim == 128) PFHIP_ATT(128, false);
  else { fprintf(stderr, "pfhip: no attention kernel for head width %d\n", o.head_dim); abort(); }
}

// The exact-width form at the padded width that holds head_dim.  The caller (pfhip_punc_*, pfhip_op_attention_dk) has checked
// 1 <= head_dim <= 64 and the leading dimensions; a width outside the range here is a programming error, as above.
void launch_attention_dk(const AttnOp& o, hipStream_t s) {
  if (o.B <= 0 || o.max_q_len <= 0 || o.H <= 0) return;
  if (o.head_dim < 1 || o.head_dim > 64) { fprintf(stderr, "pfhip: no attention_dk kernel for head width %d\n", o.head_dim); abort(); }
  const dim3 grid(o.H, o.B, (o.max_q_len + kQB - 1) / kQB), block(256);
  if (o.head_dim <= 32) PFHIP_ATT(32, true);
  else if (o.head_dim <= 48) PFHIP_ATT(48, true);
  else PFHIP_ATT(64, true);
}
#undef PFHIP_ATT

// the split-operand attention: two fp16 planes / three products (attention_x3.hip, default) or three bf16 planes / six products
// (attention_x6.hip, PFHIP_ATT_X3=0)
static bool att_x3_on() {
  static const bool x3 = env_on("PFHIP_ATT_X3");
  return x3 && !launch_ctx().exact;
}
static void launch_attention_split(const AttnOp& op, hipStream_t s) {
  if (att_x3_on()) launch_attention_x3(op, s);
  else launch_attention_x6(op, s);
}

static bool att_x6_on() {
  static const bool x6 = env_on("PFHIP_ATT_X6");
  return x6;
}

// d_k = 80 has no fused memory block and no plane-image output: its encoder layers take launch_fsmn + the attention launch
bool attention_fsmn_is_fused(int max_len, int head_dim) {
  static const bool fuse = env_on("PFHIP_ATT_FSMN");
  return fuse && att_x6_on() && max_len > 64 && head_dim == kHeadDim;
}

bool attention_planes_ok(int max_len, int head_dim) { return attention_fsmn_is_fused(max_len, head_dim) && att_x3_on(); }

void launch_attention_fsmn(const AttnOp& op, hipStream_t s) {
  if (op.B <= 0 || op.max_q_len <= 0) return;
  if (attention_fsmn_is_fused(op.max_q_len, op.head_dim)) {
    launch_attention_split(op, s);
    return;
  }
  launch_fsmn(op.V, op.ldv, op.fsmn_w, nullptr, 0, op.mem, op.ldmem, op.q_off, op.q_len, op.B, op.max_q_len, op.H * op.head_dim, s);
  launch_attention(op, s);      // (which leaves the memory block and the plane images out: fp32 rows of context)
}

void launch_attention(const AttnOp& full, hipStream_t s) {
  if (full.B <= 0 || full.max_q_len <= 0) return;
  AttnOp op = full;      // plain attention on every kernel this may take: no memory block, no plane images
  op.fsmn_w = nullptr; op.mem = nullptr; op.ldmem = 0; op.mem_accumulate = false;
  op.planes_hi = op.planes_lo = nullptr; op.plane_rows = 0;
  const bool unmasked = op.q_kv_limit == nullptr;      // the per-query key limit lives in this file's fp32 kernel
  // d_k = 128 without per-query limits (encoder self-attention, decoder cross-attention): both products on the BF16 matrix
  // cores with the exact three-way split (attention_x6.hip) — 1.5 x this file's fp32-MFMA kernel.  PFHIP_ATT_X6=0 keeps fp32.
  if (unmasked && att_x6_on() && op.head_dim == 128 && op.max_q_len > 64) {      // streaming windows (20 queries) would leave 7 of its 8 waves idle
    launch_attention_split(op, s);
    return;
  }
  // d_k = 80 (the small Paraformer): the same switch at 64 queries onto the fp16 two-plane kernel of attention_h80.hip; the exact
  // re-run of the range guard (launch_ctx().exact: no fp16 planes) and PFHIP_ATT_X6=0 / PFHIP_ATT_X3=0 keep this file's fp32 kernel
  if (unmasked && att_x6_on() && att_x3_on() && op.head_dim == 80 && op.max_q_len > 64) {
    launch_attention_h80(op, s);
    return;
  }
  launch_attention_f32(op, s);
}

}  // namespace pfhip
