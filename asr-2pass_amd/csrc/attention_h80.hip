// Fused attention for head width d_k = 80 (the small Paraformer: d_model 320, four heads), in the arithmetic class of
// attention_x3.hip: Q, K, V and the probabilities are staged as two fp16 planes (hi = fp16_rtz(x), lo = fp16_rn(x - hi)), three
// products per block on `v_mfma_f32_32x32x16_f16`, fp32 accumulation, flash-style online softmax, ragged segments through the same
// q_off / q_len / kv_off / kv_len interface.  Used for launches of more than 64 queries per utterance outside the exact launch
// context (attention.hip: launch_attention); the fp32-MFMA attention_kernel<80, false> serves the rest.
//
// One workgroup = 8 waves = 256 query rows of one (utterance, head); a wave keeps its 32 queries' Q planes in registers.  Per 32-key
// tile:
//   S^T = K Q^T    80 = 5 x 16: five k-steps x 3 plane products; A = K planes from LDS ([key][d] rows, ds_read_b128), B = Q planes.
//   O^T += V^T P^T  the output width 80 is no multiple of the 32-row MFMA tile.  V^T is PADDED TO 96 ROWS in LDS (rows 80..95 are
//                  zeroed once and never written again): three d-tiles x two k-steps x 3 products, 18 MFMAs of which 15 carry data.
//                  The alternative — 16-wide output tiles on the 16x16x32 shape — would have put the probabilities in a register
//                  layout that is not the one S^T leaves them in (the 32x32 score tile hands a lane pair a whole query's keys, and that
//                  IS the B operand of the 32x32 PV product), i.e. a cross-lane permutation of 16 values per tile on the softmax's
//                  critical path to save 3 of 33 MFMAs.
// LDS rows: a K-plane row is 80 fp16 = 40 dwords, padded to 44 (176 B).  ds_read_b128 is served in groups of 16 lanes whose rows r
// are distinct mod 16; each lane takes 4 consecutive banks starting at 44 r + c, and 44 r / 4 = 11 r runs through all residues mod 16
// (11 is odd), so the 16 lanes cover the 64 banks exactly once.  The unpadded stride 40 (10 r: even) would collide two-way.
// A V^T-plane row is 32 keys = 16 dwords padded to 18 (72 B), the stride attention_x3.hip uses: ds_read_b64 in groups of 32 lanes,
// 18 r mod 64 distinct even numbers for r < 32.
#include "kernels.h"
#include "launch_common.h"
#include "split_common.h"

#include <math.h>

namespace pfhip {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kHD = 80, kHDP = 96, kQW = 32, kNW = 8, kQB = kNW * kQW, kKT = 32;
constexpr int kKSteps = kHD / 16;                // 5 k-steps of the QK^T product
constexpr int kDT = kHDP / 32;                   // 3 d-tiles of the PV product
constexpr int kKRow = 176;                       // bytes per key row of a K plane (80 fp16 + 16 pad)
constexpr int kKPlane = kKT * kKRow;             // 5,632
constexpr int kVRow = 72;                        // bytes per d row of a V^T plane (32 keys fp16 + 8 pad)
constexpr int kVPlane = kHDP * kVRow;            // 6,912
constexpr int kBuf = 2 * kKPlane + 2 * kVPlane;  // 25,088
constexpr int kOS = kHD + 4;                     // floats per row of the output transpose tile
constexpr int kLdsBytes = kNW * kQW * kOS * 4;   // 86,016: the output transpose tile (>= 2 * kBuf = 50,176)
static_assert(kLdsBytes >= 2 * kBuf, "K/V buffers must fit");
constexpr int kKChunks = kKT * (kHD / 4);        // 640 float4 of a K tile: thread t takes chunk t, threads 384.. also chunk t + 128
constexpr int kVThreads = (kHD / 2) * (kKT / 4); // 320 threads take a 4-key x 2-d patch of the V tile each
static_assert(kKChunks == kNW * 64 + 128 && kVThreads == 5 * 64, "staging roles are whole waves");

// the fp16 two-plane primitives (sub_lo / sub_hi, hi_pair / lo_pair, split8): split_common.h
// 4 values -> 8 bytes of the high plane at base and of the low plane at base + plane_bytes
__device__ __forceinline__ void store4(float a, float c, float e, float g, unsigned char* base, int plane_bytes) {
  const unsigned h0 = hi_pair(a, c), h1 = hi_pair(e, g);
  *reinterpret_cast<uint2*>(base) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(base + plane_bytes) = make_uint2(lo_pair(sub_lo(a, h0), sub_hi(c, h0)), lo_pair(sub_lo(e, h1), sub_hi(g, h1)));
}

__global__ __launch_bounds__(512, 1) void attention_h80_kernel(
    const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk, const float* __restrict__ V, int ldv,
    float* __restrict__ O, int ldo, const int* __restrict__ q_off, const int* __restrict__ q_len,
    const int* __restrict__ kv_off, const int* __restrict__ kv_len, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int b = blockIdx.y, head = blockIdx.x;
  const int Lq = q_len[b];
  const int q0 = blockIdx.z * kQB;
  if (q0 >= Lq) return;
  const int Lk = kv_len[b];
  if (Lk <= 0) return;                               // no keys: nothing to attend to, and no row to clamp the tile loads to
  const size_t qbase = (size_t)q_off[b], kbase = (size_t)kv_off[b];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- the pad rows 80..95 of the four V^T planes (two buffers x hi / lo): zero, once ----------------------------------------
  {
    constexpr int kPadDwords = (kHDP - kHD) * kVRow / 4;      // 288 per plane
    for (int i = tid; i < 4 * kPadDwords; i += kNW * 64) {
      const int plane = i / kPadDwords, w = i % kPadDwords;
      unsigned char* base = lds + (plane >> 1) * kBuf + 2 * kKPlane + (plane & 1) * kVPlane + kHD * kVRow;
      reinterpret_cast<unsigned*>(base)[w] = 0u;
    }
  }

  // ---- Q planes of this lane: query row q0 + wave*32 + r, k-step s covers d = 16s + 8h + (0..7) ----------------------------
  half8 qf[kKSteps][2];
  {
    int qrow = q0 + wave * kQW + r;
    if (qrow >= Lq) qrow = Lq - 1;
    const float* qp = Q + (qbase + qrow) * ldq + head * kHD + 8 * h;
    const float qs = scale * 1.44269504088896340736f;          // scores come out in the base-2 softmax domain
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(qp + 16 * s);
      const float4 c = *reinterpret_cast<const float4*>(qp + 16 * s + 4);
      const float v[8] = {a.x * qs, a.y * qs, a.z * qs, a.w * qs, c.x * qs, c.y * qs, c.z * qs, c.w * qs};
      split8(v, qf[s][0], qf[s][1]);
    }
  }

  // ---- staging maps (512 threads; every role is wave-uniform) -----------------------------------------------------------------
  // K: 640 float4 per tile.  Thread t holds chunk t (key t / 20, d = 4 (t % 20)); waves 6 and 7 also hold chunk 128 + t.
  // V: waves 0..4 hold a patch of keys 4 (t / 40) + (0..3) x d = 2 (t % 40) + (0..1), transposed in registers on the way to LDS.
  const int kkey0 = tid / 20, kc0 = tid % 20;
  const bool k_second = tid >= 384;
  const int kkey1 = (tid + 128) / 20, kc1 = (tid + 128) % 20;       // chunks 512..639: keys 25..31
  const bool v_role = tid < kVThreads;
  const int vd2 = tid % 40, vkg = tid / 40;
  const float* Kh = K + kbase * ldk + head * kHD;
  const float* Vh = V + kbase * ldv + head * kHD + 2 * vd2;
  float4 rk0 = make_float4(0.f, 0.f, 0.f, 0.f), rk1 = rk0;
  float2 rv0 = make_float2(0.f, 0.f), rv1 = rv0, rv2 = rv0, rv3 = rv0;
  const int last = Lk - 1;
  auto load_tile = [&](int kt) {
    rk0 = *reinterpret_cast<const float4*>(Kh + (size_t)min(kt * kKT + kkey0, last) * ldk + 4 * kc0);
    if (k_second) rk1 = *reinterpret_cast<const float4*>(Kh + (size_t)min(kt * kKT + kkey1, last) * ldk + 4 * kc1);
    if (v_role) {
      const int k0 = kt * kKT + 4 * vkg;
      rv0 = *reinterpret_cast<const float2*>(Vh + (size_t)min(k0, last) * ldv);
      rv1 = *reinterpret_cast<const float2*>(Vh + (size_t)min(k0 + 1, last) * ldv);
      rv2 = *reinterpret_cast<const float2*>(Vh + (size_t)min(k0 + 2, last) * ldv);
      rv3 = *reinterpret_cast<const float2*>(Vh + (size_t)min(k0 + 3, last) * ldv);
    }
  };
  // the four pieces of a tile's split, placed one per k-step under the QK^T MFMAs of the tile before
  auto stage_piece = [&](int piece, int buf) {
    unsigned char* kb = lds + buf * kBuf;
    unsigned char* vb = kb + 2 * kKPlane + (2 * vd2) * kVRow + 8 * vkg;          // row d, keys 4 vkg .. + 3
    if (piece == 0) store4(rk0.x, rk0.y, rk0.z, rk0.w, kb + kkey0 * kKRow + 8 * kc0, kKPlane);
    if (piece == 1 && k_second) store4(rk1.x, rk1.y, rk1.z, rk1.w, kb + kkey1 * kKRow + 8 * kc1, kKPlane);
    if (piece == 2 && v_role) store4(rv0.x, rv1.x, rv2.x, rv3.x, vb, kVPlane);
    if (piece == 3 && v_role) store4(rv0.y, rv1.y, rv2.y, rv3.y, vb + kVRow, kVPlane);
  };

  f32x16 oacc[kDT];
#pragma unroll
  for (int dt = 0; dt < kDT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  const int nkt = (Lk + kKT - 1) / kKT;
  load_tile(0);
#pragma unroll
  for (int piece = 0; piece < 4; ++piece) stage_piece(piece, 0);
  load_tile(nkt > 1 ? 1 : 0);                          // raw registers run one tile ahead of the LDS buffers
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const unsigned char* kb = lds + cur * kBuf + r * kKRow + 16 * h;
    const unsigned char* vb = lds + cur * kBuf + 2 * kKPlane + r * kVRow + 8 * h;

    // S^T[key][q]: 5 k-steps x 3 plane products (k_lo q_hi, k_hi q_lo, k_hi q_hi); the K fragments of step s + 1 are requested before
    // the MFMAs of step s, and one piece of the next tile's split (4-6 VALU ops + LDS writes into the other buffer) rides under them
    f32x16 sacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#define PFHIP_KF(dst, p, s_) dst = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(kb + (p) * kKPlane + 32 * (s_)))
    half8 k0, k1, n0, n1;
    PFHIP_KF(k0, 0, 0); PFHIP_KF(k1, 1, 0);
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
      if (s + 1 < kKSteps) { PFHIP_KF(n0, 0, s + 1); PFHIP_KF(n1, 1, s + 1); }
      __builtin_amdgcn_sched_barrier(0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(k1, qf[s][0], sacc, 0, 0, 0);
      if (s < 4) stage_piece(s, cur ^ 1);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(k0, qf[s][1], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(k0, qf[s][0], sacc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      k0 = n0; k1 = n1;
    }
#undef PFHIP_KF
    load_tile(kt + 2 < nkt ? kt + 2 : nkt - 1);      // past the end: re-fetch the last tile (never used)
    __builtin_amdgcn_sched_barrier(0);

    // online softmax (base 2) for query column r; this lane holds keys (e&3) + 8*(e>>2) + 4*h of the tile
    float tmax = -INFINITY;
    if ((kt + 1) * kKT <= Lk) {
#pragma unroll
      for (int e = 0; e < 16; ++e) tmax = fmaxf(tmax, sacc[e]);
    } else {
      const int key0 = kt * kKT + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = key0 + (e & 3) + 8 * (e >> 2);
        const float sv = (key < Lk) ? sacc[e] : -INFINITY;
        sacc[e] = sv;
        tmax = fmaxf(tmax, sv);
      }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    // lazy rescale (attention_x3.hip): the reference m_run moves only when some query's maximum outgrew it by more than 2^10, so the
    // probabilities stay <= 2^10 (fp16's largest finite value is 65504) and most tiles skip the accumulator multiplies
    if (__any(tmax > m_run + 10.0f)) {
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < kDT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[dt][e] *= alpha;
    }
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pv = __builtin_amdgcn_exp2f(sacc[e] - m_run);
      sacc[e] = pv;
      psum += pv;
    }
    psum += __shfl_xor(psum, 32);
    l_run += psum;

    // O^T[d][q] += V^T P^T: two k-steps of 16 keys; k-slot i of step t is register e = 8t + i of the score tile, and the A operand
    // takes the same keys from the V^T planes (two ds_read_b64 per plane), so the key permutation cancels
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float pv[8] = {sacc[8 * t + 0], sacc[8 * t + 1], sacc[8 * t + 2], sacc[8 * t + 3],
                           sacc[8 * t + 4], sacc[8 * t + 5], sacc[8 * t + 6], sacc[8 * t + 7]};
      half8 p0, p1;
      split8(pv, p0, p1);
#pragma unroll
      for (int dt = 0; dt < kDT; ++dt) {
        const unsigned char* vp = vb + dt * 32 * kVRow + 32 * t;
        const uint2 a0 = *reinterpret_cast<const uint2*>(vp), a1 = *reinterpret_cast<const uint2*>(vp + 16);
        const uint2 c0 = *reinterpret_cast<const uint2*>(vp + kVPlane), c1 = *reinterpret_cast<const uint2*>(vp + kVPlane + 16);
        const half8 v0 = __builtin_bit_cast(half8, make_uint4(a0.x, a0.y, a1.x, a1.y));
        const half8 v1 = __builtin_bit_cast(half8, make_uint4(c0.x, c0.y, c1.x, c1.y));
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1, p0, oacc[dt], 0, 0, 0);
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, p1, oacc[dt], 0, 0, 0);
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, p0, oacc[dt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- normalise, transpose through LDS, store full 320-B rows --------------------------------------------------------------
  const float inv_l = 1.0f / l_run;
  float* os = reinterpret_cast<float*>(lds) + wave * (kQW * kOS);
#pragma unroll
  for (int dt = 0; dt < kDT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (dt * 32 + 8 * g + 8 <= kHD) {            // registers 4g..4g+3 are d = dt*32 + 8g + 4h + (0..3) of query column r
        float4 o4;
        o4.x = oacc[dt][4 * g + 0] * inv_l; o4.y = oacc[dt][4 * g + 1] * inv_l;
        o4.z = oacc[dt][4 * g + 2] * inv_l; o4.w = oacc[dt][4 * g + 3] * inv_l;
        *reinterpret_cast<float4*>(os + r * kOS + dt * 32 + 8 * g + 4 * h) = o4;
      }
    }
  __syncthreads();
  {
    constexpr int C4 = kHD / 4, RW = 64 / C4;      // 20 float4 per row, 3 rows per pass (lanes 60..63 idle)
#pragma unroll
    for (int pass = 0; pass < (kQW + RW - 1) / RW; ++pass) {
      const int row = pass * RW + lane / C4, cc = lane % C4;
      const int qrow = q0 + wave * kQW + row;
      if (lane < RW * C4 && row < kQW && qrow < Lq) {
        const float4 o4 = *reinterpret_cast<const float4*>(os + row * kOS + 4 * cc);
        *reinterpret_cast<float4*>(O + (qbase + qrow) * ldo + head * kHD + 4 * cc) = o4;
      }
    }
  }
}

}  // namespace

void launch_attention_h80(const AttnOp& o, hipStream_t s) {
  if (o.B <= 0 || o.max_q_len <= 0) return;
  const dim3 grid(o.H, o.B, (o.max_q_len + kQB - 1) / kQB);
  launch_with_lds<attention_h80_kernel>(grid, kLdsBytes, s, o.Q, o.ldq, o.K, o.ldk, o.V, o.ldv, o.O, o.ldo, o.q_off, o.q_len, o.kv_off,
                     o.kv_len, o.scale);
}

}  // namespace pfhip
