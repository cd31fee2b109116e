// fp32 GEMM on the gfx950 BF16 matrix cores: C = A * W^T (+bias, +residuals, ReLU), with fp32-grade results.
//
// On CDNA4 the fp32 MFMA (`v_mfma_f32_32x32x2_f32`) runs at the vector rate, 157 TFLOP/s — 1/16 of the BF16 MFMA
// (MI355X_MICROARCH.md § Matrix cores).  An fp32 number is EXACTLY the sum of three bf16 numbers (8 + 8 + 8 significand bits):
//     a = a1 + a2 + a3,  a1 = top 16 bits of a,  a2 = top 16 bits of (a - a1),  a3 = a - a1 - a2      (all subtractions exact)
// and a product of two bf16 numbers is exact in fp32, so
//     a*b = a1*b1 + (a1*b2 + a2*b1) + (a1*b3 + a3*b1 + a2*b2) + O(2^-24 |a*b|)
// costs six `v_mfma_f32_32x32x16_bf16` per 32x32x16 block instead of eight fp32 MFMAs of four times their duration: a ceiling of
// 2.5 PF / 6 = 417 TFLOP/s of fp32-equivalent work.  The three dropped terms are below fp32's own rounding of the product;
// accumulation is fp32 in the matrix core as before.  Measured against an fp64 reference the result is slightly CLOSER than
// the fp32 MFMA chain (rms 1.2e-7 vs 2.9e-7 relative at K = 512: the partial products carry no rounding of their own).
//
// Domain of the fp32-grade claim (pinned by tests/test_gpu_ops.py::test_gemm_bf16_split_stated_domain):
//   * non-finite operands: x = +-Inf gives a2 = Inf - Inf = NaN, so every output of that activation row (or weight column)
//     is NaN where an fp32 GEMM would carry +-Inf; a NaN operand gives NaN as it would there;
//   * magnitudes below 2^-110: the third plane is 2^-16 of the operand and falls into bf16's denormal range, which the matrix
//     cores flush: such operands keep ~16 significant bits.  Exact down to 2^-100.
// Neither occurs behind a LayerNorm with finite weights; callers with unbounded inputs should use the fp32-MFMA kernels
// (PFHIP_GEMM_X6=0).
//
// Tiling: 256 x 128 block tile, 8 waves as 4 x 2 (two per SIMD), each 64 x 64 = 2 x 2 MFMA tiles.  K-step 16 = one MFMA depth.
// Operands are split while they are staged: global fp32 -> registers -> three bf16 planes in LDS (row stride 48 B: the 16-lane
// groups of ds_read_b128 hit 16 distinct 16-B slots), double-buffered, one barrier per K-step; the split of the NEXT step's
// operands (5.5 VALU ops per element) and its LDS writes sit between this step's MFMAs, and the second wave of the SIMD fills
// what is left.  Per K-step a wave issues 12 ds_read_b128 for 24 MFMAs.
// Epilogue as in gemm.hip: accumulators transposed through LDS (two 128-row halves), rows written with 16-byte accesses.
#include "kernels.h"
#include "launch_common.h"
#include "split_common.h"

#include <algorithm>

namespace pfhip {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int kBM = 256, kBN = 128, kBK = 16;
constexpr int kRowB = 48;                                   // bytes per operand row in LDS (16 bf16 + pad)
constexpr int kPlaneA = kBM * kRowB, kPlaneW = kBN * kRowB; // bytes per plane
constexpr int kStageB = 3 * (kPlaneA + kPlaneW);            // 55,296 B
constexpr int kCs = kBN + 4;                                // padded C-tile row stride (floats)
constexpr int kLdsBytes = 2 * kStageB;                      // 110,592 B
static_assert(128 * kCs * 4 <= kLdsBytes, "half C tile must fit the operand buffers");

__device__ __forceinline__ unsigned top16_pair(float lo, float hi) {      // (bf16 trunc of hi) << 16 | (bf16 trunc of lo)
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
__device__ __forceinline__ float rest(float x) {                           // x - top16(x), exact
  return x - __uint_as_float(__float_as_uint(x) & 0xFFFF0000u);
}

// tile order, row statistics hand-off (tile_row_stats / ln_row_stats / ln_finish): split_common.h; the bf16 split is exact over
// fp32's whole range, so these kernels pass no range flag to ln_row_stats

__global__ __launch_bounds__(512, 1) void gemm_f32_bf16x6_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, float* C, int ldc,
    const float* __restrict__ bias, const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int tiles_n,
    int n_tiles, int gw, int relu, float* __restrict__ stats_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  int tm, tn;
  tile_of_block(blockIdx.x, n_tiles, tiles_n, gw, tm, tn);
  const int m0 = tm * kBM, n0 = tn * kBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  // staging map: thread t holds 4 consecutive k (one of the four 16-B pieces of a row's 64-B K-step) of A rows t/4 and
  // t/4 + 128 and of W row t/4: a wave's load instruction covers 16 rows x 64 contiguous bytes
  const int srow = tid >> 2, sq = tid & 3;
  const float* Ag0 = A + (size_t)min(m0 + srow, M - 1) * lda + 4 * sq;
  const float* Ag1 = A + (size_t)min(m0 + srow + 128, M - 1) * lda + 4 * sq;
  const float* Wg = W + (size_t)min(n0 + srow, N - 1) * ldw + 4 * sq;
  const int a_st = srow * kRowB + 8 * sq;                   // byte offset inside an A plane (second row: + 128 rows)
  const int w_st = 3 * kPlaneA + srow * kRowB + 8 * sq;     // byte offset of the W planes inside a stage
  const int a_fr = (wr * 64 + r) * kRowB + 16 * h;
  const int w_fr = 3 * kPlaneA + (wc * 64 + r) * kRowB + 16 * h;

  // two raw register sets: the global loads run two K-steps ahead of the split that consumes them
  float4 xa0, xa1, xw, ya0, ya1, yw;
#define PFHIP_LOAD_RAW(RA0, RA1, RW, k0)                       \
  RA0 = *reinterpret_cast<const float4*>(Ag0 + (k0));          \
  RA1 = *reinterpret_cast<const float4*>(Ag1 + (k0));          \
  RW = *reinterpret_cast<const float4*>(Wg + (k0));
  auto split3 = [&](const float4& v, unsigned char* base, int plane_bytes) {
    uint2 p;
    p.x = top16_pair(v.x, v.y); p.y = top16_pair(v.z, v.w);
    *reinterpret_cast<uint2*>(base) = p;
    float4 s = make_float4(rest(v.x), rest(v.y), rest(v.z), rest(v.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + plane_bytes) = p;
    s = make_float4(rest(s.x), rest(s.y), rest(s.z), rest(s.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + 2 * plane_bytes) = p;
  };
#define PFHIP_SPLIT_STORE(RA0, RA1, RW, stage)                                \
  split3(RA0, lds + (stage) * kStageB + a_st, kPlaneA);                       \
  split3(RA1, lds + (stage) * kStageB + a_st + 128 * kRowB, kPlaneA);         \
  split3(RW, lds + (stage) * kStageB + w_st, kPlaneW);

  f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc00[e] = 0.f; acc01[e] = 0.f; acc10[e] = 0.f; acc11[e] = 0.f; }

  // operand fragments: even K-steps in f*, odd in g* — [plane][tile]
  bf16x8 fa[3][2], fb[3][2], ga[3][2], gb[3][2];
#define PFHIP_FRAGS(FA, FB, stage)                                                                                  \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                 \
      FA[p][i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kStageB + p * kPlaneA + a_fr + i * 32 * kRowB)); \
      FB[p][i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kStageB + p * kPlaneW + w_fr + i * 32 * kRowB)); \
    }                                                                                                               \
  }
#define PFHIP_X6(FA, FB, pa, pb)                                                              \
  acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][0], FB[pb][0], acc00, 0, 0, 0);      \
  acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][0], FB[pb][1], acc01, 0, 0, 0);      \
  acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][1], FB[pb][0], acc10, 0, 0, 0);      \
  acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][1], FB[pb][1], acc11, 0, 0, 0);
#define PFHIP_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
  // The barrier is `s_waitcnt lgkmcnt(0); s_barrier` by hand: __syncthreads() also waits for vmcnt(0), i.e. for the global
  // loads issued a few instructions earlier — a full memory latency per K-step (measured: 1.16 us per step with it).
  // One K-step, one barrier.  Region 1: 16 MFMAs of this step, between them the split of the next step's operands (66 VALU
  // ops), its 6 LDS writes and the 3 global loads of the step after.  Barrier.  Region 2: the last 8 MFMAs, between them the
  // 12 fragment reads of the next step (into the other fragment set).  Masks: 0x8 MFMA, 0x2 VALU, 0x200 DS write,
  // 0x100 DS read, 0x20 VMEM read.
#define PFHIP_STEP(FA, FB, GA, GB, RA0, RA1, RW, nxt, knext)                                  \
  PFHIP_SPLIT_STORE(RA0, RA1, RW, nxt)                                                        \
  PFHIP_LOAD_RAW(RA0, RA1, RW, knext)                                                         \
  PFHIP_X6(FA, FB, 1, 1) PFHIP_X6(FA, FB, 0, 2) PFHIP_X6(FA, FB, 2, 0) PFHIP_X6(FA, FB, 0, 1)  \
  _Pragma("unroll") for (int q = 0; q < 9; ++q) {                                             \
    PFHIP_SGB(0x8, 1); PFHIP_SGB(0x2, 8); PFHIP_SGB(0x200, 1);                                \
  }                                                                                           \
  PFHIP_SGB(0x8, 1); PFHIP_SGB(0x20, 1); PFHIP_SGB(0x8, 1); PFHIP_SGB(0x20, 1);               \
  PFHIP_SGB(0x8, 1); PFHIP_SGB(0x20, 1); PFHIP_SGB(0x8, 4);                                   \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                              \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  PFHIP_FRAGS(GA, GB, nxt)                                                                    \
  PFHIP_X6(FA, FB, 1, 0) PFHIP_X6(FA, FB, 0, 0)                                               \
  _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                             \
    PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 2); PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 1);           \
  }                                                                                           \
  __builtin_amdgcn_sched_barrier(0);

  const int nk = K / kBK;
  auto kclamp = [&](int t) { return (t < nk ? t : nk - 1) * kBK; };
  PFHIP_LOAD_RAW(xa0, xa1, xw, 0)
  PFHIP_SPLIT_STORE(xa0, xa1, xw, 0)
  PFHIP_LOAD_RAW(ya0, ya1, yw, kclamp(1))                  // K-step 1 -> y, K-step 2 -> x: step kt splits set (kt + 1) & 1
  PFHIP_LOAD_RAW(xa0, xa1, xw, kclamp(2))
  __syncthreads();
  PFHIP_FRAGS(fa, fb, 0)

  // splits / loads past the last K-step redo the last one (never used): keeps the bodies straight-line
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    { const int knext = kclamp(kt + 3); PFHIP_STEP(fa, fb, ga, gb, ya0, ya1, yw, 1, knext) }
    { const int knext = kclamp(kt + 4); PFHIP_STEP(ga, gb, fa, fb, xa0, xa1, xw, 0, knext) }
  }
  if (kt < nk) { const int knext = kclamp(nk); PFHIP_STEP(fa, fb, ga, gb, ya0, ya1, yw, 1, knext) }
#undef PFHIP_STEP
#undef PFHIP_SPLIT_STORE
#undef PFHIP_LOAD_RAW
#undef PFHIP_SGB
#undef PFHIP_X6
#undef PFHIP_FRAGS
  // residual rows of the whole tile requested before the accumulators go through LDS: one memory latency for the epilogue
  // instead of one per pass
  const int c4 = tid & 31, rsub = tid >> 5;
  const int gcol = n0 + 4 * c4;
  float4 r1v[16];
#pragma unroll
  for (int pass = 0; pass < 16; ++pass) {
    const int grow = m0 + pass * 16 + rsub;
    r1v[pass] = (R1 && grow < M && gcol + 3 < N) ? *reinterpret_cast<const float4*>(R1 + (size_t)grow * ldr1 + gcol)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();                        // every wave has finished reading operand fragments

  // ---- epilogue: two 128-row halves through LDS (C/D map: col = lane&31, row = (e&3)+8*(e>>2)+4*(lane>>5)) ------------------
  float* const Cs = reinterpret_cast<float*>(lds);
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    if (gcol + 3 < N) bv = *reinterpret_cast<const float4*>(bias + gcol);
    else {
      if (gcol < N) bv.x = bias[gcol];
      if (gcol + 1 < N) bv.y = bias[gcol + 1];
      if (gcol + 2 < N) bv.z = bias[gcol + 2];
    }
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if ((wr >> 1) == half) {
      float* cw = Cs + ((wr & 1) * 64 + 4 * h) * kCs + wc * 64 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ro = ((e & 3) + 8 * (e >> 2)) * kCs;
        cw[ro] = acc00[e];
        cw[ro + 32] = acc01[e];
        cw[ro + 32 * kCs] = acc10[e];
        cw[ro + 32 * kCs + 32] = acc11[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
      const int row = pass * 16 + rsub;
      const int grow = m0 + half * 128 + row;
      float4 v = *reinterpret_cast<const float4*>(Cs + row * kCs + 4 * c4);
      v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
      if (grow < M && gcol + 3 < N) {
        if (R1) {
          const float4 t = r1v[half * 8 + pass];
          v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if (R2) {
          const float4 t = *reinterpret_cast<const float4*>(R2 + (size_t)grow * ldr2 + gcol);
          v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<float4*>(C + (size_t)grow * ldc + gcol) = v;
      } else if (grow < M && gcol < N) {      // ragged right edge: element-wise
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4 && gcol + q < N; ++q) {
          float o = vv[q];
          if (R1) o += R1[(size_t)grow * ldr1 + gcol + q];
          if (R2) o += R2[(size_t)grow * ldr2 + gcol + q];
          if (relu) o = fmaxf(o, 0.f);
          C[(size_t)grow * ldc + gcol + q] = o;
        }
      }
      if (stats_out) tile_row_stats(v, grow, M, tn, tiles_n, c4, stats_out);
    }
    __syncthreads();
  }
}

// ---- 128 x 128 sibling for grids that would not fill half a round of 256 x 128 tiles (decoder-side GEMMs over a few thousand
// token rows, batches of 4-8 utterances, rounds of streaming connections): 8 waves as 2 x 4, each 64 x 32 = 2 x 1 MFMA tiles,
// LDS 2 x 36,864 B so two blocks share a CU; same staging / split / pipelining scheme (per K-step and wave: 12 MFMAs, 44 VALU
// ops of splitting, 6 LDS writes, 2 global loads, 9 fragment reads).
constexpr int kSM = 128;
constexpr int kSPlane = kSM * kRowB;                        // 6,144 B per plane (A and W tiles have 128 rows each)
constexpr int kSStageB = 6 * kSPlane;                       // 36,864 B
constexpr int kSLdsBytes = 2 * kSStageB;                    // 73,728 B
static_assert(kSM * kCs * 4 <= kSLdsBytes, "C tile must fit the operand buffers");

template <bool LN>
__global__ __launch_bounds__(512, 2) void gemm_f32_bf16x6_128_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, float* C, int ldc,
    const float* __restrict__ bias, const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int tiles_n,
    int n_tiles, int gw, int relu, const float* __restrict__ ln_stats, int ln_tiles, float ln_eps, float* __restrict__ stats_out,
    const float* __restrict__ ln_colsum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  int tm, tn;
  tile_of_block(blockIdx.x, n_tiles, tiles_n, gw, tm, tn);
  const int m0 = tm * kSM, n0 = tn * kBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 31, h = lane >> 5;

  const int srow = tid >> 2, sq = tid & 3;
  const float* Ag = A + (size_t)min(m0 + srow, M - 1) * lda + 4 * sq;
  const float* Wg = W + (size_t)min(n0 + srow, N - 1) * ldw + 4 * sq;
  const int a_st = srow * kRowB + 8 * sq;
  const int w_st = 3 * kSPlane + a_st;
  const int a_fr = (wr * 64 + r) * kRowB + 16 * h;
  const int w_fr = 3 * kSPlane + (wc * 32 + r) * kRowB + 16 * h;

  // LayerNorm folded in (LN): the A operand is the RAW residual stream x; with gamma folded into the weights (W' = W gamma)
  //     LN(x) W^T = rstd_i * (x W'^T - mean_i * colsum(W')_n) + (bias + W beta)_n,
  // so the K-loop is the plain one and the normalisation is two FMAs per output element in the epilogue (mean_i / rstd_i merged
  // from the per-tile pairs the producing GEMM left, Chan's formula; colsum and the folded bias prepared at load).  The
  // subtraction amplifies the accumulation error by about sqrt(mean^2 + var) / std of the row — a small factor for a residual
  // stream — where normalising on load did not, but on-load cost the 4-waves-per-SIMD loop 4 % (8 VALU ops per K-step).
  float2 ln_mr = make_float2(0.f, 1.f);
  if (LN && tid < kSM) ln_mr = ln_row_stats(ln_stats, ln_tiles, ln_eps, min(m0 + tid, M - 1), nullptr);
  float4 xa, xw, ya, yw;
#define PFHIP_LOAD_RAW(RA, RW, k0)                            \
  RA = *reinterpret_cast<const float4*>(Ag + (k0));           \
  RW = *reinterpret_cast<const float4*>(Wg + (k0));
  auto split3 = [&](const float4& v, unsigned char* base) {
    uint2 p;
    p.x = top16_pair(v.x, v.y); p.y = top16_pair(v.z, v.w);
    *reinterpret_cast<uint2*>(base) = p;
    float4 s = make_float4(rest(v.x), rest(v.y), rest(v.z), rest(v.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + kSPlane) = p;
    s = make_float4(rest(s.x), rest(s.y), rest(s.z), rest(s.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + 2 * kSPlane) = p;
  };
#define PFHIP_SPLIT_STORE(RA, RW, stage)                      \
  split3(RA, lds + (stage) * kSStageB + a_st);                \
  split3(RW, lds + (stage) * kSStageB + w_st);

  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }

  bf16x8 fa[3][2], fb[3], ga[3][2], gb[3];
#define PFHIP_FRAGS(FA, FB, stage)                                                                                  \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                   \
    FA[p][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kSStageB + p * kSPlane + a_fr));               \
    FA[p][1] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kSStageB + p * kSPlane + a_fr + 32 * kRowB));  \
    FB[p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kSStageB + p * kSPlane + w_fr));                  \
  }
#define PFHIP_X6(FA, FB, pa, pb)                                                          \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][0], FB[pb], acc0, 0, 0, 0);       \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][1], FB[pb], acc1, 0, 0, 0);
#define PFHIP_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
#define PFHIP_STEP(FA, FB, GA, GB, RA, RW, nxt, knext)                                        \
  PFHIP_SPLIT_STORE(RA, RW, nxt)                                                              \
  PFHIP_LOAD_RAW(RA, RW, knext)                                                               \
  PFHIP_X6(FA, FB, 1, 1) PFHIP_X6(FA, FB, 0, 2) PFHIP_X6(FA, FB, 2, 0) PFHIP_X6(FA, FB, 0, 1)  \
  _Pragma("unroll") for (int q = 0; q < 6; ++q) {                                             \
    PFHIP_SGB(0x8, 1); PFHIP_SGB(0x2, 8); PFHIP_SGB(0x200, 1);                                \
  }                                                                                           \
  PFHIP_SGB(0x8, 1); PFHIP_SGB(0x20, 1); PFHIP_SGB(0x8, 1); PFHIP_SGB(0x20, 1);               \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                              \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  PFHIP_FRAGS(GA, GB, nxt)                                                                    \
  PFHIP_X6(FA, FB, 1, 0) PFHIP_X6(FA, FB, 0, 0)                                               \
  PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 3); PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 2);             \
  PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 2); PFHIP_SGB(0x8, 1); PFHIP_SGB(0x100, 2);             \
  __builtin_amdgcn_sched_barrier(0);

  const int nk = K / kBK;
  auto kclamp = [&](int t) { return (t < nk ? t : nk - 1) * kBK; };
  PFHIP_LOAD_RAW(xa, xw, 0)
  PFHIP_SPLIT_STORE(xa, xw, 0)
  PFHIP_LOAD_RAW(ya, yw, kclamp(1))
  PFHIP_LOAD_RAW(xa, xw, kclamp(2))
  __syncthreads();
  PFHIP_FRAGS(fa, fb, 0)
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    { const int knext = kclamp(kt + 3); PFHIP_STEP(fa, fb, ga, gb, ya, yw, 1, knext) }
    { const int knext = kclamp(kt + 4); PFHIP_STEP(ga, gb, fa, fb, xa, xw, 0, knext) }
  }
  if (kt < nk) { const int knext = kclamp(nk); PFHIP_STEP(fa, fb, ga, gb, ya, yw, 1, knext) }
#undef PFHIP_STEP
#undef PFHIP_SPLIT_STORE
#undef PFHIP_LOAD_RAW
#undef PFHIP_SGB
#undef PFHIP_X6
#undef PFHIP_FRAGS
  // residual rows of the whole tile requested before the accumulators go through LDS: one memory latency for the epilogue
  // instead of one per pass
  const int c4 = tid & 31, rsub = tid >> 5;
  const int gcol = n0 + 4 * c4;
  float4 r1v[8];
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int grow = m0 + pass * 16 + rsub;
    r1v[pass] = (R1 && grow < M && gcol + 3 < N) ? *reinterpret_cast<const float4*>(R1 + (size_t)grow * ldr1 + gcol)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  float* const Cs = reinterpret_cast<float*>(lds);
  {
    float* cw = Cs + (wr * 64 + 4 * h) * kCs + wc * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ro = ((e & 3) + 8 * (e >> 2)) * kCs;
      cw[ro] = acc0[e];
      cw[ro + 32 * kCs] = acc1[e];
    }
  }
  float2* const s_mr = reinterpret_cast<float2*>(lds + kSM * kCs * 4);          // behind the C tile: 128 x (mean, rstd)
  static_assert(kSM * kCs * 4 + kSM * 8 <= kSLdsBytes, "row statistics must fit behind the C tile");
  if (LN && tid < kSM) s_mr[tid] = ln_mr;
  __syncthreads();
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    if (gcol + 3 < N) bv = *reinterpret_cast<const float4*>(bias + gcol);
    else {
      if (gcol < N) bv.x = bias[gcol];
      if (gcol + 1 < N) bv.y = bias[gcol + 1];
      if (gcol + 2 < N) bv.z = bias[gcol + 2];
    }
  }
  float4 cs4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (LN && gcol + 3 < N) cs4 = *reinterpret_cast<const float4*>(ln_colsum + gcol);
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int row = pass * 16 + rsub;
    const int grow = m0 + row;
    float4 v = *reinterpret_cast<const float4*>(Cs + row * kCs + 4 * c4);
    if (LN) ln_finish(v, cs4, s_mr[row]);
    v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
    if (grow < M && gcol + 3 < N) {
      if (R1) {
        const float4 t = r1v[pass];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      if (R2) {
        const float4 t = *reinterpret_cast<const float4*>(R2 + (size_t)grow * ldr2 + gcol);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      *reinterpret_cast<float4*>(C + (size_t)grow * ldc + gcol) = v;
    } else if (grow < M && gcol < N) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int q = 0; q < 4 && gcol + q < N; ++q) {
        float o = vv[q];
        if (R1) o += R1[(size_t)grow * ldr1 + gcol + q];
        if (R2) o += R2[(size_t)grow * ldr2 + gcol + q];
        if (relu) o = fmaxf(o, 0.f);
        C[(size_t)grow * ldc + gcol + q] = o;
      }
    }
    if (stats_out) tile_row_stats(v, grow, M, tn, tiles_n, c4, stats_out);
  }
}


// ---- 64 x 128 sibling for grids between a quarter and three quarters of the chip's 512 workgroup slots — the decoder's
// N = 512 launches over ML ~ 7000 token rows are 220 tiles of 128 x 128: one workgroup on 220 CUs, nothing to overlap its
// prologue and epilogue with, 77 TF.  Half-height tiles double the count (two workgroups on most CUs).  8 waves as 2 x 4, each
// ONE 32 x 32 MFMA tile; A is staged by waves 0-3 (64 rows), W by all (128 rows); LDS 2 x 27,648 B.  Per K-step and wave:
// 6 MFMAs, 22-44 VALU ops of splitting, 3-6 LDS writes, 1-2 global loads, 6 fragment reads — more overhead per flop than the
// 128 x 128 tile, which stays the choice wherever its grid fills the slots.
constexpr int kHM = 64;
constexpr int kHPlaneA = kHM * kRowB;                       // 3,072 B
constexpr int kHPlaneW = kBN * kRowB;                       // 6,144 B
constexpr int kHStageB = 3 * (kHPlaneA + kHPlaneW);         // 27,648 B
constexpr int kHLdsBytes = 2 * kHStageB;                    // 55,296 B
static_assert(kHM * kCs * 4 <= kHLdsBytes, "C tile must fit the operand buffers");

template <bool LN>
__global__ __launch_bounds__(512, 2) void gemm_f32_bf16x6_64_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, float* C, int ldc,
    const float* __restrict__ bias, const float* R1, int ldr1, const float* R2, int ldr2, int M, int N, int K, int tiles_n,
    int n_tiles, int gw, int relu, const float* __restrict__ ln_stats, int ln_tiles, float ln_eps, float* __restrict__ stats_out,
    const float* __restrict__ ln_colsum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  int tm, tn;
  tile_of_block(blockIdx.x, n_tiles, tiles_n, gw, tm, tn);
  const int m0 = tm * kHM, n0 = tn * kBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 31, h = lane >> 5;

  const int srow = tid >> 2, sq = tid & 3;
  const bool stage_a = srow < kHM;                           // waves 0-3 (wave-uniform)
  const float* Ag = A + (size_t)min(m0 + (stage_a ? srow : 0), M - 1) * lda + 4 * sq;
  const float* Wg = W + (size_t)min(n0 + srow, N - 1) * ldw + 4 * sq;
  const int a_st = srow * kRowB + 8 * sq;
  const int w_st = 3 * kHPlaneA + srow * kRowB + 8 * sq;
  const int a_fr = (wr * 32 + r) * kRowB + 16 * h;
  const int w_fr = 3 * kHPlaneA + (wc * 32 + r) * kRowB + 16 * h;

  float2 ln_mr = make_float2(0.f, 1.f);
  if (LN && tid < kHM) ln_mr = ln_row_stats(ln_stats, ln_tiles, ln_eps, min(m0 + tid, M - 1), nullptr);
  float4 xa = make_float4(0.f, 0.f, 0.f, 0.f), xw, ya = xa, yw;
#define PFHIP_LOAD_RAW(RA, RW, k0)                                           \
  if (stage_a) RA = *reinterpret_cast<const float4*>(Ag + (k0));             \
  RW = *reinterpret_cast<const float4*>(Wg + (k0));
  auto split3 = [&](const float4& v, unsigned char* base, int plane_bytes) {
    uint2 p;
    p.x = top16_pair(v.x, v.y); p.y = top16_pair(v.z, v.w);
    *reinterpret_cast<uint2*>(base) = p;
    float4 s = make_float4(rest(v.x), rest(v.y), rest(v.z), rest(v.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + plane_bytes) = p;
    s = make_float4(rest(s.x), rest(s.y), rest(s.z), rest(s.w));
    p.x = top16_pair(s.x, s.y); p.y = top16_pair(s.z, s.w);
    *reinterpret_cast<uint2*>(base + 2 * plane_bytes) = p;
  };
#define PFHIP_SPLIT_STORE(RA, RW, stage)                                                              \
  if (stage_a) split3(RA, lds + (stage) * kHStageB + a_st, kHPlaneA);                                 \
  split3(RW, lds + (stage) * kHStageB + w_st, kHPlaneW);

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  bf16x8 fa[3], fb[3], ga[3], gb[3];
#define PFHIP_FRAGS(FA, FB, stage)                                                                                  \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                   \
    FA[p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kHStageB + p * kHPlaneA + a_fr)); \
    FB[p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + (stage) * kHStageB + p * kHPlaneW + w_fr)); \
  }
#define PFHIP_X6(FA, FB, pa, pb) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa], FB[pb], acc, 0, 0, 0);
#define PFHIP_STEP(FA, FB, GA, GB, RA, RW, nxt, knext)                                        \
  PFHIP_SPLIT_STORE(RA, RW, nxt)                                                              \
  PFHIP_LOAD_RAW(RA, RW, knext)                                                               \
  PFHIP_X6(FA, FB, 1, 1) PFHIP_X6(FA, FB, 0, 2) PFHIP_X6(FA, FB, 2, 0) PFHIP_X6(FA, FB, 0, 1)  \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                              \
  __builtin_amdgcn_sched_barrier(0);                                                          \
  PFHIP_FRAGS(GA, GB, nxt)                                                                    \
  PFHIP_X6(FA, FB, 1, 0) PFHIP_X6(FA, FB, 0, 0)                                               \
  __builtin_amdgcn_sched_barrier(0);

  const int nk = K / kBK;
  auto kclamp = [&](int t) { return (t < nk ? t : nk - 1) * kBK; };
  PFHIP_LOAD_RAW(xa, xw, 0)
  PFHIP_SPLIT_STORE(xa, xw, 0)
  PFHIP_LOAD_RAW(ya, yw, kclamp(1))
  PFHIP_LOAD_RAW(xa, xw, kclamp(2))
  __syncthreads();
  PFHIP_FRAGS(fa, fb, 0)
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    { const int knext = kclamp(kt + 3); PFHIP_STEP(fa, fb, ga, gb, ya, yw, 1, knext) }
    { const int knext = kclamp(kt + 4); PFHIP_STEP(ga, gb, fa, fb, xa, xw, 0, knext) }
  }
  if (kt < nk) { const int knext = kclamp(nk); PFHIP_STEP(fa, fb, ga, gb, ya, yw, 1, knext) }
#undef PFHIP_STEP
#undef PFHIP_SPLIT_STORE
#undef PFHIP_LOAD_RAW
#undef PFHIP_X6
#undef PFHIP_FRAGS
  // residual rows of the whole tile requested before the accumulators go through LDS: one memory latency for the epilogue
  // instead of one per pass
  const int c4 = tid & 31, rsub = tid >> 5;
  const int gcol = n0 + 4 * c4;
  float4 r1v[4];
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int grow = m0 + pass * 16 + rsub;
    r1v[pass] = (R1 && grow < M && gcol + 3 < N) ? *reinterpret_cast<const float4*>(R1 + (size_t)grow * ldr1 + gcol)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  float* const Cs = reinterpret_cast<float*>(lds);
  {
    float* cw = Cs + (wr * 32 + 4 * h) * kCs + wc * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) cw[((e & 3) + 8 * (e >> 2)) * kCs] = acc[e];
  }
  float2* const s_mr = reinterpret_cast<float2*>(lds + kHM * kCs * 4);
  static_assert(kHM * kCs * 4 + kHM * 8 <= kHLdsBytes, "row statistics must fit behind the C tile");
  if (LN && tid < kHM) s_mr[tid] = ln_mr;
  __syncthreads();
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    if (gcol + 3 < N) bv = *reinterpret_cast<const float4*>(bias + gcol);
    else {
      if (gcol < N) bv.x = bias[gcol];
      if (gcol + 1 < N) bv.y = bias[gcol + 1];
      if (gcol + 2 < N) bv.z = bias[gcol + 2];
    }
  }
  float4 cs4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (LN && gcol + 3 < N) cs4 = *reinterpret_cast<const float4*>(ln_colsum + gcol);
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int row = pass * 16 + rsub;
    const int grow = m0 + row;
    float4 v = *reinterpret_cast<const float4*>(Cs + row * kCs + 4 * c4);
    if (LN) ln_finish(v, cs4, s_mr[row]);
    v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
    if (grow < M && gcol + 3 < N) {
      if (R1) {
        const float4 t = r1v[pass];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      if (R2) {
        const float4 t = *reinterpret_cast<const float4*>(R2 + (size_t)grow * ldr2 + gcol);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
      if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      *reinterpret_cast<float4*>(C + (size_t)grow * ldc + gcol) = v;
    } else if (grow < M && gcol < N) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int q = 0; q < 4 && gcol + q < N; ++q) {
        float o = vv[q];
        if (R1) o += R1[(size_t)grow * ldr1 + gcol + q];
        if (R2) o += R2[(size_t)grow * ldr2 + gcol + q];
        if (relu) o = fmaxf(o, 0.f);
        C[(size_t)grow * ldc + gcol + q] = o;
      }
    }
    if (stats_out) tile_row_stats(v, grow, M, tn, tiles_n, c4, stats_out);
  }
}

}  // namespace

void launch_gemm_f32_bf16x6(const GemmOp& o, SplitTile tile, int gw, hipStream_t s) {
  if (o.M <= 0 || o.N <= 0) return;
  if (o.ln_stats && tile == SplitTile::Rows256) tile = SplitTile::Rows128;   // LayerNorm-on-load lives in the 128 / 64-row kernels (its consumers have K = 512)
  const int tm = tile == SplitTile::Rows64 ? kHM : (tile == SplitTile::Rows128 ? kSM : kBM);
  const int tiles_n = (o.N + kBN - 1) / kBN, n_tiles = ((o.M + tm - 1) / tm) * tiles_n, rl = o.relu ? 1 : 0;
  gw = std::max(1, std::min(gw, tiles_n));
  if (tile == SplitTile::Rows256) {
    launch_with_lds<gemm_f32_bf16x6_kernel>(n_tiles, kLdsBytes, s, o.A, o.lda, o.W, o.ldw, o.C, o.ldc, o.bias, o.R1, o.ldr1, o.R2, o.ldr2, o.M, o.N,
                                            o.K, tiles_n, n_tiles, gw, rl, o.stats_out);
    return;
  }
  // the 128- and 64-row kernels share one parameter list
#define PFHIP_X6_LAUNCH(KERN, LDS)                                                                                                      \
  launch_with_lds<KERN>(n_tiles, LDS, s, o.A, o.lda, o.W, o.ldw, o.C, o.ldc, o.bias, o.R1, o.ldr1, o.R2, o.ldr2, o.M, o.N, o.K, tiles_n, \
                        n_tiles, gw, rl, o.ln_stats, o.ln_tiles, 1e-12f, o.stats_out, o.ln_colsum)
  const bool ln = o.ln_stats != nullptr;
  if (tile == SplitTile::Rows64 && ln) PFHIP_X6_LAUNCH(gemm_f32_bf16x6_64_kernel<true>, kHLdsBytes);
  else if (tile == SplitTile::Rows64) PFHIP_X6_LAUNCH(gemm_f32_bf16x6_64_kernel<false>, kHLdsBytes);
  else if (ln) PFHIP_X6_LAUNCH(gemm_f32_bf16x6_128_kernel<true>, kSLdsBytes);
  else PFHIP_X6_LAUNCH(gemm_f32_bf16x6_128_kernel<false>, kSLdsBytes);
#undef PFHIP_X6_LAUNCH
}

}  // namespace pfhip
