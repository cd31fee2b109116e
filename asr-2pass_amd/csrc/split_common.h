// Device helpers shared by the split-operand kernels (gemm_x3.hip, gemm_x6.hip, gemm_p3.hip, attention_x3.hip, attention_p3.hip,
// attention_h80.hip; gemm.hip for the tile order): the fp16 two-plane split, the tile order, and the LayerNorm statistics
// hand-off.  Everything is force-inlined: a kernel that uses a helper compiles to what it did with its own copy.
#pragma once
#include "kernels.h"

namespace pfhip {

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using float2v = __attribute__((ext_vector_type(2))) float;

// ---- the fp16 two-plane split ---------------------------------------------------------------------------------------------------
// fp16 has 11 significand bits, so TWO planes carry 22-23 of fp32's 24:
//     x * S = x1 + x2 + e,   x1 = fp16_rtz(x * S),   x2 = fp16_rn(x * S - x1)   (the subtraction is exact in fp32),
//     |e| <= max(2^-22 |x1|, 2^-24)     (S a power of two; the second bound is fp16's subnormal spacing — the matrix cores keep
//                                        subnormal fp16 operands, tools/probe/f16_split_probe.hip)
// The round-toward-zero conversion of the high plane saturates instead of producing Inf; the low plane rounds to nearest
// (v_cvt_pk_f16_f32, one instruction per pair on gfx950): half the error of truncation and no bias, and it cannot overflow
// (|x - hi| < 2^-10 |hi|).  Range and the products kept: gemm_x3.hip.
//
// x - (float)h for the low / high half of a packed fp16 pair, ONE instruction each (v_fma_mix_f32 reads an fp16 source in
// place: fma(h, -1.0, x)); exact, because h has at most 11 of x's 24 significant bits and the same exponent or the one below
__device__ __forceinline__ float sub_lo(float x, unsigned h) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
  return r;
}
__device__ __forceinline__ float sub_hi(float x, unsigned h) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
  return r;
}
// a packed fp16 pair of the high plane (rtz) / of the low plane (rn of the two residuals)
__device__ __forceinline__ unsigned hi_pair(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b)); }
__device__ __forceinline__ unsigned lo_pair(float a, float b) {
  const float2v r = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(r, half2v));
}
// eight consecutive values -> 16 bytes of the hi plane and 16 bytes of the lo plane ...
__device__ __forceinline__ void split8(const float (&v)[8], uint4& hi, uint4& lo) {
  unsigned* hp = &hi.x;
  unsigned* lp = &lo.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hp[i] = hi_pair(v[2 * i], v[2 * i + 1]);
    lp[i] = lo_pair(sub_lo(v[2 * i], hp[i]), sub_hi(v[2 * i + 1], hp[i]));
  }
}
// ... or packed as MFMA operands (all four high pairs first: the order the attention kernels were scheduled with)
__device__ __forceinline__ void split8(const float (&v)[8], half8& p0, half8& p1) {
  uint4 a, b;
  a.x = hi_pair(v[0], v[1]); a.y = hi_pair(v[2], v[3]); a.z = hi_pair(v[4], v[5]); a.w = hi_pair(v[6], v[7]);
  b.x = lo_pair(sub_lo(v[0], a.x), sub_hi(v[1], a.x)); b.y = lo_pair(sub_lo(v[2], a.y), sub_hi(v[3], a.y));
  b.z = lo_pair(sub_lo(v[4], a.z), sub_hi(v[5], a.z)); b.w = lo_pair(sub_lo(v[6], a.w), sub_hi(v[7], a.w));
  p0 = __builtin_bit_cast(half8, a); p1 = __builtin_bit_cast(half8, b);
}

// ---- tile order -----------------------------------------------------------------------------------------------------------------
// XCD-aware tile order (cdna_hip_programming.md T1, bijective form): blocks that share an XCD (equal blockIdx % 8) walk a
// contiguous run of a linear tile order.  That order is column-GROUP major: group g = column tiles [g*gw, (g+1)*gw), inside
// a group row panel by row panel, n fastest — so the gw weight tiles of a group (<= 2 MiB, the host picks gw) stay in the
// XCD's 4 MB L2 while its row panels stream through, instead of the whole weight matrix being re-fetched for every
// handful of row panels.  Same time, 35-70 % less L2->fabric traffic on the wide GEMMs (tools/probe/gemm_sched.hip + PMC).
__device__ __forceinline__ void tile_of_block(int bid, int n_tiles, int tiles_n, int gw, int& tm, int& tn) {
  {
    const int q = n_tiles >> 3, r = n_tiles & 7, xcd = bid & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tiles_m = n_tiles / tiles_n, full = tiles_n / gw, span = tiles_m * gw;
  if (bid < full * span) {
    const int g = bid / span, j = bid - g * span;
    tm = j / gw; tn = g * gw + (j - tm * gw);
  } else {                                        // the last, narrower group
    const int j = bid - full * span, w = tiles_n - full * gw;
    tm = j / w; tn = full * gw + (j - tm * w);
  }
}

// ---- LayerNorm statistics hand-off ----------------------------------------------------------------------------------------------
// LayerNorm statistics of the rows a tile just finished, for the GEMM that consumes them (LN-on-load below): the 32 lanes
// that hold one row's 128 columns reduce (mean of the tile's columns, M2 = sum of squared deviations from THAT mean) and lane 0
// writes the pair to stats[row][tile column][2].  The consumer merges the tiles_n pairs of a row with Chan's formula — as
// accurate as a two-pass LayerNorm, no atomics, no ordering between tiles.
// sum over the 32 lanes of a half wave, result in every lane: four DPP steps inside the 16-lane rows (quad swaps, half-row
// mirror, row mirror — vector-ALU speed) and ONE cross-row shuffle; five ds_bpermute round trips per sum cost the epilogue
// ~2 us per tile
__device__ __forceinline__ float half_wave_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
  v += __shfl_xor(v, 16);
  return v;
}
__device__ __forceinline__ void tile_row_stats(const float4& v, int grow, int M, int tn, int tiles_n, int c4, float* __restrict__ stats) {
  const float sum = half_wave_sum((v.x + v.y) + (v.z + v.w));
  const float mean = sum * (1.0f / kTileN);
  const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
  const float q = half_wave_sum((a * a + b * b) + (c * c + d * d));
  if (c4 == 0 && grow < M) *reinterpret_cast<float2*>(stats + ((size_t)grow * tiles_n + tn) * 2) = make_float2(mean, q);
}

// the consumer's half.  Row statistics merged from the producer's per-tile pairs (Chan: n = 128 per tile) — one thread per row,
// at kernel start, parked in registers under the K-loop and published through LDS for the epilogue passes ...
// range_flag != nullptr (the forms on two fp16 planes): a row whose centred standard deviation lies outside [2^-8, 2^11], whose
// offset |mean| / std exceeds kLnOffsetMax (the fold below cancels: kernels.h) or whose statistics are not finite is outside the
// domain the fold on two fp16 planes of the raw residual stream covers at fp32 grade: the forward's range flag is raised
// (kernels.h LaunchCtx) and the host redoes the batch unfolded on the bf16 three-plane kernels, which pass nullptr.
__device__ __forceinline__ float2 ln_row_stats(const float* __restrict__ stats, int tiles, float eps, int row, int* range_flag) {
  const float* sp = stats + (size_t)row * tiles * 2;
  float msum = 0.f, m2 = 0.f;
  for (int t = 0; t < tiles; ++t) msum += sp[2 * t];
  const float mean = msum / (float)tiles;
  for (int t = 0; t < tiles; ++t) { const float dm = sp[2 * t] - mean; m2 += sp[2 * t + 1] + (float)kTileN * dm * dm; }
  const float rstd = 1.0f / sqrtf(m2 / (float)(tiles * kTileN) + eps);
  if (range_flag && ln_row_out_of_domain(mean, rstd)) atomicOr(range_flag, 2);
  return make_float2(mean, rstd);
}
// The same for T tiles (4: d_model = 512; 16: the decoder's LayerNorm over the 2048 hidden channels) from the row's 8 T bytes fetched as
// T / 2 16-byte loads — requested at kernel entry and first used behind the prologue's DMA issue.  The loop above fetches one value per
// trip with a wait in each: 2 T dependent round trips, 4,000 cycles (T = 4) in front of the first DMA of a 56,000-cycle workgroup
// (in-kernel stamps, tools/p3_stamps.py).  Same operations in the same order: bit-identical — it IS the loop above, run over the
// register copy (T is a compile-time constant: the loop unrolls and the copy never leaves its registers).
template <int T>
struct LnRaw { float4 v[T / 2]; };
template <int T>
__device__ __forceinline__ void ln_raw_load(LnRaw<T>& r, const float* __restrict__ stats, int row) {
  const float4* sp = reinterpret_cast<const float4*>(stats + (size_t)row * T * 2);
#pragma unroll
  for (int i = 0; i < T / 2; ++i) r.v[i] = sp[i];
}
template <int T>
__device__ __forceinline__ float2 ln_row_stats_raw(const LnRaw<T>& r, float eps, int* range_flag) {
  return ln_row_stats(reinterpret_cast<const float*>(r.v), T, eps, 0, range_flag);
}
// ... where v (four columns of x W'^T) becomes rstd * (v - mean * colsum)
__device__ __forceinline__ void ln_finish(float4& v, const float4& cs, float2 mr) {
  v.x = mr.y * (v.x - mr.x * cs.x); v.y = mr.y * (v.y - mr.x * cs.y);
  v.z = mr.y * (v.z - mr.x * cs.z); v.w = mr.y * (v.w - mr.x * cs.w);
}

}  // namespace pfhip
