// 3x3 convolution, pad 1, stride 1, + bias + ReLU (+ 2x2 floor max-pool) on NHWC fp32 activations: the Conv / Relu / MaxPool groups of
// the DNSMOS graphs (utils/DNSMOS/sig_bak_ovr.onnx: conv2d .. conv2d_6; model_v8.onnx: conv2d_5 .. conv2d_9).  With the channel axis
// innermost the convolution is a GEMM whose K axis is (tap, input channel): out[pixel][co] = sum_tap sum_ci x[pixel + tap][ci] w[co][ci][tap],
// and the graph's NCHW <-> NHWC Transposes have nothing left to do.
//
// Cin >= 32 (32 or a multiple of 64; Cout 32 or 64): an implicit GEMM on the fp16 matrix cores in the fp32-grade arithmetic of gemm_x3.hip —
// two fp16 planes per operand (split_common.h), three `v_mfma_f32_32x32x16_f16` per block, fp32 accumulation.
//   * A workgroup (4 waves) owns an 8 x 16 tile of output pixels of one image and every output channel: M = 128 pixels, N = Cout.
//     Wave w owns output rows 2 w and 2 w + 1 of the tile (32 pixels: one MFMA row block) and Cout / 32 column blocks.
//   * The tile's 10 x 18 halo of input pixels is split into its two planes and staged ONCE per 64 input channels in LDS; pixels
//     outside the image are staged as zeros, which is the convolution's zero padding — there is no padded copy.  The nine taps then
//     read the same image as shifted views: tap (ky, kx) of output pixel (py, px) is halo pixel (py + ky, px + kx).
//     A pixel's row in LDS is 2 CK + 16 bytes (CK channels of fp16 + 16 bytes of padding): 20 or 36 dwords, so the 16 pixels a
//     16-byte fragment read of a lane group covers start in 16 different groups of four banks.
//   * The weights arrive pre-split (launch_conv3x3_pack, once at load): per plane [tap][Cin / 16][Cout][16] fp16, times a power of
//     two S_w with max |w| S_w <= 32768 (kernels.h best_w_scale), so a lane's B fragment is 16 contiguous bytes and a wave's load one
//     contiguous KB.  The accumulator is multiplied by 1 / S_w (exact) in the epilogue.
//   * Epilogue: acc / S_w + bias, ReLU, through LDS (the staging space) so that rows leave as float4s; with `pool` a pooled pixel is
//     the maximum of its four tile pixels — tiles start on even rows and columns, so a pool window never straddles two tiles, and
//     for an odd H or W the last row or column belongs to no window and is dropped, as MaxPool's VALID floor does.
//   Range: activations are staged unscaled (|x| < 65504; the networks' are in [-12, 5]); the error is that of an fp32 chain over
//   9 Cin terms (gemm_x3.hip's argument; tests/test_gpu_dnsmos_ops.py pins it against fp64).
//
// Cin == 1 (the first layer of either network): nine FMAs per output in the fixed order ky, kx ascending, on the vector ALU.
#include "kernels.h"
#include "launch_common.h"
#include "split_common.h"

namespace pfhip {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kTH = 8, kTW = 16;                           // output tile
constexpr int kHH = kTH + 2, kHW = kTW + 2;                // halo
constexpr int kHalo = kHH * kHW;                           // 180 pixels
constexpr int kCKMax = 64;                                 // input channels staged at a time
constexpr int kLdsBytes = 2 * kHalo * (2 * kCKMax + 16);   // 51,840 B: two planes
static_assert(kTH * kTW * (64 + 4) * 4 <= kLdsBytes, "the output tile must fit the staging space");

// ReLU and max that keep a NaN (fmaxf would drop it)
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float max_keep_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// ONNX [Cout][Cin][3][3] fp32 -> per plane [tap][Cin / 16][Cout][16] fp16 of w * scale: one thread per 8 consecutive input channels
__global__ __launch_bounds__(256) void conv3x3_pack_kernel(const float* __restrict__ w, int Cin, int Cout, float scale,
                                                           uint4* __restrict__ hi, uint4* __restrict__ lo, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int h = i & 1, co = (i >> 1) % Cout, rest = (i >> 1) / Cout;
  const int kcs = Cin >> 4, kc = rest % kcs, tap = rest / kcs;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w[((size_t)co * Cin + 16 * kc + 8 * h + j) * 9 + tap] * scale;
  uint4 a, b;
  split8(v, a, b);
  hi[i] = a;
  lo[i] = b;
}

template <int NT>
__global__ __launch_bounds__(256) void conv3x3_f16x3_kernel(const float* __restrict__ x, const uint4* __restrict__ whi,
                                                            const uint4* __restrict__ wlo, const float* __restrict__ bias,
                                                            float* __restrict__ y, int H, int W, int Cin, int pool, float inv_sw) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  constexpr int Cout = 32 * NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n = blockIdx.z, y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
  const int CK = Cin < kCKMax ? Cin : kCKMax;               // 32 or 64
  const int qsh = CK == 64 ? 3 : 2;                         // 8-channel items per pixel: 1 << qsh
  const int pixb = 2 * CK + 16, plane = kHalo * pixb;
  const int ksteps = CK >> 4, kcs = Cin >> 4;
  const float* xn = x + (size_t)n * H * W * Cin;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int py = 2 * wave + (r >> 4), px = r & 15;          // this lane's A row: output pixel (py, px) of the tile

  for (int c0 = 0; c0 < Cin; c0 += CK) {
    if (c0) __syncthreads();
    for (int item = tid; item < (kHalo << qsh); item += 256) {
      const int p = item >> qsh, q = item - (p << qsh);
      const int hy = p / kHW, hx = p - hy * kHW;
      const int gy = y0 + hy - 1, gx = x0 + hx - 1;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
        const float4* src = reinterpret_cast<const float4*>(xn + ((size_t)gy * W + gx) * Cin + c0 + 8 * q);
        const float4 a = src[0], b = src[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
      }
      uint4 vh, vl;
      split8(v, vh, vl);
      *reinterpret_cast<uint4*>(lds + p * pixb + 16 * q) = vh;
      *reinterpret_cast<uint4*>(lds + plane + p * pixb + 16 * q) = vl;
    }
    __syncthreads();

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const unsigned char* ap = lds + ((py + ky) * kHW + px + kx) * pixb + 16 * h;
      const size_t wb = ((size_t)(tap * kcs + (c0 >> 4)) * Cout + r) * 2 + h;
      for (int ks = 0; ks < ksteps; ++ks) {
        const half8 ah = *reinterpret_cast<const half8*>(ap + 32 * ks);
        const half8 al = *reinterpret_cast<const half8*>(ap + plane + 32 * ks);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const size_t wi = wb + ((size_t)ks * Cout + 32 * t) * 2;
          const half8 bh = __builtin_bit_cast(half8, whi[wi]);
          const half8 bl = __builtin_bit_cast(half8, wlo[wi]);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
        }
      }
    }
  }

  // the tile as [pixel][Cout + 4] fp32 in the staging space
  __syncthreads();
  constexpr int kSt = Cout + 4, C4 = Cout / 4;
  float* st = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 32 * t + r;
    const float b = bias[c];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      st[m * kSt + c] = relu_keep_nan(acc[t][e] * inv_sw + b);
    }
  }
  __syncthreads();

  if (!pool) {
    float* yn = y + (size_t)n * H * W * Cout;
    for (int idx = tid; idx < kTH * kTW * C4; idx += 256) {
      const int m = idx / C4, c4 = idx - m * C4;
      const int gy = y0 + (m >> 4), gx = x0 + (m & 15);
      if (gy < H && gx < W)
        *reinterpret_cast<float4*>(yn + ((size_t)gy * W + gx) * Cout + 4 * c4) = *reinterpret_cast<const float4*>(st + m * kSt + 4 * c4);
    }
  } else {
    const int Hp = H >> 1, Wp = W >> 1;
    float* yn = y + (size_t)n * Hp * Wp * Cout;
    for (int idx = tid; idx < (kTH / 2) * (kTW / 2) * C4; idx += 256) {
      const int pp = idx / C4, c4 = idx - pp * C4;
      const int pi = pp >> 3, pj = pp & 7;
      const int gy = (y0 >> 1) + pi, gx = (x0 >> 1) + pj;
      if (gy < Hp && gx < Wp) {
        const float* s0 = st + (2 * pi * kTW + 2 * pj) * kSt + 4 * c4;
        const float4 a = *reinterpret_cast<const float4*>(s0), b = *reinterpret_cast<const float4*>(s0 + kSt);
        const float4 c = *reinterpret_cast<const float4*>(s0 + kTW * kSt), d = *reinterpret_cast<const float4*>(s0 + (kTW + 1) * kSt);
        float4 o;
        o.x = max_keep_nan(max_keep_nan(a.x, b.x), max_keep_nan(c.x, d.x));
        o.y = max_keep_nan(max_keep_nan(a.y, b.y), max_keep_nan(c.y, d.y));
        o.z = max_keep_nan(max_keep_nan(a.z, b.z), max_keep_nan(c.z, d.z));
        o.w = max_keep_nan(max_keep_nan(a.w, b.w), max_keep_nan(c.w, d.w));
        *reinterpret_cast<float4*>(yn + ((size_t)gy * Wp + gx) * Cout + 4 * c4) = o;
      }
    }
  }
}

// Cin == 1: one thread per output value (channel fastest), 1 or 4 convolution positions of nine FMAs each
__global__ __launch_bounds__(256) void conv3x3_c1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int H, int W, int Cout,
                                                         int Ho, int Wo, int pool, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % Cout);
  const long long pix = i / Cout;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const long long n = pix / ((long long)Wo * Ho);
  const float* xn = x + n * H * W;
  float k[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) k[t] = w[co * 9 + t];
  const float b = bias[co];
  const int np = pool ? 2 : 1;
  float best = 0.f;
  for (int a = 0; a < np; ++a)
    for (int c = 0; c < np; ++c) {
      const int cy = oy * np + a, cx = ox * np + c;
      float s = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int gy = cy + ky - 1, gx = cx + kx - 1;
          const float v = ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? xn[(size_t)gy * W + gx] : 0.f;
          s = fmaf(v, k[3 * ky + kx], s);
        }
      s = relu_keep_nan(s + b);
      best = (a | c) ? max_keep_nan(best, s) : s;
    }
  y[i] = best;
}

}  // namespace

size_t conv3x3_plane_bytes(int Cin, int Cout) { return (size_t)9 * Cin * Cout * 2; }

// the channel counts the matrix-core kernel takes: the halo is staged min(Cin, 64) channels at a time, and Cin must be whole stages
static bool conv3x3_shape_ok(int Cin, int Cout) { return (Cin == 32 || (Cin >= 64 && Cin % 64 == 0 && Cin <= 4096)) && (Cout == 32 || Cout == 64); }

bool launch_conv3x3_pack(const float* w, int Cin, int Cout, float scale, void* hi, void* lo, hipStream_t s) {
  if (!w || !hi || !lo || !conv3x3_shape_ok(Cin, Cout) || !(scale > 0.f)) return false;
  const int total = 9 * (Cin / 16) * Cout * 2;
  hipLaunchKernelGGL(conv3x3_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w, Cin, Cout, scale, static_cast<uint4*>(hi),
                     static_cast<uint4*>(lo), total);
  return true;
}

bool launch_conv3x3_relu(const float* x, const void* whi, const void* wlo, float w_scale, const float* bias, float* y, int N, int H, int W,
                         int Cin, int Cout, bool pool, hipStream_t s) {
  if (!x || !whi || !wlo || !bias || !y || N < 0 || N > 65535 || H < 1 || W < 1 || !conv3x3_shape_ok(Cin, Cout) || !(w_scale > 0.f))
    return false;
  if ((long long)H * W >= (1ll << 31) / 256) return false;
  if (N == 0 || (pool && (H < 2 || W < 2))) return true;
  const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), (unsigned)N);
  if (grid.y > 65535) return false;
  const uint4* a = static_cast<const uint4*>(whi);
  const uint4* b = static_cast<const uint4*>(wlo);
  if (Cout == 32)
    hipLaunchKernelGGL(conv3x3_f16x3_kernel<1>, grid, dim3(256), 0, s, x, a, b, bias, y, H, W, Cin, pool ? 1 : 0, 1.0f / w_scale);
  else
    hipLaunchKernelGGL(conv3x3_f16x3_kernel<2>, grid, dim3(256), 0, s, x, a, b, bias, y, H, W, Cin, pool ? 1 : 0, 1.0f / w_scale);
  return true;
}

bool launch_conv3x3_c1_relu(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout, bool pool,
                            hipStream_t s) {
  if (!x || !w || !bias || !y || N < 0 || H < 1 || W < 1 || Cout < 1) return false;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const long long total = (long long)N * Ho * Wo * Cout;
  if (total == 0) return true;
  const long long blocks = (total + 255) / 256;
  if (blocks >= (1ll << 31)) return false;
  hipLaunchKernelGGL(conv3x3_c1_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, w, bias, y, H, W, Cout, Ho, Wo, pool ? 1 : 0, total);
  return true;
}

}  // namespace pfhip
