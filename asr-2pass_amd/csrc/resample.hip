// Windowed-sinc polyphase resampling ahead of the front end: the device half of Kaldi's LinearResample as the reference's
// Audio::WavResample runs it (onnxruntime/src/audio.cpp:259-284, resample.cpp:155-218, flush = true, fresh state per call).
// The plan (first index, tap count and weight row per output phase) is built on the host by resample.cpp.
//
// Each output sample is the reference's serial fp32 dot product in tap order, acc = acc + w[j] * x[idx], every multiply and
// add rounded on its own; taps whose input index falls outside [0, n) are skipped (the reference's edge branch,
// resample.cpp:187-205), so outputs are bitwise those of the CPU code.
//
// Shape: a workgroup owns a span of (up to 1024) consecutive output samples of one utterance; the (utterance, span) pairs of up to
// kMaxUtts utterances are flattened into one grid through a prefix table passed by value.  The workgroup stages the input
// window its span reads into LDS (16-byte loads where the window is 16-byte aligned in HBM), then each lane computes
// outputs from LDS with its phase's weight row, read from the plan table (a few KB to 1.5 MB: L2-resident), and stores
// them coalesced.  Outputs whose window is not wholly staged (utterance edges) read HBM directly.
//
// 16-bit PCM in: the same kernel with every load converted (float)s * (1.f / 32768.f) — exactly s / 32768.f — so the staged window
// and the tap loop hold the floats the f32 form would have read.  s16 windows are staged sample by sample, never through a wider
// cast (an utterance may start at an odd sample of a packed buffer: 2-byte alignment is all that is assumed).
#include <algorithm>
#include <type_traits>

#include "kernels.h"

namespace pfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxUtts = 64;                 // utterances per launch (the prefix table travels as a kernel argument)
constexpr int kMaxLds = 16384;               // floats of staged input per workgroup (64 KB)

struct ResampleBatch {
  int64_t in_off[kMaxUtts];
  int64_t out_off[kMaxUtts];
  int n_in[kMaxUtts];
  int n_out[kMaxUtts];
  int blk_off[kMaxUtts + 1];                 // first workgroup of each utterance; blk_off[nb] = grid size
  int nb;
  int span;                                  // output samples per workgroup (multiple of kThreads)
  int lds;                                   // staged floats per workgroup (0: no staging, every read from HBM)
  int vec;                                   // input base pointer is 16-byte aligned: stage with float4 loads (f32 input only)
};

__device__ __forceinline__ float load_sample(const float* in, int64_t e) { return in[e]; }
__device__ __forceinline__ float load_sample(const int16_t* in, int64_t e) { return (float)in[e] * (1.f / 32768.f); }

__device__ __forceinline__ int64_t first_in(const ResampleTable& t, int s, int* ph) {
  const int unit = s / t.Q;
  *ph = s - unit * t.Q;
  return (int64_t)t.first[*ph] + (int64_t)unit * t.P;
}

template <typename Sample>
__global__ __launch_bounds__(kThreads) void resample_kernel(const Sample* __restrict__ in, float* __restrict__ out,
                                                            const ResampleBatch a, const ResampleTable t) {
  extern __shared__ float4 win_raw[];                // 16-byte aligned for the float4 staging stores
  float* win = reinterpret_cast<float*>(win_raw);
  const int blk = blockIdx.x;
  int b = 0;
  while (b + 1 < a.nb && a.blk_off[b + 1] <= blk) ++b;
  const int s0 = (blk - a.blk_off[b]) * a.span;
  const int n = a.n_in[b];
  const int cnt = min(a.span, a.n_out[b] - s0);
  const int64_t base = a.in_off[b];
  const Sample* x = in + base;
  float* y = out + a.out_off[b] + s0;

  // input window [lo, hi) of this span, clamped to the utterance; staged as LDS[e - g0] for global element e = base + idx
  int ph0, ph1;
  const int64_t lo = max(first_in(t, s0, &ph0), (int64_t)0);
  const int64_t hi = min(first_in(t, s0 + cnt - 1, &ph1) + t.K, (int64_t)n);
  int64_t g0 = base + lo, g1 = base + hi;            // element range in `in`
  if (a.vec) { g0 &= ~(int64_t)3; g1 = (g1 + 3) & ~(int64_t)3; }
  const bool staged = hi > lo && g1 - g0 <= a.lds;
  if (staged) {
    const int64_t e0 = base + lo, e1 = base + hi;    // elements that may be read (inside this utterance)
    if constexpr (std::is_same<Sample, float>::value) {
      if (a.vec) {
        // 16-byte groups wholly inside [e0, e1); the partial groups at both ends element by element
        const int64_t v0 = (e0 + 3) & ~(int64_t)3, v1 = e1 & ~(int64_t)3;
        for (int64_t e = v0 + 4 * (int64_t)threadIdx.x; e < v1; e += 4 * kThreads)
          *reinterpret_cast<float4*>(win + (e - g0)) = *reinterpret_cast<const float4*>(in + e);
        const int64_t h1 = min(v0, e1);
        for (int64_t e = e0 + threadIdx.x; e < h1; e += kThreads) win[e - g0] = in[e];
        for (int64_t e = max(v1, h1) + threadIdx.x; e < e1; e += kThreads) win[e - g0] = in[e];
      } else {
        for (int64_t e = e0 + threadIdx.x; e < e1; e += kThreads) win[e - g0] = in[e];
      }
    } else {
      for (int64_t e = e0 + threadIdx.x; e < e1; e += kThreads) win[e - g0] = load_sample(in, e);
    }
  }
  __syncthreads();

  // x[idx] = win[idx - sh] for idx in [wlo, whi).  Only in-range LDS addresses are ever formed: a pointer before `win` would
  // wrap in the 32-bit LDS space and leave the shared aperture once converted to a flat address.
  const int64_t wlo = staged ? lo : 0, whi = staged ? hi : 0;
  const int64_t sh = g0 - base;
  for (int o = threadIdx.x; o < cnt; o += kThreads) {
    int ph;
    const int64_t f = first_in(t, s0 + o, &ph);
    const int nt = t.ntap[ph];
    const float* w = t.w + (size_t)ph * t.K;
    float acc = 0.0f;
    if (f >= wlo && f + nt <= whi) {                 // every tap inside the utterance and staged
      const float* xs = win + (f - sh);
      for (int j = 0; j < nt; ++j) acc = __fadd_rn(acc, __fmul_rn(w[j], xs[j]));
    } else {
      for (int j = 0; j < nt; ++j) {
        const int64_t idx = f + j;
        if (idx < 0 || idx >= n) continue;           // skipped, not added as zero (resample.cpp:187-205)
        float v;
        if (idx >= wlo && idx < whi) v = win[idx - sh];
        else if constexpr (std::is_same<Sample, float>::value) v = x[idx];
        else v = load_sample(x, idx);
        acc = __fadd_rn(acc, __fmul_rn(w[j], v));
      }
    }
    y[o] = acc;
  }
}

}  // namespace

namespace {
template <typename Sample>
void launch_resample_any(const Sample* in, const int64_t* in_off, const int* n_in, float* out, const int64_t* out_off, const int* n_out,
                         int B, const ResampleTable& t, hipStream_t s) {
  // span: 4 outputs per lane, fewer when the staged window would not fit (strong downsampling to a low rate)
  int span = 4 * kThreads;
  auto window = [&](int sp) { return (int)(((int64_t)(sp - 1) * t.P + t.Q - 1) / t.Q) + t.K + 2 + 8; };
  while (span > kThreads && window(span) > kMaxLds) span -= kThreads;
  const int lds = window(span) <= kMaxLds ? window(span) : 0;
  for (int u0 = 0; u0 < B; u0 += kMaxUtts) {
    ResampleBatch a{};
    a.nb = std::min(kMaxUtts, B - u0);
    a.span = span;
    a.lds = lds;
    a.vec = std::is_same<Sample, float>::value && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    int blocks = 0;
    for (int i = 0; i < a.nb; ++i) {
      a.in_off[i] = in_off[u0 + i];
      a.out_off[i] = out_off[u0 + i];
      a.n_in[i] = n_in[u0 + i];
      a.n_out[i] = n_out[u0 + i];
      a.blk_off[i] = blocks;
      blocks += (std::max(n_out[u0 + i], 0) + span - 1) / span;
    }
    a.blk_off[a.nb] = blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(resample_kernel<Sample>, dim3(blocks), dim3(kThreads), (size_t)lds * sizeof(float), s, in, out, a, t);
  }
}
}  // namespace

void launch_resample(const float* in, const int64_t* in_off, const int* n_in, float* out, const int64_t* out_off, const int* n_out,
                     int B, const ResampleTable& t, hipStream_t s) {
  launch_resample_any(in, in_off, n_in, out, out_off, n_out, B, t, s);
}
void launch_resample(const int16_t* in, const int64_t* in_off, const int* n_in, float* out, const int64_t* out_off, const int* n_out,
                     int B, const ResampleTable& t, hipStream_t s) {
  launch_resample_any(in, in_off, n_in, out, out_off, n_out, B, t, s);
}

}  // namespace pfhip
