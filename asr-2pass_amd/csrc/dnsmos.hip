// The DNSMOS networks' front ends and head (utils/dnsmos_local.py with utils/DNSMOS/sig_bak_ovr.onnx and model_v8.onnx); the
// convolutions between them are conv3x3.hip.
//
// logpow_spec — the primary net's graph up to its first Conv2D: the two Slices / Reshapes / Concat that frame the window (frame f =
//   samples [160 f, 160 f + 320)), the STFT written as two 1x1 Convs against the file's own kernels `time2freq/stft-real|imag/kernel:0`
//   [161][320], then Square, Square_1, Add, Sqrt, Pow(2), Max(floor, .), Log, Div: out[f][b] = log(max(floor, sqrt(re^2 + im^2)^2)) / denom.
//   fp32, fixed summation order: four accumulators over k mod 4, k ascending, combined as (a0 + a1) + (a2 + a3).  One thread per bin,
//   eight frames per workgroup; the weights are read as the transposed table [320][2][kBinStride] the host builds once
//   (dnsmos_stft_table), so a wave's weight load is contiguous.  s16 input stands for s / 32768.f, bit for bit.
//
// melspec_db — what dnsmos_local.py:30-34 computes outside the graph for model_v8.onnx: librosa.feature.melspectrogram(n_fft = 321,
//   hop 160, 120 mels) of the window's first 144000 samples, then (power_to_db(S, ref = max) + 40) / 40, transposed.  librosa is not
//   part of this tree: its defaults (periodic Hann window, centred frames with ZERO padding, Slaney mel scale and normalisation,
//   amin 1e-10, top_db 80) are RECALLED from librosa 0.10.0, not read from a file.  The 321-point transform is a [321 -> 161]
//   real / imaginary matrix product against a table the host builds in double with the window folded in.  Two kernels: the mel power
//   of every frame plus the window's maximum (an atomic maximum on the bits of a non-negative float), then the decibel map.
//
// globalmax_mlp — ReduceMax over H and W, then MatMul + Add (+ Relu) three times: one workgroup per window, fp32, k ascending.
#include "kernels.h"
#include "launch_common.h"

namespace pfhip {
namespace {

constexpr int kHop = 160, kFrame = 320, kBins = 161;
constexpr int kBinStride = kDnsmosBinStride;    // 168
constexpr int kFpb = 8;                         // frames per workgroup
constexpr int kFft = 321, kMels = 120, kMelWin = 144000;

__device__ inline float sample_f32(float v) { return v; }
__device__ inline float sample_f32(int16_t v) { return __fmul_rn((float)v, 1.0f / 32768.0f); }      // exact

// re / im of kFpb frames for bin b: smp holds the frames' samples (frame f starts at f * kHop), tab is [K][2][kBinStride]
template <int K>
__device__ __forceinline__ void dft_rows(const float* __restrict__ smp, const float* __restrict__ tab, int b, float (&re)[kFpb],
                                         float (&im)[kFpb]) {
  float ar[kFpb][4], ai[kFpb][4];
#pragma unroll
  for (int f = 0; f < kFpb; ++f)
#pragma unroll
    for (int j = 0; j < 4; ++j) { ar[f][j] = 0.f; ai[f][j] = 0.f; }
  for (int k0 = 0; k0 < K - 3; k0 += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float wr = tab[(size_t)(2 * (k0 + j)) * kBinStride + b], wi = tab[(size_t)(2 * (k0 + j) + 1) * kBinStride + b];
#pragma unroll
      for (int f = 0; f < kFpb; ++f) {
        const float v = smp[f * kHop + k0 + j];
        ar[f][j] = fmaf(v, wr, ar[f][j]);
        ai[f][j] = fmaf(v, wi, ai[f][j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < (K & 3); ++j) {           // the tail of a K that is no multiple of 4 (321: one term into accumulator 0)
    const int k = (K & ~3) + j;
    const float wr = tab[(size_t)(2 * k) * kBinStride + b], wi = tab[(size_t)(2 * k + 1) * kBinStride + b];
#pragma unroll
    for (int f = 0; f < kFpb; ++f) {
      const float v = smp[f * kHop + k];
      ar[f][j] = fmaf(v, wr, ar[f][j]);
      ai[f][j] = fmaf(v, wi, ai[f][j]);
    }
  }
#pragma unroll
  for (int f = 0; f < kFpb; ++f) {
    re[f] = (ar[f][0] + ar[f][1]) + (ar[f][2] + ar[f][3]);
    im[f] = (ai[f][0] + ai[f][1]) + (ai[f][2] + ai[f][3]);
  }
}

template <typename Sample>
__global__ __launch_bounds__(192) void dnsmos_logpow_kernel(const Sample* __restrict__ pcm, const int64_t* __restrict__ win_off,
                                                            const float* __restrict__ tab, int n_frames, float floor_v, float denom,
                                                            float* __restrict__ out) {
  __shared__ float smp[(kFpb + 1) * kHop];
  const int win = blockIdx.y, f0 = blockIdx.x * kFpb, tid = threadIdx.x;
  const int nf = min(kFpb, n_frames - f0);
  const int span = (nf + 1) * kHop;                           // samples of this block's frames: all inside the window
  const Sample* src = pcm + win_off[win] + (int64_t)f0 * kHop;
  for (int j = tid; j < (kFpb + 1) * kHop; j += 192) smp[j] = j < span ? sample_f32(src[j]) : 0.f;
  __syncthreads();
  if (tid >= kBins) return;
  float re[kFpb], im[kFpb];
  dft_rows<kFrame>(smp, tab, tid, re, im);
#pragma unroll
  for (int f = 0; f < kFpb; ++f)
    if (f < nf) {
      const float mag = sqrtf(re[f] * re[f] + im[f] * im[f]);
      out[((size_t)win * n_frames + f0 + f) * kBins + tid] = logf(fmaxf(floor_v, mag * mag)) / denom;
    }
}

// mel power of frames [f0, f0 + kFpb) of a window: frame t = samples [160 t - 160, 160 t + 161) of the window's first kMelWin samples,
// zeros outside them
template <typename Sample>
__global__ __launch_bounds__(192) void dnsmos_melpow_kernel(const Sample* __restrict__ pcm, const int64_t* __restrict__ win_off,
                                                            const float* __restrict__ tab, const float* __restrict__ melT, int n_frames,
                                                            float* __restrict__ melpow, unsigned* __restrict__ wmax) {
  constexpr int kSpan = (kFpb - 1) * kHop + kFft;             // 1441
  __shared__ float smp[kSpan + 3];
  __shared__ float pw[kFpb][kBinStride];
  __shared__ unsigned bmax;
  const int win = blockIdx.y, f0 = blockIdx.x * kFpb, tid = threadIdx.x;
  const int nf = min(kFpb, n_frames - f0);
  const Sample* src = pcm + win_off[win];
  const int s0 = f0 * kHop - kHop;                            // window sample of smp[0]
  for (int j = tid; j < kSpan + 3; j += 192) {
    const int g = s0 + j;
    smp[j] = (j < kSpan && g >= 0 && g < kMelWin) ? sample_f32(src[g]) : 0.f;
  }
  if (tid == 0) bmax = 0u;
  __syncthreads();
  if (tid < kBins) {
    float re[kFpb], im[kFpb];
    dft_rows<kFft>(smp, tab, tid, re, im);
#pragma unroll
    for (int f = 0; f < kFpb; ++f) pw[f][tid] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();
  if (tid < kMels) {
    // two accumulators over b mod 2, b ascending
    float a0[kFpb], a1[kFpb];
#pragma unroll
    for (int f = 0; f < kFpb; ++f) { a0[f] = 0.f; a1[f] = 0.f; }
    for (int b = 0; b < kBins - 1; b += 2) {
      const float w0 = melT[b * kMels + tid], w1 = melT[(b + 1) * kMels + tid];
#pragma unroll
      for (int f = 0; f < kFpb; ++f) { a0[f] = fmaf(pw[f][b], w0, a0[f]); a1[f] = fmaf(pw[f][b + 1], w1, a1[f]); }
    }
    const float wl = melT[(kBins - 1) * kMels + tid];
    float mx = 0.f;
#pragma unroll
    for (int f = 0; f < kFpb; ++f)
      if (f < nf) {
        const float v = fmaf(pw[f][kBins - 1], wl, a0[f]) + a1[f];       // >= 0: non-negative weights and powers
        melpow[((size_t)win * n_frames + f0 + f) * kMels + tid] = v;
        mx = fmaxf(mx, v);
      }
    atomicMax(&bmax, __float_as_uint(mx));                    // the bits of non-negative floats order as the floats
  }
  __syncthreads();
  if (tid == 0) atomicMax(wmax + win, bmax);
}

__global__ __launch_bounds__(256) void dnsmos_meldb_kernel(float* __restrict__ mel, const unsigned* __restrict__ wmax, int per_win,
                                                           long long total, float amin, float top_db) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float ref = __uint_as_float(wmax[i / per_win]);
  const float db = 10.0f * log10f(fmaxf(amin, mel[i])) - 10.0f * log10f(fmaxf(amin, ref));
  // power_to_db's floor is max(db) - top_db, and max(db) is the reference's own value minus itself: 0
  mel[i] = (fmaxf(db, -top_db) + 40.0f) / 40.0f;
}

// grid = windows; 256 threads: thread t reduces channel t % C over pixels t / C, t / C + 256 / C, ..
__global__ __launch_bounds__(256) void globalmax_mlp_kernel(const float* __restrict__ x, int HW, int C, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, int D1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, int D2, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, int D3, float* __restrict__ out) {
  __shared__ float part[256];
  __shared__ float va[256], vb[256];
  const int tid = threadIdx.x, win = blockIdx.x;
  const float* xw = x + (size_t)win * HW * C;
  const int groups = 256 / C, c = tid % C, g = tid / C;
  float m = -INFINITY;
  if (g < groups)
    for (int p = g; p < HW; p += groups) {
      const float v = xw[(size_t)p * C + c];
      m = (v > m || v != v) ? v : m;
    }
  part[tid] = m;
  __syncthreads();
  if (tid < C) {
    float r = part[tid];
    for (int j = 1; j < groups; ++j) {
      const float v = part[j * C + tid];
      r = (v > r || v != v) ? v : r;
    }
    va[tid] = r;
  }
  __syncthreads();
  if (tid < D1) {
    float s = 0.f;
    for (int k = 0; k < C; ++k) s = fmaf(va[k], w1[k * D1 + tid], s);
    s += b1[tid];
    vb[tid] = s < 0.f ? 0.f : s;
  }
  __syncthreads();
  if (tid < D2) {
    float s = 0.f;
    for (int k = 0; k < D1; ++k) s = fmaf(vb[k], w2[k * D2 + tid], s);
    s += b2[tid];
    va[tid] = s < 0.f ? 0.f : s;
  }
  __syncthreads();
  if (tid < D3) {
    float s = 0.f;
    for (int k = 0; k < D2; ++k) s = fmaf(va[k], w3[k * D3 + tid], s);
    out[(size_t)win * D3 + tid] = s + b3[tid];
  }
}

template <typename Sample>
bool logpow_launch(const Sample* pcm, const int64_t* win_off, int n_win, const float* tab, int n_frames, float floor_v, float denom,
                   float* out, hipStream_t s) {
  if (!pcm || !win_off || !tab || !out || n_win < 0 || n_win > 65535 || n_frames < 1 || !(denom != 0.f)) return false;
  if (n_win == 0) return true;
  hipLaunchKernelGGL(dnsmos_logpow_kernel<Sample>, dim3((unsigned)((n_frames + kFpb - 1) / kFpb), (unsigned)n_win), dim3(192), 0, s, pcm,
                     win_off, tab, n_frames, floor_v, denom, out);
  return true;
}

template <typename Sample>
bool melspec_launch(const Sample* pcm, const int64_t* win_off, int n_win, const float* tab, const float* melT, float* out, unsigned* wmax,
                    hipStream_t s) {
  if (!pcm || !win_off || !tab || !melT || !out || !wmax || n_win < 0 || n_win > 65535) return false;
  if (n_win == 0) return true;
  const int n_frames = kDnsmosMelFrames;
  if (hipMemsetAsync(wmax, 0, (size_t)n_win * sizeof(unsigned), s) != hipSuccess) return false;
  hipLaunchKernelGGL(dnsmos_melpow_kernel<Sample>, dim3((unsigned)((n_frames + kFpb - 1) / kFpb), (unsigned)n_win), dim3(192), 0, s, pcm,
                     win_off, tab, melT, n_frames, out, wmax);
  const int per_win = n_frames * kMels;
  const long long total = (long long)n_win * per_win;
  hipLaunchKernelGGL(dnsmos_meldb_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out, wmax, per_win, total, 1e-10f, 80.0f);
  return true;
}

}  // namespace

void dnsmos_stft_table(const float* wr, const float* wi, float* tab) {
  for (int k = 0; k < kFrame; ++k)
    for (int b = 0; b < kBinStride; ++b) {
      tab[(size_t)(2 * k) * kBinStride + b] = b < kBins ? wr[b * kFrame + k] : 0.f;
      tab[(size_t)(2 * k + 1) * kBinStride + b] = b < kBins ? wi[b * kFrame + k] : 0.f;
    }
}

// The mel front end's two tables, in double, rounded once (RECALLED librosa 0.10.0 defaults, see the head of this file):
//   tab [321][2][kBinStride]: hann_periodic(k) cos(2 pi k b / 321) and -hann_periodic(k) sin(2 pi k b / 321);
//   melT [161][120]: librosa.filters.mel(sr = 16000, n_fft = 321, n_mels = 120, fmin = 0, fmax = 8000, htk = False, norm = 'slaney'),
//   transposed.
void dnsmos_mel_tables(float* tab, float* melT) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < kFft; ++k) {
    const double w = 0.5 - 0.5 * cos(2.0 * pi * k / kFft);
    for (int b = 0; b < kBinStride; ++b) {
      // the angle reduced exactly: k b mod 321 keeps the argument below 2 pi
      const double ang = 2.0 * pi * (double)((k * b) % kFft) / kFft;
      tab[(size_t)(2 * k) * kBinStride + b] = b < kBins ? (float)(w * cos(ang)) : 0.f;
      tab[(size_t)(2 * k + 1) * kBinStride + b] = b < kBins ? (float)(-w * sin(ang)) : 0.f;
    }
  }
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp; };
  auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m; };
  double mel_f[kMels + 2];
  const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(8000.0);
  for (int i = 0; i < kMels + 2; ++i) mel_f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (kMels + 1));
  for (int i = 0; i < kMels; ++i) {
    const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int b = 0; b < kBins; ++b) {
      const double f = (double)b * 16000.0 / kFft;
      const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]), upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
      const double v = lower < upper ? lower : upper;
      melT[b * kMels + i] = (float)((v > 0.0 ? v : 0.0) * enorm);
    }
  }
}

bool launch_dnsmos_logpow(const float* pcm, const int64_t* win_off, int n_win, const float* tab, int n_frames, float floor_v, float denom,
                          float* out, hipStream_t s) {
  return logpow_launch(pcm, win_off, n_win, tab, n_frames, floor_v, denom, out, s);
}
bool launch_dnsmos_logpow(const int16_t* pcm, const int64_t* win_off, int n_win, const float* tab, int n_frames, float floor_v, float denom,
                          float* out, hipStream_t s) {
  return logpow_launch(pcm, win_off, n_win, tab, n_frames, floor_v, denom, out, s);
}
bool launch_dnsmos_melspec(const float* pcm, const int64_t* win_off, int n_win, const float* tab, const float* melT, float* out,
                           unsigned* wmax, hipStream_t s) {
  return melspec_launch(pcm, win_off, n_win, tab, melT, out, wmax, s);
}
bool launch_dnsmos_melspec(const int16_t* pcm, const int64_t* win_off, int n_win, const float* tab, const float* melT, float* out,
                           unsigned* wmax, hipStream_t s) {
  return melspec_launch(pcm, win_off, n_win, tab, melT, out, wmax, s);
}

bool launch_globalmax_mlp(const float* x, int N, int HW, int C, const float* w1, const float* b1, int D1, const float* w2, const float* b2,
                          int D2, const float* w3, const float* b3, int D3, float* out, hipStream_t s) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out || N < 0 || HW < 1 || C < 1 || C > 256 || D1 < 1 || D1 > 256 || D2 < 1 ||
      D2 > 256 || D3 < 1 || D3 > 256)
    return false;
  if (N == 0) return true;
  hipLaunchKernelGGL(globalmax_mlp_kernel, dim3((unsigned)N), dim3(256), 0, s, x, HW, C, w1, b1, D1, w2, b2, D2, w3, b3, D3, out);
  return true;
}

}  // namespace pfhip
