// Frame energies for the end-point detector's decibel track (E2EVadModel::ComputeDecibel, e2e-vad.h:437-452, restated in
// host/vad_segmenter.cpp AppendDecibel): e[f] = sum_{i < flen} x[f * fshift + i]^2 in ONE fp32 accumulator, i ascending, every
// product rounded to fp32 before it is added — bit for bit the host loop, so one lane owns a frame and nothing is reduced across
// lanes.  What is shared is the memory traffic: a workgroup (one wave) takes kFramesPerBlock consecutive frames of one utterance,
// brings their sample span into LDS with 16-byte loads (scalar up to the first 16-byte boundary and after the last whole vector:
// an s16 utterance may start at an odd sample, an f32 one at any float) and each lane then walks its own frame in LDS.
//
// LDS layout.  Lane t's frame starts at word t * fshift; with fshift = 160 that is bank 0 or 16 of the 32 banks a ds_read_b32
// resolves over (MI355X: bank = word mod 32, lanes in groups of 32), a 16-way conflict on every read.  Sample j is therefore kept
// at word j + j / fshift: lane t's i-th read is word t * (fshift + 1) + i + i / fshift, a lane stride of fshift + 1 — odd for an
// even fshift, so the 32 lanes of a group hit 32 banks.  An odd fshift is conflict-free as it is and gets no padding.
#include "kernels.h"
#include "launch_common.h"

namespace pfhip {
namespace {

constexpr int kFramesPerBlock = 64;

__device__ inline float sample_f32(float v) { return v; }
__device__ inline float sample_f32(int16_t v) { return __fmul_rn((float)v, 1.0f / 32768.0f); }      // exact

template <typename Sample, bool kPad>
__global__ __launch_bounds__(64) void frame_energy_kernel(const Sample* __restrict__ pcm, const int64_t* __restrict__ sample_off,
                                                          const int* __restrict__ frame_off, const int* __restrict__ nframes, int B,
                                                          int flen, int fshift, unsigned magic, float* __restrict__ e) {
  extern __shared__ float img[];
  // block k of the launch is block k' of utterance b: utterance b has ceil(nframes[b] / 64) blocks
  int k = blockIdx.x, b = 0;
  for (; b < B; ++b) {
    const int nb = (nframes[b] + kFramesPerBlock - 1) / kFramesPerBlock;
    if (k < nb) break;
    k -= nb;
  }
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int f0 = k * kFramesPerBlock;
  const int nfr = min(kFramesPerBlock, nframes[b] - f0);
  const int span = (nfr - 1) * fshift + flen;                 // samples of this block's frames: all inside the utterance
  const Sample* src = pcm + sample_off[b] + (int64_t)f0 * fshift;
  // magic = floor(2^32 / fshift) + 1: umulhi(j, magic) == j / fshift for j * fshift < 2^32 (the launcher checks the span)
  auto slot = [&](int j) -> int { return kPad ? j + (int)__umulhi((unsigned)j, magic) : j; };

  constexpr int V = 16 / (int)sizeof(Sample);                 // samples per 16-byte load
  const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15);
  const int head = min(span, (int)(((16u - mis) & 15u) / sizeof(Sample)));
  const int nvec = (span - head) / V;
  for (int j = lane; j < head; j += 64) img[slot(j)] = sample_f32(src[j]);
  for (int v = lane; v < nvec; v += 64) {
    const int j = head + v * V;
    const uint4 raw = *reinterpret_cast<const uint4*>(src + j);
    Sample x[V];
    __builtin_memcpy(x, &raw, 16);
#pragma unroll
    for (int u = 0; u < V; ++u) img[slot(j + u)] = sample_f32(x[u]);
  }
  for (int j = head + nvec * V + lane; j < span; j += 64) img[slot(j)] = sample_f32(src[j]);
  __syncthreads();

  if (lane >= nfr) return;
  const float* w = img + lane * (fshift + (kPad ? 1 : 0));
  float s = 0.0f;
  for (int i0 = 0, q = 0; i0 < flen; i0 += fshift, q += kPad ? 1 : 0) {
    const int i1 = min(i0 + fshift, flen);
#pragma unroll 8
    for (int i = i0; i < i1; ++i) {
      const float x = w[i + q];
      s = __fadd_rn(s, __fmul_rn(x, x));
    }
  }
  e[frame_off[b] + f0 + lane] = s;
}

template <typename Sample>
bool launch_energy(const Sample* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                   int flen, int fshift, float* e, hipStream_t s) {
  if (B < 0 || total_frames < 0 || flen < 1 || fshift < 1) return false;
  const long long span = (long long)(kFramesPerBlock - 1) * fshift + flen;
  // PFHIP_ENERGY_PAD=0: the row-major image (measurements only: same results, conflicting reads)
  const bool pad = fshift % 2 == 0 && env_on("PFHIP_ENERGY_PAD");
  const long long words = span + (pad ? span / fshift + 1 : 0);
  if (words * 4 > 64 * 1024 || span * fshift >= (1ll << 32)) return false;
  if (B == 0 || total_frames == 0) return true;
  const unsigned magic = (unsigned)((1ull << 32) / (unsigned)fshift + 1);      // fshift >= 2 where it is used
  const dim3 grid((unsigned)((total_frames + kFramesPerBlock - 1) / kFramesPerBlock + B));
  if (pad)
    hipLaunchKernelGGL((frame_energy_kernel<Sample, true>), grid, dim3(64), (size_t)words * 4, s, pcm, sample_off, frame_off, nframes, B,
                       flen, fshift, magic, e);
  else
    hipLaunchKernelGGL((frame_energy_kernel<Sample, false>), grid, dim3(64), (size_t)words * 4, s, pcm, sample_off, frame_off, nframes, B,
                       flen, fshift, magic, e);
  return true;
}

}  // namespace

bool launch_frame_energy(const float* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                         int flen, int fshift, float* e, hipStream_t s) {
  return launch_energy(pcm, sample_off, frame_off, nframes, B, total_frames, flen, fshift, e, s);
}
bool launch_frame_energy(const int16_t* pcm, const int64_t* sample_off, const int* frame_off, const int* nframes, int B, int total_frames,
                         int flen, int fshift, float* e, hipStream_t s) {
  return launch_energy(pcm, sample_off, frame_off, nframes, B, total_frames, flen, fshift, e, s);
}

}  // namespace pfhip
