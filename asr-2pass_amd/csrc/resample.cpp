// Host half of the resampling ahead of the front end: the polyphase plan of Kaldi's LinearResample as the reference's
// Audio::WavResample builds it (onnxruntime/src/audio.cpp:259-284: cutoff 0.99 * 0.5 * min(fs_in, fs_out), 6 zero crossings,
// flush = true), its per-device upload cache, and the host-only / operator-level C entries.
//
// Bit-exactness rests on the reference's precision choices, restated here: the cutoff is a float; the filter function takes a
// float t, evaluates window and sinc in double through libm cos / sin, rounds each to float and returns their float product;
// each weight is that product divided by the input rate in float (resample.cpp:104-153).  Built with -ffp-contract=off.
#include <climits>
#include <cmath>
#include <cstdint>

#include "internal.h"
#include "../../include/pfhip_ops.h"

namespace pfhip_impl {
namespace {

constexpr int kMinRate = 1000, kMaxRate = 192000, kZeros = 6;
constexpr double kTwoPi = 6.283185307179586476925286766559005;
constexpr double kPi = 3.1415926535897932384626433832795;

int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t r = a % b; a = b; b = r; }
  return a;
}

float cutoff_of(int fs_in, int fs_out) {
  const float min_freq = (float)std::min(fs_in, fs_out);
  return (float)(0.99 * 0.5 * min_freq);
}

// the windowed sinc h(t) = f(t) g(t) at a float offset t (seconds) from the filter centre
float filter_at(float t, float cutoff) {
  float window, filter;
  if (std::fabs(t) < kZeros / (2.0 * cutoff))
    window = (float)(0.5 * (1 + std::cos(kTwoPi * cutoff / kZeros * t)));
  else
    window = 0.0f;
  if (t != 0)
    filter = (float)(std::sin(kTwoPi * cutoff * t) / (kPi * t));
  else
    filter = 2 * cutoff;
  return filter * window;
}

}  // namespace

bool resample_supported(int fs_in, int fs_out, std::string* why) {
  char buf[160];
  if (fs_in < kMinRate || fs_in > kMaxRate || fs_out < kMinRate || fs_out > kMaxRate) {
    std::snprintf(buf, sizeof buf, "sample rate %d -> %d: rates must lie in [%d, %d] Hz", fs_in, fs_out, kMinRate, kMaxRate);
    if (why) *why = buf;
    return false;
  }
  const int64_t lcm = (int64_t)fs_in / gcd64(fs_in, fs_out) * fs_out;
  if (lcm > INT32_MAX) {        // the tick arithmetic of LinearResample::GetNumOutputSamples is int32 (resample.cpp:220-265)
    std::snprintf(buf, sizeof buf, "sample rate %d -> %d: lcm %lld exceeds int32", fs_in, fs_out, (long long)lcm);
    if (why) *why = buf;
    return false;
  }
  return true;
}

int64_t resample_out_len(int fs_in, int fs_out, int64_t n_in) {
  if (!resample_supported(fs_in, fs_out, nullptr) || n_in < 0) return -1;
  if (fs_in == fs_out) return n_in;
  // flush-mode count in ticks of 1 / lcm (GetNumOutputSamples, resample.cpp:220-265)
  const int64_t tick = (int64_t)fs_in / gcd64(fs_in, fs_out) * fs_out;
  const int64_t interval = n_in * (tick / fs_in);
  if (interval <= 0) return 0;
  const int64_t per_out = tick / fs_out;
  int64_t last = interval / per_out;
  if (last * per_out == interval) --last;
  return last + 1;
}

void build_resample_plan(int fs_in, int fs_out, ResamplePlan* p) {
  const int base = (int)gcd64(fs_in, fs_out);
  p->P = fs_in / base;
  p->Q = fs_out / base;
  const float cutoff = cutoff_of(fs_in, fs_out);
  const double window_width = kZeros / (2.0 * cutoff);
  p->first.assign(p->Q, 0);
  p->ntap.assign(p->Q, 0);
  std::vector<std::vector<float>> rows(p->Q);
  p->K = 0;
  // SetIndexesAndWeights (resample.cpp:104-136): ceil on the window's start, floor on its end
  for (int i = 0; i < p->Q; ++i) {
    const double out_t = i / static_cast<double>(fs_out);
    const double min_t = out_t - window_width, max_t = out_t + window_width;
    const int32_t lo = (int32_t)std::ceil(min_t * fs_in), hi = (int32_t)std::floor(max_t * fs_in);
    const int32_t nt = hi - lo + 1;
    p->first[i] = lo;
    p->ntap[i] = nt;
    rows[i].resize(std::max(nt, 0));
    for (int32_t j = 0; j < nt; ++j) {
      const double in_t = (lo + j) / static_cast<double>(fs_in), delta_t = in_t - out_t;
      rows[i][j] = filter_at((float)delta_t, cutoff) / fs_in;
    }
    p->K = std::max(p->K, nt);
  }
  p->w.assign((size_t)p->Q * p->K, 0.0f);
  for (int i = 0; i < p->Q; ++i) std::copy(rows[i].begin(), rows[i].end(), p->w.begin() + (size_t)i * p->K);
}

pfhip_status ResampleCache::get(int device, int fs_in, int fs_out, pfhip::ResampleTable* out) {
  std::string why;
  if (!resample_supported(fs_in, fs_out, &why)) return fail(PFHIP_ERR_UNSUPPORTED, why);
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(device, fs_in, fs_out);
  auto it = plans.find(key);
  if (it != plans.end()) { *out = it->second.t; return PFHIP_OK; }
  ResamplePlan p;
  build_resample_plan(fs_in, fs_out, &p);
  Plan dev;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(dev.first.upload(p.first));
  HIP_TRY(dev.ntap.upload(p.ntap));
  HIP_TRY(dev.w.upload(p.w));
  dev.t = pfhip::ResampleTable{dev.first.as<int>(), dev.ntap.as<int>(), dev.w.f(), p.P, p.Q, p.K};
  *out = dev.t;
  plans.emplace(key, std::move(dev));
  return PFHIP_OK;
}

}  // namespace pfhip_impl

extern "C" {

int64_t pfhip_resample_len(int fs_in, int fs_out, int64_t n_in) { return pfhip_impl::resample_out_len(fs_in, fs_out, n_in); }

int pfhip_op_resample_table(int fs_in, int fs_out, int32_t* first_index, int32_t* ntaps, float* weights, size_t cap_floats,
                            int* n_phases, int* taps, int* in_unit) {
  if (!pfhip_impl::resample_supported(fs_in, fs_out, nullptr)) return (int)hipErrorInvalidValue;
  pfhip_impl::ResamplePlan p;
  pfhip_impl::build_resample_plan(fs_in, fs_out, &p);
  if (n_phases) *n_phases = p.Q;
  if (taps) *taps = p.K;
  if (in_unit) *in_unit = p.P;
  if (!first_index && !ntaps && !weights) return 0;
  if (cap_floats < p.w.size()) return (int)hipErrorInvalidValue;
  if (first_index) std::copy(p.first.begin(), p.first.end(), first_index);
  if (ntaps) std::copy(p.ntap.begin(), p.ntap.end(), ntaps);
  if (weights) std::copy(p.w.begin(), p.w.end(), weights);
  return 0;
}

int pfhip_op_resample(const float* d_in, const int64_t* in_off, const int* n_in, int batch, int fs_in, int fs_out, float* d_out,
                      const int64_t* out_off, void* stream) {
  // process-wide plans for the operator entry (the handle API keeps its own per handle)
  static pfhip_impl::ResampleCache* cache = new pfhip_impl::ResampleCache;
  if (batch < 0 || (batch > 0 && (!in_off || !n_in || !out_off))) return (int)hipErrorInvalidValue;
  if (!pfhip_impl::resample_supported(fs_in, fs_out, nullptr)) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<int> n_out(batch);
  for (int b = 0; b < batch; ++b) {
    const int64_t n = pfhip_impl::resample_out_len(fs_in, fs_out, n_in[b]);
    if (n < 0 || n > INT_MAX) return (int)hipErrorInvalidValue;
    n_out[b] = (int)n;
  }
  if (fs_in == fs_out) {        // identity: a copy, no kernel (the reference skips WavResample, audio.cpp:808-810)
    for (int b = 0; b < batch; ++b)
      if (n_in[b] > 0) {
        const hipError_t e = hipMemcpyAsync(d_out + out_off[b], d_in + in_off[b], (size_t)n_in[b] * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
      }
    return 0;
  }
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  pfhip::ResampleTable t;
  if (cache->get(dev, fs_in, fs_out, &t) != PFHIP_OK) return (int)hipErrorInvalidValue;
  pfhip::launch_resample(d_in, in_off, n_in, d_out, out_off, n_out.data(), batch, t, s);
  return (int)hipGetLastError();
}

}  // extern "C"
