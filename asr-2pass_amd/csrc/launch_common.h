// Host helpers shared by the launchers: the opt-in for more than 64 KB of dynamic LDS and the PFHIP_* environment knobs.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

namespace pfhip {

// Launches `kern` with `lds_bytes` of dynamic LDS.  > 64 KB of dynamic LDS needs the opt-in once per kernel (= per instantiation of
// this function) and device.
template <auto kern, int threads = 512, class... Args>
void launch_with_lds(dim3 grid, int lds_bytes, hipStream_t s, Args... args) {
  static std::atomic<unsigned long long> attr_done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!(attr_done.load(std::memory_order_relaxed) >> (dev & 63) & 1ull)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    attr_done.fetch_or(1ull << (dev & 63));
  }
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds_bytes, s, args...);
}

// Environment knobs.  These read the environment on every call: a knob that is fixed for the process keeps the result in a
// function-local `static const` at its point of use (read once, at first use); one that tests switch is read per launch.
inline bool env_on(const char* name) {          // on unless set to 0
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
inline bool env_is1(const char* name) {         // off unless set to 1
  const char* e = getenv(name);
  return e && e[0] == '1';
}
inline int env_int(const char* name, int dflt) {      // a number; unset or empty: dflt
  const char* e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}

}  // namespace pfhip
