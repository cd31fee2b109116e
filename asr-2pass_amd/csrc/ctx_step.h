// One step of the hotword context graph on the device, shared by the two beam searches that walk it (ctc_beam.hip, nar_beam.hip).
#ifndef PFHIP_CTX_STEP_H_
#define PFHIP_CTX_STEP_H_
#include "kernels.h"

namespace pfhip {

// GetNextState (context_graph.cpp:95-118): the arc of `state` with label tok, else the state's escape weight and state 0
__device__ __forceinline__ int ctx_step(const CtxGraphDev& g, int state, int tok, float* w) {
  state = min(max(state, 0), g.n_states - 1);
  int lo = g.arc_begin[state], hi = g.arc_begin[state + 1];
  lo = min(max(lo, 0), g.n_arcs);
  hi = min(max(hi, lo), g.n_arcs);
  const int end = hi;
  while (lo < hi) {                                                  // at most 31 trips
    const int mid = lo + ((hi - lo) >> 1);
    if (g.arc_label[mid] < tok) lo = mid + 1; else hi = mid;
  }
  if (lo < end && g.arc_label[lo] == tok) {
    *w = g.arc_weight[lo];
    return min(max(g.arc_next[lo], 0), g.n_states - 1);
  }
  *w = g.escape[state];
  return 0;
}

}  // namespace pfhip
#endif
