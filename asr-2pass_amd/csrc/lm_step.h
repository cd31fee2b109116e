// One step of the token n-gram language model on the device (lm_graph.h; include/pfhip.h states the automaton), shared by the sentence
// scorer (lm_score.hip) and the beam searches that walk the model.
#ifndef PFHIP_LM_STEP_H_
#define PFHIP_LM_STEP_H_
#include "kernels.h"

namespace pfhip {

// The weight of `label` (0 .. vocab, vocab = </s>) after the history `state` and the state behind it: the arc of the state, else its
// back-off weight and the same question in its back-off state, down to state 0, which answers every label.  *w is the fp32 sum of
// what was collected, each a single add in the order met, starting from 0.  The loop is bounded by kLmOrderMax trips whatever the
// image holds (a builder's back-off state is a strictly shorter history: order - 1 trips at most); past them the step falls to
// state 0.  Every index is clamped into its array.
__device__ __forceinline__ int lm_step(const LmGraphDev& g, int state, int label, float* w) {
  float acc = 0.f;
  label = min(max(label, 0), g.vocab);
  state = min(max(state, 0), g.n_states - 1);
  for (int trip = 0; trip < kLmOrderMax && state != 0; ++trip) {
    int lo = g.arc_begin[state], hi = g.arc_begin[state + 1];
    lo = min(max(lo, 0), g.n_arcs);
    hi = min(max(hi, lo), g.n_arcs);
    const int end = hi;
    while (lo < hi) {                                                // at most 31 trips
      const int mid = lo + ((hi - lo) >> 1);
      if (g.arc_label[mid] < label) lo = mid + 1; else hi = mid;
    }
    if (lo < end && g.arc_label[lo] == label) {
      acc = acc + g.arc_weight[lo];
      *w = acc;
      return min(max(g.arc_next[lo], 0), g.n_states - 1);
    }
    acc = acc + g.backoff_w[state];
    state = min(max(g.backoff_state[state], 0), g.n_states - 1);
  }
  acc = acc + g.uni_w[label];
  *w = acc;
  return min(max(g.uni_next[label], 0), g.n_states - 1);
}

}  // namespace pfhip
#endif
