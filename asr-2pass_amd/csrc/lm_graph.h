// The token n-gram language model of the device searches as the library keeps it (lm_graph.cpp builds it, lm_step.h walks it): a
// back-off automaton over the model's own tokens.  State 0 is the empty history and is direct-indexed by label (uni_w / uni_next,
// labels 0 .. vocab, vocab = </s>); every other state is a kept n-gram of length 1 .. order - 1 with its arcs in CSR form, sorted by
// label (state 0 has none there: arc_begin[0] == arc_begin[1] == 0), a back-off weight and a back-off state that is a strictly
// shorter history.  All weights are natural logarithms with scale and bonus baked in (include/pfhip.h states the rule).  Host only:
// no HIP here.
#ifndef PFHIP_LM_GRAPH_H_
#define PFHIP_LM_GRAPH_H_
#include <cstdint>
#include <vector>

struct pfhip_lm_graph {
  int vocab = 0, order = 0, start = 0, has_eos = 0;
  std::vector<float> uni_w;                      // [vocab + 1]
  std::vector<int32_t> uni_next;                 // [vocab + 1]
  std::vector<int32_t> arc_begin;                // [n_states + 1]
  std::vector<float> backoff_w;                  // [n_states]
  std::vector<int32_t> backoff_state;            // [n_states]
  std::vector<int32_t> arc_label, arc_next;      // [n_arcs]
  std::vector<float> arc_weight;                 // [n_arcs]
  // the eight arrays back to back as 32-bit words, in the order uni_w, uni_next, arc_begin, backoff_w, backoff_state, arc_label,
  // arc_next, arc_weight: what one copy takes to the device (ops_abi.cpp)
  std::vector<int32_t> packed;
  int n_states() const { return (int)backoff_w.size(); }
  int n_arcs() const { return (int)arc_label.size(); }
};

#endif
