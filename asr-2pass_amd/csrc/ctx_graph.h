// The hotword context graph of the CTC prefix beam search as the library keeps it (ctx_graph.cpp builds it, ctc_beam.hip walks it):
// a deterministic trie in CSR form.  State 0 is the start; arcs of state s are arc_*[arc_begin[s] .. arc_begin[s + 1]), sorted by
// label; escape[s] is what a token that matches no arc of s scores (next state 0; escape[0] = 0).  Host only: no HIP here.
#ifndef PFHIP_CTX_GRAPH_H_
#define PFHIP_CTX_GRAPH_H_
#include <cstdint>
#include <vector>

struct pfhip_ctx_graph {
  int vocab = 0;
  std::vector<int32_t> arc_begin;                // [n_states + 1]
  std::vector<int32_t> arc_label, arc_next;      // [n_arcs]
  std::vector<float> arc_weight;                 // [n_arcs]
  std::vector<float> escape;                     // [n_states]
  // the five arrays back to back as 32-bit words, in the order arc_begin, escape, arc_label, arc_next, arc_weight: what one copy
  // takes to the device (ops_abi.cpp)
  std::vector<int32_t> packed;
  int n_states() const { return (int)escape.size(); }
  int n_arcs() const { return (int)arc_label.size(); }
};

#endif
