// What launch_ctc_prefix_beam_multi reads from device memory besides the rows, laid out as one block that goes up in ONE copy: the
// descriptors BeamUtt [B] | the table CtxGraphDev [n_graphs] | the packed image of every graph that is not on the device already.
// Every part starts on a 16-byte boundary.  A graph with a device image elsewhere (resident[g] != null: the graph bank) takes no
// room here; its table entry points there.  Used by pfhip_op_ctc_prefix_beam_multi (ops_abi.cpp) and the SenseVoice head (heads.cpp).
#ifndef PFHIP_BEAM_FRONT_H_
#define PFHIP_BEAM_FRONT_H_
#include <cstring>

#include "ctx_graph.h"
#include "kernels.h"
#include "lm_graph.h"

namespace pfhip {

inline size_t ctx_graph_image_bytes(const pfhip_ctx_graph* g) { return g ? (g->packed.size() * 4 + 15) / 16 * 16 : 0; }

// the five arrays of g inside its packed image at `image` (a device address)
inline CtxGraphDev ctx_graph_dev(const pfhip_ctx_graph* g, const void* image) {
  CtxGraphDev dev;
  if (!g) return dev;
  const int S_ = g->n_states(), A = g->n_arcs();
  const int32_t* w = static_cast<const int32_t*>(image);
  dev.n_states = S_; dev.n_arcs = A;
  dev.arc_begin = w;
  dev.escape = reinterpret_cast<const float*>(w + S_ + 1);
  dev.arc_label = w + 2 * S_ + 1;
  dev.arc_next = w + 2 * S_ + 1 + A;
  dev.arc_weight = reinterpret_cast<const float*>(w + 2 * S_ + 1 + 2 * A);
  return dev;
}

// the token n-gram language model the same way (lm_graph.h `packed`): its image follows the block above in the same copy
inline size_t lm_graph_image_bytes(const pfhip_lm_graph* g) { return g ? (g->packed.size() * 4 + 15) / 16 * 16 : 0; }
inline LmGraphDev lm_graph_dev(const pfhip_lm_graph* g, const void* image) {
  LmGraphDev dev;
  if (!g) return dev;
  if (!image) {                                  // the counts alone: what a launcher's own checks read at B = 0
    dev.n_states = g->n_states(); dev.n_arcs = g->n_arcs(); dev.vocab = g->vocab; dev.start = g->start; dev.has_eos = g->has_eos;
    return dev;
  }
  const size_t U = (size_t)g->vocab + 1, S_ = (size_t)g->n_states(), A = (size_t)g->n_arcs();
  const int32_t* w = static_cast<const int32_t*>(image);
  dev.n_states = g->n_states(); dev.n_arcs = g->n_arcs(); dev.vocab = g->vocab; dev.start = g->start; dev.has_eos = g->has_eos;
  dev.uni_w = reinterpret_cast<const float*>(w);
  dev.uni_next = w + U;
  dev.arc_begin = w + 2 * U;
  dev.backoff_w = reinterpret_cast<const float*>(w + 2 * U + S_ + 1);
  dev.backoff_state = w + 2 * U + 2 * S_ + 1;
  dev.arc_label = w + 2 * U + 3 * S_ + 1;
  dev.arc_next = w + 2 * U + 3 * S_ + 1 + A;
  dev.arc_weight = reinterpret_cast<const float*>(w + 2 * U + 3 * S_ + 1 + 2 * A);
  return dev;
}

inline size_t beam_front_table_off(int B) { return ((size_t)B * sizeof(BeamUtt) + 15) / 16 * 16; }
inline size_t beam_front_image_off(int B, int n_graphs) { return beam_front_table_off(B) + ((size_t)n_graphs * sizeof(CtxGraphDev) + 15) / 16 * 16; }
inline size_t beam_front_bytes(int B, const pfhip_ctx_graph* const* graphs, int n_graphs, const void* const* resident = nullptr) {
  size_t n = beam_front_image_off(B, n_graphs);
  for (int g = 0; g < n_graphs; ++g)
    if (!resident || !resident[g]) n += ctx_graph_image_bytes(graphs[g]);
  return n;
}
// host: beam_front_bytes(...) bytes; dev: where they will lie on the device
inline void beam_front_fill(char* host, const char* dev, const BeamUtt* utt, int B, const pfhip_ctx_graph* const* graphs, int n_graphs,
                            const void* const* resident = nullptr) {
  if (B > 0) std::memcpy(host, utt, (size_t)B * sizeof(BeamUtt));
  CtxGraphDev* table = reinterpret_cast<CtxGraphDev*>(host + beam_front_table_off(B));
  size_t at = beam_front_image_off(B, n_graphs);
  for (int g = 0; g < n_graphs; ++g) {
    if (resident && resident[g]) { table[g] = ctx_graph_dev(graphs[g], resident[g]); continue; }
    table[g] = ctx_graph_dev(graphs[g], dev + at);
    std::memcpy(host + at, graphs[g]->packed.data(), graphs[g]->packed.size() * 4);
    at += ctx_graph_image_bytes(graphs[g]);
  }
}

}  // namespace pfhip
#endif
