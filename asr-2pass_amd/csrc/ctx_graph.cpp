// The hotword context graph of the CTC prefix beam search (pfhip_ctx_graph_*, include/pfhip.h): host only, no HIP include, so that
// it builds stand-alone (make ctxgraph_selftest).
//
// What the reference walks (BuildContextGraph + GetNextState, onnxruntime/src/context_graph.cpp:33-118) is the tropical
// determinisation of one linear chain per hotword from state 0 back to state 0, every inner chain state carrying an escape arc
// (label 0) of minus the weight collected so far.  Determinised, the chains that share a prefix share its states, and a state's
// subset holds one residual per chain: the chain's cumulative weight minus the least cumulative weight of the subset.  So, with
// minCum(node) = the least cumulative weight over the hotwords through that trie node:
//   * the arc into a node weighs minCum(node) - minCum(parent);
//   * the last token of a hotword leads back to state 0 and weighs its cumulative weight - minCum(parent) (duplicates: the least);
//   * the escape arcs of a subset (all label 0, all to state 0) collapse to the least, -cum + residual = -minCum(state);
//   * a hotword that is a proper prefix of another puts state 0 (residual r0 = its cumulative weight - minCum) into the subset of
//     the node S the longer one continues from: S also has state 0's arcs, each r0 heavier, and keeps its escape -minCum(S).
// One simplification against the full subset construction (DESIGN §6 says so too): where S has an arc of its own with the label
// of one of state 0's arcs, its own arc is kept alone; the determiniser would fuse the two destinations into a further subset.
// All sums and differences are single fp32 operations in the order written here; tests/ctc_beam_ref.py restates them.
#include "ctx_graph.h"

#include "../../include/pfhip.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <cstring>
#include <map>
#include <new>

namespace {

struct Node {
  std::map<int, int> child;                      // label -> node
  std::map<int, float> end;                      // label of a hotword's last token -> its least cumulative weight
  float min_cum = std::numeric_limits<float>::infinity();
  bool is_final = false;                         // a hotword ends ON this node (it is a proper prefix of another)
  float end_cum = std::numeric_limits<float>::infinity();
};

struct Arc {
  int label, next;
  float weight;
};

}  // namespace

extern "C" {

pfhip_status pfhip_ctx_graph_create(const int32_t* ids, const int* n_ids, const float* tok_weight, int n_words, int vocab, pfhip_ctx_graph** g) {
  if (!g) return PFHIP_ERR_ARG;
  *g = nullptr;
  if (n_words < 0 || vocab < 2 || (n_words > 0 && (!ids || !n_ids || !tok_weight))) return PFHIP_ERR_ARG;
  long long total = 0;
  for (int j = 0; j < n_words; ++j) {
    if (n_ids[j] < 1) return PFHIP_ERR_ARG;                          // an empty word
    total += n_ids[j];
    if (total > 0x3fffffffLL) return PFHIP_ERR_ARG;
  }
  for (long long i = 0; i < total; ++i)
    if (ids[i] < 1 || ids[i] >= vocab || !std::isfinite(tok_weight[i])) return PFHIP_ERR_ARG;      // 0 is the escape label

  std::vector<Node> nodes(1);
  nodes[0].min_cum = 0.f;
  size_t at = 0;
  for (int j = 0; j < n_words; ++j) {
    float cum = 0.f;
    int node = 0;
    for (int i = 0; i < n_ids[j]; ++i, ++at) {
      const int t = ids[at];
      cum = cum + tok_weight[at];
      if (!std::isfinite(cum)) return PFHIP_ERR_ARG;
      if (i + 1 < n_ids[j]) {
        auto it = nodes[node].child.find(t);
        int c;
        if (it == nodes[node].child.end()) {
          c = (int)nodes.size();
          nodes[node].child[t] = c;
          nodes.emplace_back();
        } else {
          c = it->second;
        }
        nodes[c].min_cum = std::min(nodes[c].min_cum, cum);
        node = c;
      } else {
        auto it = nodes[node].end.find(t);
        if (it == nodes[node].end.end()) nodes[node].end[t] = cum;
        else it->second = std::min(it->second, cum);
      }
    }
  }
  // a hotword that ends where another goes on: the shared node is final and its least weight counts the shorter word too
  for (Node& u : nodes)
    for (const auto& e : u.end) {
      auto it = u.child.find(e.first);
      if (it == u.child.end()) continue;
      Node& v = nodes[it->second];
      v.is_final = true;
      v.end_cum = std::min(v.end_cum, e.second);
      v.min_cum = std::min(v.min_cum, e.second);
    }
  const int n_states = (int)nodes.size();
  std::vector<std::vector<Arc>> arcs((size_t)n_states);
  for (int u = 0; u < n_states; ++u) {
    for (const auto& c : nodes[u].child) arcs[u].push_back({c.first, c.second, nodes[c.second].min_cum - nodes[u].min_cum});
    for (const auto& e : nodes[u].end)
      if (!nodes[u].child.count(e.first)) arcs[u].push_back({e.first, 0, e.second - nodes[u].min_cum});
  }
  const std::vector<Arc> root = arcs[0];
  for (int u = 1; u < n_states; ++u) {
    if (!nodes[u].is_final) continue;
    const float r0 = nodes[u].end_cum - nodes[u].min_cum;
    for (const Arc& a : root)
      if (!nodes[u].child.count(a.label) && !nodes[u].end.count(a.label)) arcs[u].push_back({a.label, a.next, r0 + a.weight});
  }
  pfhip_ctx_graph* out = new (std::nothrow) pfhip_ctx_graph;
  if (!out) return PFHIP_ERR_ARG;
  out->vocab = vocab;
  out->arc_begin.push_back(0);
  for (int u = 0; u < n_states; ++u) {
    std::sort(arcs[u].begin(), arcs[u].end(), [](const Arc& a, const Arc& b) { return a.label < b.label; });
    for (const Arc& a : arcs[u]) {
      out->arc_label.push_back(a.label);
      out->arc_next.push_back(a.next);
      out->arc_weight.push_back(a.weight);
    }
    out->arc_begin.push_back((int32_t)out->arc_label.size());
    out->escape.push_back(u == 0 ? 0.f : -nodes[u].min_cum);
  }
  auto words = [&](const void* src, size_t n) {
    const size_t at = out->packed.size();
    out->packed.resize(at + n);
    if (n) std::memcpy(out->packed.data() + at, src, 4 * n);
  };
  words(out->arc_begin.data(), out->arc_begin.size());
  words(out->escape.data(), out->escape.size());
  words(out->arc_label.data(), out->arc_label.size());
  words(out->arc_next.data(), out->arc_next.size());
  words(out->arc_weight.data(), out->arc_weight.size());
  *g = out;
  return PFHIP_OK;
}

void pfhip_ctx_graph_destroy(pfhip_ctx_graph* g) { delete g; }

int pfhip_ctx_graph_vocab(const pfhip_ctx_graph* g) { return g ? g->vocab : 0; }

pfhip_status pfhip_ctx_graph_dump(const pfhip_ctx_graph* g, int* n_states, int* n_arcs, int32_t* arc_begin, float* escape, int cap_states,
                         int32_t* arc_label, int32_t* arc_next, float* arc_weight, int cap_arcs) {
  if (!g || !n_states || !n_arcs) return PFHIP_ERR_ARG;
  *n_states = g->n_states();
  *n_arcs = g->n_arcs();
  if (!arc_begin && !escape && !arc_label && !arc_next && !arc_weight) return PFHIP_OK;       // the sizes alone
  if (!arc_begin || !escape || !arc_label || !arc_next || !arc_weight) return PFHIP_ERR_ARG;
  if (cap_states < g->n_states() || cap_arcs < g->n_arcs()) return PFHIP_ERR_CAPACITY;
  std::copy(g->arc_begin.begin(), g->arc_begin.end(), arc_begin);
  std::copy(g->escape.begin(), g->escape.end(), escape);
  std::copy(g->arc_label.begin(), g->arc_label.end(), arc_label);
  std::copy(g->arc_next.begin(), g->arc_next.end(), arc_next);
  std::copy(g->arc_weight.begin(), g->arc_weight.end(), arc_weight);
  return PFHIP_OK;
}

}  // extern "C"
