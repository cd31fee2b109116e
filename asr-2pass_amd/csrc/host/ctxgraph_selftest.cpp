// Stand-alone check of the hotword context graph (ctx_graph.cpp; pfhip_ctx_graph_* of include/pfhip.h): hand-derived graphs and the
// refused inputs, with no device and no library.  Meant for a sanitizer build (make ctxgraph_selftest):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ctx_graph.cpp host/ctxgraph_selftest.cpp
// The buffers are heap blocks of exactly the size a call may touch, so an overrun by one element is a report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../../include/pfhip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Words {
  std::vector<int32_t> ids;
  std::vector<int> n;
  std::vector<float> w;
  void add(std::vector<int32_t> t, std::vector<float> ws) {
    n.push_back((int)t.size());
    ids.insert(ids.end(), t.begin(), t.end());
    w.insert(w.end(), ws.begin(), ws.end());
  }
};

struct Dump {
  std::vector<int32_t> begin, label, next;
  std::vector<float> escape, weight;
};

static pfhip_status build(const Words& in, int vocab, pfhip_ctx_graph** g) {
  // exactly-sized copies: a read past the last id or weight is a report
  std::unique_ptr<int32_t[]> ids(new int32_t[in.ids.size()]);
  std::unique_ptr<int[]> n(new int[in.n.size()]);
  std::unique_ptr<float[]> w(new float[in.w.size()]);
  for (size_t i = 0; i < in.ids.size(); ++i) ids[i] = in.ids[i];
  for (size_t i = 0; i < in.n.size(); ++i) n[i] = in.n[i];
  for (size_t i = 0; i < in.w.size(); ++i) w[i] = in.w[i];
  return pfhip_ctx_graph_create(ids.get(), n.get(), w.get(), (int)in.n.size(), vocab, g);
}

static Dump dump(const pfhip_ctx_graph* g) {
  Dump d;
  int S = -1, A = -1;
  CHECK(pfhip_ctx_graph_dump(g, &S, &A, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) == PFHIP_OK);
  CHECK(S >= 1 && A >= 0);
  std::unique_ptr<int32_t[]> begin(new int32_t[S + 1]), label(new int32_t[A]), next(new int32_t[A]);
  std::unique_ptr<float[]> escape(new float[S]), weight(new float[A]);
  CHECK(pfhip_ctx_graph_dump(g, &S, &A, begin.get(), escape.get(), S, label.get(), next.get(), weight.get(), A) == PFHIP_OK);
  if (A > 0) CHECK(pfhip_ctx_graph_dump(g, &S, &A, begin.get(), escape.get(), S, label.get(), next.get(), weight.get(), A - 1) == PFHIP_ERR_CAPACITY);
  CHECK(pfhip_ctx_graph_dump(g, &S, &A, begin.get(), escape.get(), S - 1, label.get(), next.get(), weight.get(), A) == PFHIP_ERR_CAPACITY);
  CHECK(pfhip_ctx_graph_dump(g, &S, &A, begin.get(), nullptr, S, label.get(), next.get(), weight.get(), A) == PFHIP_ERR_ARG);
  d.begin.assign(begin.get(), begin.get() + S + 1);
  d.escape.assign(escape.get(), escape.get() + S);
  d.label.assign(label.get(), label.get() + A);
  d.next.assign(next.get(), next.get() + A);
  d.weight.assign(weight.get(), weight.get() + A);
  // what the kernel relies on: monotone offsets, sorted labels inside a state, labels and states in range
  CHECK(d.begin[0] == 0 && d.begin[S] == A && d.escape[0] == 0.f);
  for (int s = 0; s < S; ++s) {
    CHECK(d.begin[s] <= d.begin[s + 1]);
    for (int a = d.begin[s]; a < d.begin[s + 1]; ++a) {
      CHECK(a == d.begin[s] || d.label[a - 1] < d.label[a]);
      CHECK(d.label[a] >= 1 && d.label[a] < pfhip_ctx_graph_vocab(g) && d.next[a] >= 0 && d.next[a] < S && std::isfinite(d.weight[a]));
    }
  }
  return d;
}

static void expect(const Words& in, int vocab, const Dump& want) {
  pfhip_ctx_graph* g = nullptr;
  CHECK(build(in, vocab, &g) == PFHIP_OK);
  if (!g) return;
  CHECK(pfhip_ctx_graph_vocab(g) == vocab);
  const Dump d = dump(g);
  CHECK(d.begin == want.begin);
  CHECK(d.label == want.label);
  CHECK(d.next == want.next);
  CHECK(d.escape == want.escape);
  CHECK(d.weight == want.weight);
  pfhip_ctx_graph_destroy(g);
}

static void refused(const Words& in, int vocab) {
  pfhip_ctx_graph* g = reinterpret_cast<pfhip_ctx_graph*>(1);
  CHECK(build(in, vocab, &g) == PFHIP_ERR_ARG);
  CHECK(g == nullptr);
}

int main() {
  {  // no hotword at all: state 0 alone
    Words w;
    expect(w, 10, {{0, 0}, {}, {}, {0.f}, {}});
  }
  {  // disjoint words [1 2] and [3]: one inner state
    Words w;
    w.add({1, 2}, {1.f, 1.f});
    w.add({3}, {2.f});
    expect(w, 10, {{0, 2, 3}, {1, 3, 2}, {1, 0, 0}, {0.f, -1.f}, {1.f, 2.f, 1.f}});
  }
  {  // shared prefix with different weights: [1 2] at 1 a token, [1 3] at 3 a token: minCum of the shared node is 1
    Words w;
    w.add({1, 2}, {1.f, 1.f});
    w.add({1, 3}, {3.f, 3.f});
    expect(w, 10, {{0, 1, 3}, {1, 2, 3}, {1, 0, 0}, {0.f, -1.f}, {1.f, 1.f, 5.f}});
  }
  {  // a duplicate word keeps the lighter copy
    Words w;
    w.add({4, 5}, {2.f, 2.f});
    w.add({4, 5}, {1.f, 1.f});
    expect(w, 10, {{0, 1, 2}, {4, 5}, {1, 0}, {0.f, -1.f}, {1.f, 1.f}});
  }
  {  // [1 2] (1 a token) is a prefix of [1 2 3] (0.5 a token); [1 4] at 2 a token.  Node after 1: minCum 0.5.  Node after 1 2:
     // minCum min(1.0, 2) = 1.0, final with r0 = 1; it carries state 0's arc 1 -> node 1 at r0 + 0.5 and keeps its escape -1.
    Words w;
    w.add({1, 2}, {1.f, 1.f});
    w.add({1, 2, 3}, {.5f, .5f, .5f});
    w.add({1, 4}, {2.f, 2.f});
    expect(w, 6, {{0, 1, 3, 5}, {1, 2, 4, 1, 3}, {1, 2, 0, 1, 0}, {0.f, -.5f, -1.f}, {.5f, .5f, 3.5f, 1.5f, .5f}});
  }
  {  // 200 random words of 2 .. 6 tokens over 50 ids: the invariants of dump() and no sanitizer report
    std::mt19937 rng(7);
    Words w;
    for (int j = 0; j < 200; ++j) {
      std::vector<int32_t> t;
      std::vector<float> ws;
      const int n = 2 + (int)(rng() % 5);
      for (int i = 0; i < n; ++i) { t.push_back(1 + (int)(rng() % 49)); ws.push_back(0.25f * (float)(1 + rng() % 16)); }
      w.add(t, ws);
    }
    pfhip_ctx_graph* g = nullptr;
    CHECK(build(w, 50, &g) == PFHIP_OK);
    if (g) { dump(g); pfhip_ctx_graph_destroy(g); }
  }
  {  // the refused inputs
    Words a; a.add({1, 0}, {1.f, 1.f}); refused(a, 10);                                   // id 0 is the escape label
    Words b; b.add({1, 10}, {1.f, 1.f}); refused(b, 10);                                  // id == vocab
    Words c; c.add({-1}, {1.f}); refused(c, 10);
    Words d; d.add({1}, {1.f}); d.n.push_back(0); refused(d, 10);                         // an empty word
    Words e; e.add({1, 2}, {1.f, std::numeric_limits<float>::infinity()}); refused(e, 10);
    Words f; f.add({1, 2}, {std::nanf(""), 1.f}); refused(f, 10);
    Words h; h.add({1, 2}, {3e38f, 3e38f}); refused(h, 10);                               // the cumulative weight overflows
    Words i; i.add({1}, {1.f}); refused(i, 1);                                            // no vocabulary
    CHECK(pfhip_ctx_graph_create(nullptr, nullptr, nullptr, 1, 10, nullptr) == PFHIP_ERR_ARG);
    pfhip_ctx_graph* g = nullptr;
    CHECK(pfhip_ctx_graph_create(nullptr, nullptr, nullptr, 1, 10, &g) == PFHIP_ERR_ARG);
    int S, A;
    CHECK(pfhip_ctx_graph_dump(nullptr, &S, &A, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) == PFHIP_ERR_ARG);
    pfhip_ctx_graph_destroy(nullptr);
    CHECK(pfhip_ctx_graph_vocab(nullptr) == 0);
  }
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("ctxgraph_selftest: ok\n");
  return 0;
}
