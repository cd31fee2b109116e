// Stand-alone check of the graph bank's bookkeeping (../graph_bank.h over ../hotword_bank.h), keyed by the packed images of graphs
// the real builder made (../ctx_graph.cpp): host code only, no device and no library.  Meant for a sanitizer build
// (make graph_bank_selftest):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ctx_graph.cpp host/graph_bank_selftest.cpp
//   graph_bank_selftest [hit_miss|pinned|lru|refusal|collision|padding]   no argument: every case.  Prints "ok <case>" per case.
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/pfhip.h"
#include "../ctx_graph.h"
#include "../graph_bank.h"

using pfhip_impl::HotwordBank;
using pfhip_impl::kGraphRowBytes;
using pfhip_impl::kGraphRowWords;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
constexpr int kVocab = 5000;

// n_words hotwords of `len` tokens each, all different through `seed`: the image has 2 S + 1 + 3 A words with A = S - 1 + n_words
struct Graph {
  pfhip_ctx_graph* g = nullptr;
  Graph(int n_words, int len, int seed) {
    std::vector<int32_t> ids;
    std::vector<int> n;
    std::vector<float> w;
    for (int i = 0; i < n_words; ++i) {
      n.push_back(len);
      for (int j = 0; j < len; ++j) { ids.push_back(1 + (seed * 131 + i * 17 + j * 7) % (kVocab - 1)); w.push_back(0.5f + 0.25f * (float)(j % 3)); }
    }
    if (pfhip_ctx_graph_create(ids.data(), n.data(), w.data(), n_words, kVocab, &g) != PFHIP_OK) g = nullptr;
  }
  ~Graph() { pfhip_ctx_graph_destroy(g); }
  Graph(const Graph&) = delete;
  Graph& operator=(const Graph&) = delete;
  size_t words() const { return g->packed.size(); }
  int rows() const { return pfhip_impl::graph_bank_rows(words()); }
};

int acquire(HotwordBank& b, const Graph& x, bool* hit) {
  std::vector<float> scratch;
  return pfhip_impl::graph_bank_acquire(b, x.g->packed.data(), x.words(), hit, &scratch);
}

uint64_t same_hash(const float*, size_t, int) { return 42; }

int hit_miss() {
  HotwordBank b;
  pfhip_impl::graph_bank_configure(b, 1 << 20);
  CHECK(b.capacity_granules() == (1 << 20) / (int)kGraphRowBytes && b.granule_rows() == 1);
  const Graph A(20, 3, 1), A2(20, 3, 1), B(20, 3, 2);
  CHECK(A.g && A2.g && B.g && A.g != A2.g && A.g->packed == A2.g->packed && A.g->packed != B.g->packed);
  bool hit = true;
  const int a = acquire(b, A, &hit);
  CHECK(a >= 0 && !hit && b.misses == 1 && b.hits == 0);
  CHECK(b.used_granules() == A.rows() && A.rows() == (int)((A.words() + 63) / 64));
  CHECK(acquire(b, A2, &hit) == a && hit && b.hits == 1);              // another handle, the same content: found again
  const int c = acquire(b, B, &hit);
  CHECK(c >= 0 && c != a && !hit && b.misses == 2);
  CHECK(pfhip_impl::graph_bank_offset(b, c) == (size_t)A.rows() * kGraphRowBytes && pfhip_impl::graph_bank_offset(b, a) == 0);
  // what the books keep is the image, zero-padded to whole rows
  const HotwordBank::Entry& e = b.entry(a);
  CHECK(e.H == A.rows() && e.host.size() == (size_t)A.rows() * kGraphRowWords && e.pins == 2);
  CHECK(std::memcmp(e.host.data(), A.g->packed.data(), A.words() * 4) == 0);
  for (size_t i = A.words(); i < e.host.size(); ++i) CHECK(e.host[i] == 0.f);
  return 0;
}

int pinned() {                                   // a pin blocks eviction; the release makes room
  const Graph A(40, 4, 3), B(40, 4, 4), C(40, 4, 5);
  CHECK(A.rows() == B.rows() && B.rows() == C.rows() && A.rows() >= 2);
  HotwordBank b;
  pfhip_impl::graph_bank_configure(b, (int64_t)2 * A.rows() * (int64_t)kGraphRowBytes);      // room for two of them
  bool hit;
  const int a = acquire(b, A, &hit), bb = acquire(b, B, &hit);
  CHECK(a >= 0 && bb >= 0 && b.pinned_entries() == 2);
  CHECK(acquire(b, C, &hit) == -1 && !hit && b.refused == 1 && b.evictions == 0);            // both in use: C goes up with its call
  b.release(bb);                                 // B's forward has synchronised
  const int c = acquire(b, C, &hit);
  CHECK(c >= 0 && !hit && b.evictions == 1);
  CHECK(b.entry(a).live && b.entry(a).pins == 1 && pfhip_impl::graph_bank_offset(b, a) == 0);      // A was not touched
  CHECK(pfhip_impl::graph_bank_offset(b, c) == (size_t)A.rows() * kGraphRowBytes);
  CHECK(acquire(b, B, &hit) == -1 && !hit);      // B went, and A and C are pinned
  return 0;
}

int lru() {
  const Graph A(40, 4, 6), B(40, 4, 7), C(40, 4, 8), D(40, 4, 9);
  HotwordBank b;
  pfhip_impl::graph_bank_configure(b, (int64_t)3 * A.rows() * (int64_t)kGraphRowBytes);
  bool hit;
  const int a = acquire(b, A, &hit); b.release(a);
  const int bb = acquire(b, B, &hit); b.release(bb);
  const int c = acquire(b, C, &hit); b.release(c);
  CHECK(acquire(b, A, &hit) == a && hit); b.release(a);                // A is the most recent now, B the oldest
  const int d = acquire(b, D, &hit);
  CHECK(d >= 0 && !hit && b.evictions == 1); b.release(d);
  CHECK(acquire(b, A, &hit) == a && hit); b.release(a);                // A and C stayed
  CHECK(acquire(b, C, &hit) == c && hit); b.release(c);
  const int b2 = acquire(b, B, &hit);                                  // B went: a miss again, and D — the oldest now — goes for it
  CHECK(b2 >= 0 && !hit && b.evictions == 2); b.release(b2);
  (void)acquire(b, D, &hit);
  CHECK(!hit);
  return 0;
}

int refusal() {
  const Graph Small(2, 2, 10), Big(1000, 5, 11);
  CHECK(Big.rows() > 100 && Small.rows() == 1);
  HotwordBank b;
  pfhip_impl::graph_bank_configure(b, 0);       // a bank of nothing: every graph goes up with its call
  bool hit = true;
  CHECK(b.capacity_granules() == 0 && acquire(b, Small, &hit) == -1 && !hit && b.refused == 1 && b.misses == 0);
  pfhip_impl::graph_bank_configure(b, (int64_t)100 * (int64_t)kGraphRowBytes + 17);       // whole rows only
  CHECK(b.capacity_granules() == 100);
  CHECK(acquire(b, Big, &hit) == -1 && !hit && b.evictions == 0);      // larger than the arena: nothing is evicted for it
  const int s = acquire(b, Small, &hit);
  CHECK(s >= 0 && !hit && b.used_granules() == 1);
  b.release(s);
  pfhip_impl::graph_bank_configure(b, -5);      // a negative bound is no bound to allocate
  CHECK(b.capacity_granules() == 0 && b.live_entries() == 0);
  return 0;
}

int collision() {                                // two contents under one hash are two entries, told apart by the byte compare
  const Graph A(20, 3, 12), B(20, 3, 13);
  CHECK(A.words() == B.words() && A.g->packed != B.g->packed);
  HotwordBank b;
  b.hash_fn = same_hash;
  pfhip_impl::graph_bank_configure(b, 1 << 20);
  bool hit = true;
  const int a = acquire(b, A, &hit);
  CHECK(a >= 0 && !hit);
  const int c = acquire(b, B, &hit);
  CHECK(c >= 0 && c != a && !hit && pfhip_impl::graph_bank_offset(b, a) != pfhip_impl::graph_bank_offset(b, c));
  CHECK(acquire(b, A, &hit) == a && hit);
  CHECK(acquire(b, B, &hit) == c && hit);
  CHECK(b.hits == 2 && b.misses == 2);
  return 0;
}

int padding() {                                  // an image and its zero-extended twin differ in their row count: two entries
  HotwordBank b;
  pfhip_impl::graph_bank_configure(b, 1 << 16);
  std::vector<int32_t> one((size_t)kGraphRowWords, 7), two((size_t)kGraphRowWords + 1, 7);
  two.back() = 0;
  std::vector<float> scratch;
  bool hit;
  const int a = pfhip_impl::graph_bank_acquire(b, one.data(), one.size(), &hit, &scratch);
  CHECK(a >= 0 && !hit && b.entry(a).H == 1);
  const int c = pfhip_impl::graph_bank_acquire(b, two.data(), two.size(), &hit, &scratch);
  CHECK(c >= 0 && c != a && !hit && b.entry(c).H == 2);
  std::vector<int32_t> short_one((size_t)kGraphRowWords - 3, 7);       // fewer words, the same rows, other bytes
  const int d = pfhip_impl::graph_bank_acquire(b, short_one.data(), short_one.size(), &hit, &scratch);
  CHECK(d >= 0 && d != a && !hit);
  return 0;
}

const struct { const char* name; int (*run)(); } kCases[] = {{"hit_miss", hit_miss}, {"pinned", pinned},       {"lru", lru},
                                                             {"refusal", refusal},   {"collision", collision}, {"padding", padding}};
}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  int ran = 0;
  for (const auto& c : kCases) {
    if (!what.empty() && what != c.name) continue;
    ++ran;
    if (c.run() != 0) return 1;
    std::printf("ok %s\n", c.name);
  }
  if (!ran) { std::printf("usage: %s [hit_miss|pinned|lru|refusal|collision|padding]\n", argv[0]); return 2; }
  return 0;
}
