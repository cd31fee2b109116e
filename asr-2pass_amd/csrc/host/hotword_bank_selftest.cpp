// Self-test of the hotword bank's bookkeeping (../hotword_bank.h): host code only, built by tests/test_hotword_bank.py with
// g++ -fsanitize=address,undefined.   hotword_bank_selftest <case>   prints "ok <case>" and exits 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../hotword_bank.h"

using pfhip_impl::HotwordBank;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
constexpr int kD = 8, kG = 4;          // 8 floats per row, 4-row granules
std::vector<float> make_set(int H, float seed) {
  std::vector<float> v((size_t)H * kD);
  for (size_t i = 0; i < v.size(); ++i) v[i] = seed + 0.25f * (float)i;
  return v;
}
uint64_t same_hash(const float*, size_t, int) { return 42; }

int collision() {
  HotwordBank b;
  b.hash_fn = same_hash;                 // every set collides
  b.configure(kG, kD, 8);
  const auto A = make_set(3, 1.f), B = make_set(3, 2.f);
  bool hit = true;
  const int a = b.acquire(A.data(), 3, &hit);
  CHECK(a >= 0 && !hit);
  const int c = b.acquire(B.data(), 3, &hit);
  CHECK(c >= 0 && c != a && !hit);        // same hash, same H, other bytes: another entry
  CHECK(b.row_off(a) != b.row_off(c));
  const int a2 = b.acquire(A.data(), 3, &hit);
  CHECK(a2 == a && hit);
  const int c2 = b.acquire(B.data(), 3, &hit);
  CHECK(c2 == c && hit);
  const auto A5 = make_set(5, 1.f);       // same leading bytes, other H
  const int e = b.acquire(A5.data(), 5, &hit);
  CHECK(e >= 0 && e != a && e != c && !hit);
  CHECK(b.hits == 2 && b.misses == 3 && b.evictions == 0);
  // the real hash separates H as well as content
  CHECK(pfhip_impl::hotword_hash(A.data(), A.size(), 3) != pfhip_impl::hotword_hash(B.data(), B.size(), 3));
  CHECK(pfhip_impl::hotword_hash(A.data(), A.size(), 3) != pfhip_impl::hotword_hash(A.data(), A.size(), 4));
  return 0;
}

int lru() {
  HotwordBank b;
  b.configure(kG, kD, 3);                 // three one-granule slabs
  const auto A = make_set(2, 1.f), B = make_set(4, 2.f), C = make_set(1, 3.f), D = make_set(3, 4.f);
  bool hit;
  const int a = b.acquire(A.data(), 2, &hit); b.release(a);
  const int bb = b.acquire(B.data(), 4, &hit); b.release(bb);
  const int c = b.acquire(C.data(), 1, &hit); b.release(c);
  CHECK(b.used_granules() == 3);
  CHECK(b.acquire(A.data(), 2, &hit) == a && hit); b.release(a);       // A is now the most recent; B the oldest
  const int d = b.acquire(D.data(), 3, &hit);
  CHECK(d >= 0 && !hit && b.evictions == 1);
  b.release(d);
  CHECK(b.acquire(A.data(), 2, &hit) == a && hit); b.release(a);       // A and C stayed
  CHECK(b.acquire(C.data(), 1, &hit) == c && hit); b.release(c);
  const int b2 = b.acquire(B.data(), 4, &hit);                         // B went: a miss again, and D (now the oldest) goes for it
  CHECK(b2 >= 0 && !hit && b.evictions == 2);
  b.release(b2);
  (void)b.acquire(D.data(), 3, &hit);
  CHECK(!hit);
  return 0;
}

int pinned() {
  HotwordBank b;
  b.configure(kG, kD, 2);
  const auto A = make_set(4, 1.f), B = make_set(4, 2.f), C = make_set(4, 3.f), Big = make_set(9, 5.f);
  bool hit;
  const int a = b.acquire(A.data(), 4, &hit);       // stays pinned: a forward in flight
  const int bb = b.acquire(B.data(), 4, &hit);      // pinned too
  CHECK(a >= 0 && bb >= 0);
  CHECK(b.acquire(C.data(), 4, &hit) == -1 && !hit);          // no room beside the pinned slabs: the per-call path
  CHECK(b.evictions == 0 && b.refused == 1);
  CHECK(b.acquire(A.data(), 4, &hit) == a && hit);            // a second forward with the same set: second pin
  b.release(a);
  CHECK(b.acquire(C.data(), 4, &hit) == -1);                  // one pin of A is left
  b.release(bb);                                              // B's forward completed
  const int c = b.acquire(C.data(), 4, &hit);
  CHECK(c >= 0 && !hit && b.evictions == 1);
  CHECK(b.row_off(c) != b.row_off(a));                        // A's slab was not touched
  CHECK(b.entry(a).live && b.entry(a).pins == 1 && b.entry(a).host == A);
  CHECK(b.acquire(Big.data(), 9, &hit) == -1);                // three granules never fit an arena of two
  CHECK(b.evictions == 1);                                    // ... and nothing was evicted for it
  return 0;
}

int freelist() {
  HotwordBank b;
  b.configure(kG, kD, 6);
  const auto A = make_set(4, 1.f), B = make_set(8, 2.f), C = make_set(4, 3.f), D = make_set(12, 4.f), E = make_set(7, 6.f);
  bool hit;
  const int a = b.acquire(A.data(), 4, &hit);       // granule 0
  const int bb = b.acquire(B.data(), 8, &hit);      // 1-2
  const int c = b.acquire(C.data(), 4, &hit);       // 3
  CHECK(b.row_off(a) == 0 && b.row_off(bb) == 4 && b.row_off(c) == 12 && b.used_granules() == 4);
  b.release(a); b.release(bb);                       // C stays pinned
  // D needs three granules in a row: 4-5 are free, 0 and 1-2 come free by eviction and coalesce into 0-2
  const int d = b.acquire(D.data(), 12, &hit);
  CHECK(d >= 0 && !hit && b.row_off(d) == 0 && b.evictions == 2 && b.used_granules() == 4);
  // the entry ids of the evicted sets are handed out again, and the tail run serves the next set
  const int e = b.acquire(E.data(), 7, &hit);
  CHECK(e >= 0 && (e == a || e == bb) && b.row_off(e) == 16 && b.used_granules() == 6);
  CHECK(b.id_count() == 3);
  CHECK(b.entry(c).live && b.row_off(c) == 12);
  return 0;
}

int unpin() {
  HotwordBank b;
  b.configure(kG, kD, 1);
  const auto A = make_set(2, 1.f), B = make_set(2, 2.f);
  bool hit;
  const int a = b.acquire(A.data(), 2, &hit);
  CHECK(b.pinned_entries() == 1);
  CHECK(b.acquire(B.data(), 2, &hit) == -1);
  b.release(a);                                     // the forward completed
  CHECK(b.pinned_entries() == 0 && b.live_entries() == 1);
  b.release(a);                                     // a stray second release does not go negative
  CHECK(b.entry(a).pins == 0);
  const int bb = b.acquire(B.data(), 2, &hit);
  CHECK(bb >= 0 && !hit && b.evictions == 1 && b.row_off(bb) == 0);
  b.release(bb);
  // a slab whose upload failed is taken out again: the set is a miss next time, and the failed attempt is no eviction
  const auto C = make_set(3, 7.f);
  const int c = b.acquire(C.data(), 3, &hit);
  CHECK(c >= 0 && !hit && b.evictions == 2);
  b.discard(c);
  CHECK(b.live_entries() == 0 && b.used_granules() == 0 && b.evictions == 2);
  CHECK(b.acquire(C.data(), 3, &hit) >= 0 && !hit);
  // reconfiguring drops everything and resizes
  b.configure(kG, kD, 0);
  CHECK(b.live_entries() == 0 && b.acquire(A.data(), 2, &hit) == -1);
  b.configure(kG, kD, 2);
  CHECK(b.acquire(A.data(), 2, &hit) >= 0 && !hit);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (what == "collision") rc = collision();
  else if (what == "lru") rc = lru();
  else if (what == "pinned") rc = pinned();
  else if (what == "freelist") rc = freelist();
  else if (what == "unpin") rc = unpin();
  else std::printf("usage: %s collision|lru|pinned|freelist|unpin\n", argv[0]);
  if (rc == 0) std::printf("ok %s\n", what.c_str());
  return rc;
}
