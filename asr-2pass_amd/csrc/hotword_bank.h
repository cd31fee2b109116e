// Bookkeeping of the per-device hotword bank (hotwords.cpp): which hotword sets have their bias-decoder K/V rows resident in the
// device arena, where, and which of them may be overwritten.  Host code only — no HIP — so it is tested without a GPU
// (host/hotword_bank_selftest.cpp).  The arena is a row-addressed array of `granule`-row granules; a set of H rows owns a
// contiguous run of ceil(H / granule) granules (its slab), so a projection GEMM that pads its M to the granule writes only rows
// of its own slab.
//   * Sets are keyed by content: a 64-bit hash of the H x d floats and H, confirmed by a byte compare against the host copy the
//     entry keeps (two sets with one hash are two entries).
//   * acquire() pins the entry it returns; release() unpins.  A pinned slab is never evicted or handed out again: a forward pins
//     its sets before its first launch and releases them after its last synchronise.
//   * Room is made by evicting the least recently used unpinned entries.  A set larger than the arena, or one that does not fit
//     beside the pinned slabs, is refused (-1): the caller serves it from a per-call buffer.
// Not thread-safe: the owner serialises calls (the device's bank mutex, held until the uploads of the misses are enqueued).
#pragma once
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <unordered_map>
#include <vector>

namespace pfhip_impl {

// word-wise multiply-xorshift over the floats' bytes, H mixed in
inline uint64_t hotword_hash(const float* emb, size_t n_floats, int H) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)(uint32_t)H * 0xD6E8FEB86659FD93ull);
  const unsigned char* p = reinterpret_cast<const unsigned char*>(emb);
  size_t bytes = n_floats * sizeof(float);
  for (; bytes >= 8; bytes -= 8, p += 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  if (bytes) {
    uint64_t w = 0;
    std::memcpy(&w, p, bytes);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  return h;
}

class HotwordBank {
 public:
  struct Entry {
    bool live = false;
    uint64_t hash = 0, stamp = 0;
    int H = 0, g0 = 0, ng = 0, pins = 0;
    std::vector<float> host;            // the set itself: confirms a hash hit, source of the upload
    // device side, managed by the owner: event recorded after the slab's projection, the stream it was recorded on, and
    // whether that work is known to be complete (no wait needed any more).  They stay with the entry id across reuse.
    void* ready = nullptr;
    const void* ready_on = nullptr;
    bool settled = false;
  };
  using HashFn = uint64_t (*)(const float*, size_t, int);
  HashFn hash_fn = hotword_hash;
  int64_t hits = 0, misses = 0, evictions = 0, refused = 0;

  // Drops every entry (the caller makes sure nothing is pinned) and sizes the arena: `granules` granules of `granule_rows` rows
  void configure(int granule_rows, int row_floats, int granules) {
    granule_ = granule_rows; d_ = row_floats; cap_ = granules < 0 ? 0 : granules;
    for (Entry& e : entries_) { e.live = false; e.pins = 0; e.host.clear(); e.host.shrink_to_fit(); }
    free_ids_.clear();
    for (int i = (int)entries_.size() - 1; i >= 0; --i) free_ids_.push_back(i);
    index_.clear();
    free_.clear();
    if (cap_ > 0) free_[0] = cap_;
    used_ = 0;
  }
  int granule_rows() const { return granule_; }
  int capacity_granules() const { return cap_; }
  int used_granules() const { return used_; }
  int pinned_entries() const { int n = 0; for (const Entry& e : entries_) n += e.live && e.pins > 0; return n; }
  int live_entries() const { int n = 0; for (const Entry& e : entries_) n += e.live; return n; }
  size_t id_count() const { return entries_.size(); }
  Entry& entry(int id) { return entries_[(size_t)id]; }
  int row_off(int id) const { return entries_[(size_t)id].g0 * granule_; }

  // The entry that holds this set, pinned; *hit says whether its slab already holds (or is being filled with) the set.
  // -1: no room (larger than the arena, or everything that would have to go is pinned).
  int acquire(const float* emb, int H, bool* hit) {
    const size_t n = (size_t)H * d_;
    const uint64_t h = hash_fn(emb, n, H);
    auto range = index_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it) {
      Entry& e = entries_[(size_t)it->second];
      if (e.H == H && std::memcmp(e.host.data(), emb, n * sizeof(float)) == 0) {
        ++e.pins; e.stamp = ++clock_; ++hits;
        if (hit) *hit = true;
        return it->second;
      }
    }
    if (hit) *hit = false;
    const int need = (H + granule_ - 1) / granule_;
    if (granule_ <= 0 || need > cap_) { ++refused; return -1; }
    int evictable = 0;
    for (const Entry& e : entries_) if (e.live && e.pins == 0) evictable += e.ng;
    if (cap_ - used_ + evictable < need) { ++refused; return -1; }
    int g0 = alloc(need);
    while (g0 < 0) {
      const int victim = lru_unpinned();
      if (victim < 0) { ++refused; return -1; }          // free room exists but the pinned slabs split it
      evict(victim);
      g0 = alloc(need);
    }
    int id;
    if (!free_ids_.empty()) { id = free_ids_.back(); free_ids_.pop_back(); }
    else { id = (int)entries_.size(); entries_.emplace_back(); }
    Entry& e = entries_[(size_t)id];
    e.live = true; e.hash = h; e.H = H; e.g0 = g0; e.ng = need; e.pins = 1; e.stamp = ++clock_;
    e.host.assign(emb, emb + n);
    e.ready_on = nullptr; e.settled = false;
    index_.emplace(h, id);
    ++misses;
    return id;
  }
  void release(int id) {
    Entry& e = entries_[(size_t)id];
    if (e.live && e.pins > 0) --e.pins;
  }
  // An entry whose slab could not be filled after all (the upload failed): it must not be found again.  The caller's pin is its
  // only one — nobody else can have found it while the owner's mutex was held.
  void discard(int id) {
    Entry& e = entries_[(size_t)id];
    if (!e.live) return;
    e.pins = 0;
    evict(id);
    --evictions;
  }

 private:
  int alloc(int need) {                       // first fit
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second < need) continue;
      const int g0 = it->first, rest = it->second - need;
      free_.erase(it);
      if (rest > 0) free_[g0 + need] = rest;
      used_ += need;
      return g0;
    }
    return -1;
  }
  void give_back(int g0, int ng) {            // coalesces with both neighbours
    auto next = free_.lower_bound(g0);
    if (next != free_.begin()) {
      auto prev = std::prev(next);
      if (prev->first + prev->second == g0) { g0 = prev->first; ng += prev->second; free_.erase(prev); }
    }
    if (next != free_.end() && g0 + ng == next->first) { ng += next->second; free_.erase(next); }
    free_[g0] = ng;
  }
  int lru_unpinned() const {
    int best = -1;
    for (size_t i = 0; i < entries_.size(); ++i) {
      const Entry& e = entries_[i];
      if (e.live && e.pins == 0 && (best < 0 || e.stamp < entries_[(size_t)best].stamp)) best = (int)i;
    }
    return best;
  }
  void evict(int id) {
    Entry& e = entries_[(size_t)id];
    auto range = index_.equal_range(e.hash);
    for (auto it = range.first; it != range.second; ++it)
      if (it->second == id) { index_.erase(it); break; }
    give_back(e.g0, e.ng);
    used_ -= e.ng;
    e.live = false;
    e.host.clear();
    free_ids_.push_back(id);
    ++evictions;
  }

  int granule_ = 0, d_ = 0, cap_ = 0, used_ = 0;
  uint64_t clock_ = 0;
  std::vector<Entry> entries_;
  std::vector<int> free_ids_;
  std::unordered_multimap<uint64_t, int> index_;
  std::map<int, int> free_;                   // first granule -> run length
};

}  // namespace pfhip_impl
