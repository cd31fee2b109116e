// Bookkeeping of the per-device bank of hotword context graphs (graph_bank.cpp): which packed graph images (ctx_graph.h `packed`)
// are resident in the device arena, where, and which may be overwritten.  Host code only — no HIP — so it is tested without a GPU
// (host/graph_bank_selftest.cpp).  The books are hotword_bank.h's (content hash plus byte compare, pin / release, least recently
// used among the unpinned, refusal when nothing fits) over rows of kGraphRowWords 32-bit words, one row a granule: an image is
// padded with zeros to whole rows, and the row count is part of the key, so an image and its zero-extended twin are two entries.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "hotword_bank.h"

namespace pfhip_impl {

constexpr int kGraphRowWords = 64;
constexpr size_t kGraphRowBytes = (size_t)kGraphRowWords * 4;

inline int graph_bank_rows(size_t words) { return (int)((words + kGraphRowWords - 1) / kGraphRowWords); }
// drops every entry and sizes the arena to whole rows within `bytes`
inline void graph_bank_configure(HotwordBank& bank, int64_t bytes) {
  const int64_t rows = bytes <= 0 ? 0 : bytes / (int64_t)kGraphRowBytes;
  bank.configure(1, kGraphRowWords, (int)(rows > INT32_MAX / 2 ? INT32_MAX / 2 : rows));
}
// HotwordBank::acquire for an image of `words` 32-bit words (> 0); `scratch` holds the padded copy the books compare and keep
inline int graph_bank_acquire(HotwordBank& bank, const int32_t* packed, size_t words, bool* hit, std::vector<float>* scratch) {
  const int rows = graph_bank_rows(words);
  scratch->assign((size_t)rows * kGraphRowWords, 0.f);
  std::memcpy(scratch->data(), packed, words * 4);
  return bank.acquire(scratch->data(), rows, hit);
}
inline size_t graph_bank_offset(const HotwordBank& bank, int id) { return (size_t)bank.row_off(id) * kGraphRowBytes; }

}  // namespace pfhip_impl
