// Stand-alone check of the CIF time-stamp rule (timestamp.cpp CifTimestamps / CifTimestampSpans): the known answers and the
// error cases of pfhip_cif_timestamps, with no device and no library.  Meant for a sanitizer build (make timestamp_selftest):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all host/timestamp.cpp host/timestamp_selftest.cpp
// The buffers are heap blocks of exactly the size the call may touch, so an overrun by one element is a report.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "timestamp.h"

using namespace pfhip_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Want { float b, e; bool sil; };

static void expect(const std::vector<int>& fires, int n_chars, int n_frames, float frame_ms, float begin_ms, const std::vector<Want>& want) {
  std::unique_ptr<int[]> f(new int[fires.size()]);                       // exactly n_fires ints
  for (size_t i = 0; i < fires.size(); ++i) f[i] = fires[i];
  std::unique_ptr<float[]> spans(new float[3 * want.size()]);            // exactly the spans it needs
  int n = -1;
  const CifStampStatus st = CifTimestampSpans(f.get(), (int)fires.size(), n_chars, n_frames, frame_ms, begin_ms, spans.get(), (int)want.size(), &n);
  CHECK(st == kCifOk);
  CHECK(n == (int)want.size());
  for (int i = 0; st == kCifOk && i < n && i < (int)want.size(); ++i) {
    CHECK(std::fabs(spans[3 * i] - want[i].b) < 1e-6f);
    CHECK(std::fabs(spans[3 * i + 1] - want[i].e) < 1e-6f);
    CHECK((spans[3 * i + 2] != 0.f) == want[i].sil);
  }
  if (!want.empty()) {                                                   // one span less of room: the count comes back, nothing is written past
    std::unique_ptr<float[]> small(new float[3 * (want.size() - 1) + 1]);
    int m = -1;
    CHECK(CifTimestampSpans(f.get(), (int)fires.size(), n_chars, n_frames, frame_ms, begin_ms, small.get(), (int)want.size() - 1, &m) == kCifCapacity);
    CHECK(m == (int)want.size());
  }
}

int main() {
  // the header's known answer
  expect({4, 9, 30, 33, 40}, 4, 40, 60.f, 0.f,
         {{0.f, .30f, false}, {.30f, .60f, false}, {.60f, 1.26f, true}, {1.26f, 1.86f, false}, {1.86f, 2.04f, false}, {2.04f, 2.40f, true}});
  // a gap of exactly maxtok = 10 rows: no <sil>; of 11: one row of <sil>
  expect({4, 14}, 2, 15, 60.f, 0.f, {{0.f, .30f, false}, {.30f, .90f, false}});
  expect({4, 15}, 2, 16, 60.f, 0.f, {{0.f, .30f, false}, {.30f, .36f, true}, {.36f, .96f, false}});
  // a trailing row is absorbed, two are <sil>
  expect({4, 8}, 2, 10, 60.f, 0.f, {{0.f, .30f, false}, {.30f, .60f, false}});
  expect({4, 8}, 2, 11, 60.f, 0.f, {{0.f, .30f, false}, {.30f, .54f, false}, {.54f, .66f, true}});
  // two fires in one row: a zero-length token
  expect({3, 3, 6}, 3, 7, 60.f, 0.f, {{0.f, .24f, false}, {.24f, .24f, false}, {.24f, .42f, false}});
  // the VAD segment's offset
  expect({4, 8}, 2, 10, 60.f, 1500.f, {{1.5f, 1.80f, false}, {1.80f, 2.10f, false}});
  // every token fired by the tail slot of a one-row utterance; fire frames outside the utterance stay inside it
  expect({1}, 1, 1, 60.f, 0.f, {{0.f, .06f, false}});
  expect({-5, 1000}, 2, 3, 60.f, 0.f, {{0.f, 0.f, false}, {0.f, .18f, false}});
  // no characters: no spans, no buffer needed
  int n = -1;
  CHECK(CifTimestampSpans(nullptr, 0, 0, 40, 60.f, 0.f, nullptr, 0, &n) == kCifOk && n == 0);
  const int two[2] = {4, 9};
  CHECK(CifTimestampSpans(two, 2, 0, 40, 60.f, 0.f, nullptr, 0, &n) == kCifOk && n == 0);
  // refused
  float room[3 * 8];
  CHECK(CifTimestampSpans(two, 2, 3, 40, 60.f, 0.f, room, 8, &n) == kCifBadArg);        // more characters than fires
  CHECK(CifTimestampSpans(two, -1, 0, 40, 60.f, 0.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, -1, 40, 60.f, 0.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, -1, 60.f, 0.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, 40, 0.f, 0.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, 40, 60.f, -1.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, 40, 60.f, 0.f, room, -1, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(nullptr, 2, 2, 40, 60.f, 0.f, room, 8, &n) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, 40, 60.f, 0.f, room, 8, nullptr) == kCifBadArg);
  CHECK(CifTimestampSpans(two, 2, 2, 40, 60.f, 0.f, nullptr, 8, &n) == kCifCapacity && n == 3);
  std::printf(failures ? "timestamp_selftest: %d FAILED\n" : "timestamp_selftest OK\n", failures);
  return failures ? 1 : 0;
}
