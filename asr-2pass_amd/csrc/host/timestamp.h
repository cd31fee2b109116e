// Token time stamps from the upsampled CIF outputs — behaviourally `funasr::TimestampOnnx`
// (onnxruntime/src/util.cpp:838-963): peaks of us_cif_peak (> 1 - 1e-4) are token boundaries on a 20-ms grid
// (TIME_RATE = 10*6/1000/3 s, :851); when their count is not tokens+1 the peaks are re-derived from the rescaled
// us_alphas (:872-904); long gaps are split into token + <sil> (:918-928); leading / trailing silence (:911-915,
// :936-943).  Host post-processing that consumes two extra model outputs.
#pragma once
#include <vector>

namespace pfhip_host {

struct TimeSpan { float begin_s; float end_s; bool is_sil; };

// n_chars = recognised tokens WITHOUT a trailing "</s>" (the reference pops it, :856-858).  us_alphas is rescaled in
// place like the reference's by-reference parameter.  Returns every span incl. <sil>; the caller keeps the non-sil
// ones as the token stamps (:957-961).
std::vector<TimeSpan> TimestampOnnx(std::vector<float>& us_alphas, const std::vector<float>& us_cif_peak, int n_chars,
                                    float begin_time_ms = 0.0f, float total_offset = -1.5f);

// Token spans from the fire frames of the CIF scan (an extension; the reference has no counterpart: the head behind TimestampOnnx,
// paraformer.cpp:545, is its only source of stamps).  fire_frame[k] = the LFR row token k fired in (n_frames for the tail slot), the
// first n_chars of them are stamped; frame_ms = one LFR row.  No constants of its own: TimestampOnnx's MAX_TOKEN_DURATION (30 x 20 ms)
// and START_END_THRESHOLD (5 x 20 ms) as times.  In frames, e[-1] = 0, maxtok = 600 / frame_ms:
//   e[k] = min(fire_frame[k] + 1, n_frames);  b[k] = max(e[k-1], e[k] - maxtok);  b[k] > e[k-1]: <sil> [e[k-1], b[k]], then token [b[k], e[k]]
//   after the last token: (n_frames - e[last]) * frame_ms > 100 -> <sil> [e[last], n_frames], else the last token ends at n_frames
// n_frames = 40, 60 ms, fires {4, 9, 30, 33, 40}, n_chars = 4 ->
//   [0, .30] [.30, .60] <sil> [.60, 1.26] [1.26, 1.86] [1.86, 2.04] <sil> [2.04, 2.40]
// The caller has checked 0 <= n_chars <= the fires it passes, n_frames >= 0 and frame_ms > 0.
std::vector<TimeSpan> CifTimestamps(const int* fire_frame, int n_chars, int n_frames, float frame_ms, float begin_time_ms = 0.0f);
// The same behind the argument checks of the C entry (pfhip_cif_timestamps): (begin_s, end_s, is_sil) triplets into spans[3 * cap],
// *n_spans = the count (also where cap is too small).  kCifBadArg: a negative argument, n_chars > n_fires, frame_ms <= 0, a NULL
// pointer that is needed.
enum CifStampStatus { kCifOk = 0, kCifBadArg = 1, kCifCapacity = 2 };
CifStampStatus CifTimestampSpans(const int* fire_frame, int n_fires, int n_chars, int n_frames, float frame_ms, float begin_time_ms,
                                 float* spans, int cap, int* n_spans);

}  // namespace pfhip_host
