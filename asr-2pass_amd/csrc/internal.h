// Internal definitions shared by the offline path (pfhip.cpp and the files behind offline.h) and stream.cpp (chunk-streaming forward).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pfhip.h"
#include "kernels.h"
#include "weights.h"
#include "hotword_bank.h"
#include "graph_bank.h"
#include "merge_queue.h"

namespace pfhip_impl {

std::string& last_error();          // thread-local, defined in pfhip.cpp

inline pfhip_status fail(pfhip_status st, const std::string& msg) {
  last_error() = msg;
  return st;
}

// The sample formats audio arrives in.  f32: samples in [-1, 1) as Model::Forward gets them.  s16: 16-bit PCM as the server receives
// it; the sample s stands for the float s / 32768.f (audio.cpp:787-857 divide exactly so), which is exact, and so is the x 32768 the
// front end applies again (paraformer.cpp:312-314) — the s16 kernels therefore give bit for bit what the f32 kernels give.
// PcmView: one buffer (host or device); HostPcm: a call's array of per-utterance host buffers, all of one format.
struct PcmView {
  const void* p; bool s16;
  const float* f32() const { return static_cast<const float*>(p); }
  const int16_t* i16() const { return static_cast<const int16_t*>(p); }
  size_t sample_bytes() const { return s16 ? 2 : 4; }
};
struct HostPcm {
  const void* const* p; bool s16;
  HostPcm(const float* const* f) : p(reinterpret_cast<const void* const*>(f)), s16(false) {}
  HostPcm(const int16_t* const* i) : p(reinterpret_cast<const void* const*>(i)), s16(true) {}
  HostPcm(const void* const* v, bool is_s16) : p(v), s16(is_s16) {}
  size_t sample_bytes() const { return s16 ? 2 : 4; }
};
// n samples of `src` as floats: a copy, or s / 32768.f (the streaming families convert during the one copy they make anyway)
inline void pcm_to_f32(float* dst, PcmView src, size_t n) {
  if (!src.s16) { if (n) std::memcpy(dst, src.p, n * 4); return; }
  const int16_t* s = src.i16();
  for (size_t i = 0; i < n; ++i) dst[i] = (float)s[i] / 32768.f;
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess)                                                                   \
      return pfhip_impl::fail(PFHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~Buf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    bytes = (bytes + (1u << 20) - 1) & ~((size_t)(1u << 20) - 1);
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  float* f() const { return static_cast<float*>(p); }
  int* i() const { return static_cast<int*>(p); }
};

// Pinned host staging, grown on demand to twice the request (callers have no copy in flight from the old block: every forward ends
// with a sync); freed by its destructor.
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    hipError_t e = hipHostMalloc(&p, bytes * 2, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes * 2;
    return e;
  }
  int* i() const { return static_cast<int*>(p); }
};

pfhip_status build_frontend_tables(int n_mels, int sample_rate, FrontendTables* ft);   // model_build.cpp

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// A linear layer repacked for the GEMM kernels: W zero-padded to [ceil(N/128)*128][ceil(K/32)*32], bias to the
// padded N, so pad outputs are exact zeros (odd widths: FSMN-VAD 140/250/248, punctuation head 6).
struct PackedLin { DevMem w, b; int N = 0, K = 0, Np = 0, Kp = 0; float ws = 1.0f; };
inline pfhip_status pack_linear(const float* w, const float* bias, int N, int K, PackedLin* out) {
  out->N = N; out->K = K; out->Np = round_up(N, 128); out->Kp = round_up(K, 32);
  std::vector<float> pw((size_t)out->Np * out->Kp, 0.f), pb((size_t)out->Np, 0.f);
  for (int n = 0; n < N; ++n) std::memcpy(&pw[(size_t)n * out->Kp], w + (size_t)n * K, sizeof(float) * K);
  if (bias) std::memcpy(pb.data(), bias, sizeof(float) * N);
  float mx = 0.f;
  for (float v : pw) mx = std::max(mx, std::fabs(v));
  out->ws = pfhip::best_w_scale(mx);
  HIP_TRY(out->w.upload(pw));
  HIP_TRY(out->b.upload(pb));
  return PFHIP_OK;
}
inline void lin_gemm(hipStream_t s, const PackedLin& l, const float* A, int lda, float* C, int ldc, const float* R1, int ldr1,
                     const float* R2, int ldr2, int M, bool relu) {
  pfhip::launch_gemm({.A = A, .lda = lda, .W = l.w.f(), .ldw = l.Kp, .C = C, .ldc = ldc, .M = M, .N = l.Np, .K = l.Kp, .bias = l.b.f(),
                      .R1 = R1, .ldr1 = ldr1, .R2 = R2, .ldr2 = ldr2, .relu = relu, .w_scale = l.ws},
                     pfhip::GemmKernel::BySize, false, s);
}

struct ProfRec { int cls; hipEvent_t e0, e1; };

// ---- resampling ahead of the front end (resample.cpp / resample.hip) -------------------------------------------------
// The polyphase plan of one rate pair on the host: Q output phases per unit of P input samples, per phase its first input
// index, tap count and weight row ([Q][K], rows zero-padded past ntap).
struct ResamplePlan {
  int P = 0, Q = 0, K = 0;
  std::vector<int32_t> first, ntap;
  std::vector<float> w;
};
// both rates in [1000, 192000] Hz and lcm(fs_in, fs_out) within int32; otherwise false and a message in *why
bool resample_supported(int fs_in, int fs_out, std::string* why);
int64_t resample_out_len(int fs_in, int fs_out, int64_t n_in);     // flush-mode output count, -1 for an unsupported pair
void build_resample_plan(int fs_in, int fs_out, ResamplePlan* p);
// Device images of the plans, uploaded once per (device, rate pair) and kept until the cache dies; safe for concurrent callers.
class ResampleCache {
 public:
  pfhip_status get(int device, int fs_in, int fs_out, pfhip::ResampleTable* out);
 private:
  struct Plan { DevMem first, ntap, w; pfhip::ResampleTable t; };
  std::mutex mu;
  std::map<std::tuple<int, int, int>, Plan> plans;
};

}  // namespace pfhip_impl

using pfhip_impl::Buf;
using pfhip_impl::Config;
using pfhip_impl::ModelWeights;
using pfhip_impl::PinBuf;
using pfhip_impl::ProfRec;

struct BatchReq;
struct StreamReq;
namespace pfhip_impl { struct NarBias; }

namespace pfhip_impl {
// The hotword bank of one device (on the weight owner; its contexts share it as they share the weights): the bias decoder's
// projected K/V rows [rows][2d] of many hotword sets in one arena, addressed by row offset, so that one attention launch takes one
// K base and one V base plus per-utterance offsets / counts.  hotword_bank.h keeps the books; `mu` covers them AND the enqueue of a
// miss's upload + projection + ready event, so that whoever finds the entry afterwards finds its event recorded.
struct HwBankDev {
  std::mutex mu;
  HotwordBank bank;
  float* arena = nullptr;
  bool configured = false;
  int64_t bound_bytes = -1;           // -1: PFHIP_HOTWORD_BANK_MB (default 64) at first use
  int default_id = -1;                // the entry of the pfhip_set_hotwords set, pinned for as long as it is the default
  int64_t forwards = 0, sets_total = 0, sets_max = 0, percall_forwards = 0;
};
// The graph bank of one device (on the weight owner, shared by its contexts): packed images of hotword context graphs (ctx_graph.h)
// in one arena, found again by content.  graph_bank.h keeps the books.  `mu` covers them AND the enqueue of a miss's fill + ready
// event, so that whoever finds the entry afterwards finds its event recorded.
struct GraphBankDev {
  std::mutex mu;
  HotwordBank bank;
  char* arena = nullptr;
  bool configured = false;
  int64_t bound_bytes = -1;           // -1: PFHIP_CTX_GRAPH_BANK_MB (default 16) at first use
};
}  // namespace pfhip_impl

namespace pfhip_impl {
// The token n-gram language model of a handle (pfhip_set_token_lm): the packed image of an lm_graph.h automaton in device memory this
// object owns, and the view the searches take (kernels.h).  Immutable once built; a forward holds a reference for its length.
struct TokenLm {
  DevMem image;
  pfhip::LmGraphDev dev;
};
}  // namespace pfhip_impl

namespace pfhip_impl {
// a number no other handle of the process ever had: what a thread's note of "my last forward ran there" is matched on (an address
// can be that of a handle destroyed since)
inline uint64_t next_model_uid() { static std::atomic<uint64_t> n{0}; return ++n; }
}  // namespace pfhip_impl

struct pfhip_model {
  const uint64_t uid = pfhip_impl::next_model_uid();
  int device = 0;
  hipStream_t own_stream = nullptr;
  // decoder K/V projections of a large batch run beside the (under-filled) token-side launches: forward.cpp enqueue_locked
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_enc_ready = nullptr;
  std::vector<hipEvent_t> ev_kv;
  std::mutex mu;
  // everything that is read-only after load, shared by the weight owner and its contexts (weights.h); the last of them frees it
  std::shared_ptr<const ModelWeights> weights;
  // guard of the fp16 two-plane domain (heads.cpp fetch_locked): the forward's flag word (inside `meta`, cleared by the metadata
  // upload), its pinned host mirror, what a re-run on the exact kernels needs, and the count of such re-runs
  int* d_range_flag = nullptr;
  PinBuf h_flag;
  int range_hit = 0, debug_range_flag = 0;
  bool exact_rerun = false, last_feats_only = false;
  long long range_fallbacks = 0;
  pfhip_impl::PcmView last_pcm{nullptr, false};               // the device buffer AND its sample format
  std::vector<int64_t> last_off;
  std::vector<int> last_n;
  int plane_forwards = 0;                                       // forwards of this context that took the plane path (debug read-out)
  Buf ctxP, xP, hP;                                             // activation plane images of a large batch: context, residual stream, FFN hidden
  Buf kvP;                                                      // K | V of an encoder layer as row-major fp16 planes (attention_p3.hip)
  int kvplane_forwards = 0;                                     // forwards whose encoder attention took K | V as planes (debug read-out)
  Buf encP, xdP;                                                // decoder on plane operands: images of the encoder output and of the token-side residual stream
  int dec_plane_forwards = 0;                                   // forwards whose decoder took the plane path (debug read-out)

  // workspace
  Buf pcm, meta, feats, x0, x, y, qkv, mem, ctx, hbuf, enc, alphas, counts;
  Buf emb, xd, yd, hd, hd2, td, t2, qd, ctxd, logits, logp, ids, dmeta, cat, hw, hwkv;
  Buf sseg;                     // StreamSeg descriptors of a streaming batch
  Buf rs_in;                    // audio at the caller's rate, resampled into `pcm` (pfhip_offline_forward_rate, pfhip_resample)
  // resampling plans of this device (on the weight owner; contexts use their owner's)
  std::unique_ptr<pfhip_impl::ResampleCache> rs_cache{new pfhip_impl::ResampleCache};
  Buf kvside;                   // [dec_layers][Mp][2d]: every decoder layer's K/V projection of the encoder output (side stream)
  Buf lnstats2;                 // the decoder's second hand-off (FFN1 -> ffn_norm -> FFN2): [ML][dec_ffn / 128][2]
  Buf lnstats;                  // per-row LayerNorm statistics handed from a producing GEMM's epilogue to the consumer [M][4][2]
  Buf kvall;                    // one window's K/V projections of every decoder layer [32][layers * 2d]
  Buf fbk, d_ops;               // streaming batch: fbank frames of all connections, operation descriptors
  PinBuf h_ops;                 // pinned staging of the same (+ the batch's PCM)
  Buf ts_up, ts_gx, ts_y, ts_hx, ts_a2, ts_alphas, ts_peaks, ts_meta, ts_cst;
  bool have_ts = false;
  int debug_blstm_flag = 0;        // pfhip_debug_poke
  hipStream_t blstm_stream = nullptr;      // per DEVICE (on the weight owner): every context's persistent recurrence runs here, in turn
  hipEvent_t ev_ts_in = nullptr, ev_ts_out = nullptr;
  bool ts_persistent = false;              // the last timestamp head ran the persistent kernel: its error word is read with the results
  int blstm_fallbacks = 0;         // timestamp requests served by the per-step recurrence after a barrier time-out
  // hotwords of the forward being run (resolve_hotwords_locked): per utterance the first row and the row count of its set's
  // K/V rows under fw_hwkv — the device's bank arena, or this context's `hwkv` when a set did not fit the bank — and the bank
  // entries this forward has pinned
  std::vector<int> fw_hw_off, fw_hw_len, fw_pins;
  const float* fw_hwkv = nullptr;
  std::unique_ptr<pfhip_impl::HwBankDev> hwbank{new pfhip_impl::HwBankDev};      // on the weight owner
  PinBuf h_meta, h_counts;      // pinned: the metadata uploads (two halves), the token counts [2*B]

  // state of the last forward
  int B = 0, M = 0, ML = 0, maxT = 0, maxL = 0;
  std::vector<int> T, row_off, n_fires, token_num, tok_off;
  bool have_logp = false;
  // N-best candidates (topk.hip): k of the forward being run (0 = the arg-max kernel alone, as ever), the [token rows, k] id and
  // value buffers the head fills, the k the device-pointer form asks for (pfhip_set_nbest) and the max_tokens of its last fetch
  int nbest_k = 0, nbest_enqueue_k = 0, nbest_fetch_max_tokens = 0;
  Buf nb_ids, nb_logp;
  // pfhip_offline_forward_bias: the search of the forward being run over its candidates (null: none; set for the length of the call
  // by forward_direct, so a range-guard re-run reads it again).  nbest_k is then at least the largest width in use.  bias_ws: the
  // front block (beam_front.h) and the trie nodes; bias_stage: the pinned staging of the front block's one copy; bias_res / h_bias:
  // the results on the device and on the host (n_hyp [B] | n_tokens [B][nb] | ids [B][nb][bias_mt] | score, am, ctx [B][nb]), which
  // cross with the forward's other results in front of fetch_once's synchronise
  const pfhip_impl::NarBias* bias = nullptr;
  // pfhip_set_token_lm: on the handle the caller holds, the model every search of its forwards walks (null: none), under lm_mu; on
  // the executing slot, fw_lm: the model of the forward being run (a range-guard re-run reads it again) and, of the last forward that
  // searched with one, each hypothesis's share of the total [B][beam_lm_stride] on the device with every utterance's nbest (0: it did
  // not search) — what pfhip_get_tensor "beam_lm_score" reads; beam_lm_stride 0: that forward had no model
  std::mutex lm_mu;
  std::shared_ptr<const pfhip_impl::TokenLm> token_lm;
  const pfhip_impl::TokenLm* fw_lm = nullptr;
  Buf beam_lm;
  int beam_lm_stride = 0;
  std::vector<int> beam_lm_nbest;
  Buf bias_ws, bias_res;
  PinBuf bias_stage, h_bias;
  int bias_mt = 0;
  // Fire frames (cif.hip, the sibling kernel): whether the forward being run records them (a range-guard re-run reads it again), whether
  // the last forward did, and what the device-pointer forms ask for (pfhip_set_fire_frames; read on the handle the caller holds).  They
  // sit behind the token counts in `counts` — [2B | M + B], laid out like the CIF's staging rows: fire nf of utterance b at
  // row_off[b] + b + nf — and cross to the pinned `h_counts` in the one copy forward_cif makes and synchronises on anyway
  bool want_fires = false, have_fires = false;
  std::atomic<int> fires_enqueue{0};
  const int32_t* host_fires() const { return h_counts.i() + 2 * B; }
  // SenseVoice (cfg.svs): the prompt ids of the forward being run [B][4] (a range-guard re-run reads them again), whether the caller
  // wants full log-prob rows (the unfused head), the debug switch to the unfused head, the chunks the last unfused head ran, the
  // results of the last forward on the host (h_counts: token_num [B] | ids, tok_frame, tok_logp [B][maxT] | frame ids, logp [M])
  std::vector<int32_t> svs_prompt;
  float* svs_logp_host = nullptr;
  int debug_ctc_unfused = 0, svs_head_chunks = 0, svs_unfused_forwards = 0;
  // a merged batch (svs_api.cpp): per utterance the host buffer for its full log-prob rows, or null (empty: a lone caller, who asks
  // through svs_logp_host); the rows the unfused chunks of the last head covered (pfhip_debug_poke "svs_unfused_rows")
  std::vector<float*> svs_logp_rows;
  long long svs_unfused_rows = 0;
  Buf svs_ws, svs_frame, svs_logits, svs_logp;
  // pfhip_svs_align: the log-sum-exp of every row of the last forward [M] (either head writes it), whether that forward completed,
  // and the aligner's own buffers (metadata, emissions, back-pointers, results)
  Buf svs_lse, al_meta, al_E, al_ws, al_out;
  PinBuf al_host;
  bool svs_fwd_ok = false;
  uint64_t svs_serial = 0;       // counts this context's SenseVoice forwards: a thread's note of its last one is matched on it
  // pfhip_svs_forward_spans: per utterance of the forward being run whether its greedy tokens are aligned inside the forward (empty:
  // none are — pfhip_svs_forward; a range-guard re-run reads it again), the plan kernel's outputs (n_lab, lab_off [B] | e_off [B],
  // total: int64), and of the last head: the token slots per utterance of the span results, their first word in counts / h_counts
  // (tok_begin, tok_end, tok_logp [B][svs_span_mt] | score [B]; 0 slots = no spans were formed).  debug_span_cap: a test's
  // stand-in for PFHIP_SVS_SPAN_MAX_FLOATS (pfhip_debug_poke "svs_span_cap", 0 = the constant).
  std::vector<char> svs_span_want;
  Buf al_plan;
  int svs_span_mt = 0;
  size_t svs_span_word = 0;
  long long debug_span_cap = 0;
  // pfhip_svs_forward_beam: the beams of the forward being run (svs_beam_fb == 0: no search; a range-guard re-run reads them again),
  // its graph (the caller's, alive for the call), and of the last head: the k best columns of every row [M][svs_topk_k] (kept for
  // pfhip_get_tensor "ctc_topk_*"), the token slots per hypothesis and the first word of the search's results in counts / h_counts
  // (n_hyp [B] | n_tokens [B][nbest] | ids [B][nbest][svs_beam_mt] | score, ctc_score, ctx_score [B][nbest])
  int svs_beam_fb = 0, svs_beam_sb = 0, svs_beam_nbest = 0, svs_topk_k = 0, svs_beam_mt = 0;
  const pfhip_ctx_graph* svs_beam_graph = nullptr;
  size_t svs_beam_word = 0;
  Buf svs_topk_ids, svs_topk_logp, svs_beam_ws;
  // pfhip_svs_forward_beam_sets and merged beam callers: every utterance on its own beams and graph.  svs_beam_utt [B] (empty: the
  // one-set form above) with svs_beam_fb / _sb / _nbest the maxima over the searching utterances — the head's k, the node stride
  // and the hypothesis stride of the results; svs_beam_graphs is the table the descriptors' graph indices name, svs_graph_dev per
  // graph its image in the device's graph bank or null (then it goes up with the call, in front of the search's workspace),
  // svs_graph_pins the bank entries the forward holds until after its last synchronise (graph_bank.cpp).  svs_beam_stage: the
  // pinned staging of the copy that takes descriptors, table and unbanked images up (beam_front.h); svs_graph_stage / svs_graph_up:
  // the pinned and the device staging of the ONE copy that takes a forward's bank misses up.
  std::vector<pfhip::BeamUtt> svs_beam_utt;
  std::vector<const pfhip_ctx_graph*> svs_beam_graphs;
  std::vector<const void*> svs_graph_dev;
  std::vector<int> svs_graph_pins;
  PinBuf svs_beam_stage, svs_graph_stage;
  Buf svs_graph_up;
  std::unique_ptr<pfhip_impl::GraphBankDev> gbank{new pfhip_impl::GraphBankDev};      // on the weight owner
  int *m_feat_off = nullptr, *m_prompt = nullptr, *m_speech_len = nullptr;
  // device views into meta / dmeta
  int *m_frame_off = nullptr, *m_nframes = nullptr, *m_row_off = nullptr, *m_len = nullptr,
      *m_row_pos = nullptr, *m_row_len = nullptr;
  int64_t* m_sample_off = nullptr;
  int *m_tok_off = nullptr, *m_tok_len = nullptr, *m_src_row = nullptr, *m_hw_off = nullptr, *m_hw_len = nullptr;

  // cross-request batching (pfhip_set_batching): callers queue at the handle they hold (ONE queue for every execution slot of
  // the handle: contexts on this device, replicas on other devices); the caller at the front leads a merged forward on an idle
  // slot while the next one already gathers the next batch (merge_queue.h PoolQueue)
  pfhip_impl::PoolQueue<BatchReq, pfhip_model> bq;
  int batch_wait_us = 0, batch_max_utts = 32;
  long long format_splits = 0;              // on the head, under bq.mu: picks that left callers of the other sample format queued
  // the same for streaming calls: concurrent pfhip_stream_forward callers (one thread per connection) are merged
  pfhip_impl::MergeQueue<StreamReq> sq;
  int stream_wait_us = 0, stream_max = 128;
  std::atomic<int> live_streams{0};     // open pfhip_streams: a leader stops waiting once all of them have queued

  // profiling
  int prof_mask = 0;             // bit c set -> launches of kernel class c are bracketed by events
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  pfhip_profile prof{};
  hipStream_t prof_stream = nullptr;

  // in-process multi-GPU router (replicas only): the handle the caller holds is replica 0; `replicas` are full
  // models on the other devices of PFHIP_DEVICES / pfhip_create_group.  Offline calls go to the replica with the fewest calls
  // in flight, a new stream to the one with the fewest open streams (a connection stays on its device for life).
  std::vector<pfhip_model*> replicas;
  pfhip_model* group_head = nullptr;        // replica / context -> the handle the caller holds (nullptr on the head itself)
  std::atomic<int> inflight{0};
  std::atomic<int64_t> served_calls{0}, served_utts{0}, served_forwards{0};
  std::atomic<unsigned> rr{0};
  // Execution contexts (pfhip_set_inflight / PFHIP_INFLIGHT): further pfhip_model objects on THIS device that share the
  // `weights` of `weights_of` and own only a workspace, streams and events — the reference's one shared Ort::Session under many
  // decoder threads (paraformer.cpp:35-41,541).
  std::vector<pfhip_model*> contexts;       // on a device replica: its extra contexts (the replica itself is context 0)
  pfhip_model* weights_of = nullptr;        // on a context: whose weights it borrows
  int ctx_index = 0;
  int ctx_limit = 1;                        // on the head: contexts per device that take calls (pfhip_set_inflight)
  std::vector<pfhip_model*> slots;          // on the head: every execution slot of the handle, device-major round order; guarded by bq.mu
  // on the head: the default hotword set (pfhip_set_hotwords) of calls that bring none (pfhip_offline_enqueue,
  // pfhip_offline_forward_resident); guarded by bq.mu
  std::shared_ptr<const std::vector<float>> hw_default;
  bool hw_merge = false;                    // on the head: contextual callers join the merge queue (pfhip_set_hotword_merging)
  bool beam_merge = false;                  // on the head: SenseVoice beam callers join it (pfhip_svs_set_beam_merging); guarded by bq.mu

  // sets the device, waits for it, destroys contexts / replicas, events and streams; the members then free what they own
  ~pfhip_model();
};

namespace pfhip_impl {
inline pfhip_model* route_stream(pfhip_model* m) {
  pfhip_model* best = m;
  for (pfhip_model* r : m->replicas)
    if (r->live_streams.load() < best->live_streams.load()) best = r;
  return best;
}
}  // namespace pfhip_impl

namespace pfhip_impl {

struct Scope {
  pfhip_model* m; hipStream_t s; int cls; hipEvent_t e1 = nullptr;
  Scope(pfhip_model* m_, hipStream_t s_, int cls_, double flops, double bytes) : m(m_), s(s_), cls(cls_) {
    if (!((m->prof_mask >> cls) & 1)) return;
    if (m->ev_used + 2 > m->ev_pool.size()) {
      for (int i = 0; i < 256; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; m->ev_pool.push_back(e); }
    }
    hipEvent_t e0 = m->ev_pool[m->ev_used++];
    e1 = m->ev_pool[m->ev_used++];
    (void)hipEventRecord(e0, s);
    m->prof_recs.push_back({cls, e0, e1});
    m->prof.flops[cls] += flops;
    m->prof.bytes[cls] += bytes;
    m->prof.launches[cls] += 1;
  }
  ~Scope() { if (e1) (void)hipEventRecord(e1, s); }
};

enum { K_GEMM = 0, K_ATTN = 1, K_LN = 2, K_FSMN = 3, K_FBANK = 4, K_CIF = 5, K_HEAD = 6, K_OTHER = 7 };

// C = A L.w^T + L.b (+ R1 + R2)
inline void gemm(pfhip_model* m, hipStream_t s, const float* A, int lda, const Linear& L, int N, int K, int Ktrue,
          float* C, int ldc, const float* R1, int ldr1, const float* R2, int ldr2, int M, bool relu) {
  Scope sc(m, s, K_GEMM, 2.0 * M * (double)N * Ktrue, 4.0 * ((double)M * Ktrue + (double)N * Ktrue + (double)M * N));
  // N that is no multiple of the column tile AND a C too narrow for the tile's pad columns (d_model 320: N = 320 / 960 with ldc = N):
  // the bounds-checked epilogue.  The model's other shapes (N % 128 == 0, or the vocabulary with ldc = vocab_pad) keep the unguarded one.
  const bool guard = N % pfhip::kTileN != 0 && ldc < (N + pfhip::kTileN - 1) / pfhip::kTileN * pfhip::kTileN;
  pfhip::launch_gemm({.A = A, .lda = lda, .W = L.w, .ldw = K, .C = C, .ldc = ldc, .M = M, .N = N, .K = K, .bias = L.b, .R1 = R1, .ldr1 = ldr1,
                      .R2 = R2, .ldr2 = ldr2, .relu = relu, .w_scale = L.scale},
                     pfhip::GemmKernel::BySize, guard, s);
}
// A split-kernel GEMM (GemmKernel::SplitBySize) over M rows of the model's buffers.  op names A, C, ldc, N, K, the residuals
// (row stride d), relu, ln_colsum (the LayerNorm fold: four statistics pairs per row read from lnstats) and stats_out; every
// other field is filled here, over whatever the caller put there.
inline void split_gemm(hipStream_t s, const Linear& W, pfhip::GemmOp op, int M, int d, const float* lnstats) {
  op.lda = op.ldw = op.K; op.W = W.w; op.bias = W.b; op.w_scale = W.scale; op.M = M; op.ldr1 = op.ldr2 = d;
  op.ln_stats = op.ln_colsum ? lnstats : nullptr; op.ln_tiles = 4;
  pfhip::launch_gemm(op, pfhip::GemmKernel::SplitBySize, false, s);
}
// The matrices of an attention launch as the model lays them out; the caller adds segments, sizes, scale and what else it uses.
// Self-attention: Q | K | V in the columns of one [rows, 3d] buffer, context [rows, d].
inline pfhip::AttnOp qkv_attention(const float* qkv, int d, float* ctx) {
  return {.Q = qkv, .ldq = 3 * d, .K = qkv + d, .ldk = 3 * d, .V = qkv + 2 * d, .ldv = 3 * d, .O = ctx, .ldo = d};
}
// Cross-attention: Q [rows, d], K | V in columns 0 and d of a buffer of row stride ldkv, context [rows, d].
inline pfhip::AttnOp kv_attention(const float* q, int d, const float* kv, int ldkv, float* ctx) {
  return {.Q = q, .ldq = d, .K = kv, .ldk = ldkv, .V = kv + d, .ldv = ldkv, .O = ctx, .ldo = d};
}
inline void lnorm(pfhip_model* m, hipStream_t s, const float* x, int ldx, float* y, int ldy, const Norm& n, int M, int D, int Dout) {
  Scope sc(m, s, K_LN, 8.0 * M * D, 8.0 * M * D);
  pfhip::launch_layernorm(x, ldx, y, ldy, n.g, n.b, M, D, Dout, 1e-12f, s);
}

}  // namespace pfhip_impl
