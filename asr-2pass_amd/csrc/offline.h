// What the files of the offline path name across a file boundary: declarations and small shared structs, no data.
#pragma once
#include "internal.h"

namespace pfhip_impl {
// hotword sets of a call: n_sets sets (emb[k]: [n[k], d]) and, per utterance, which one it attends to (of_utt == nullptr: all set 0)
struct HwSets { const float* const* emb; const int* n; int n_sets; const int* of_utt; };
// pfhip_offline_forward_bias: per utterance the search's descriptor (first_beam = the width, 0: no search; graph: an index into
// graphs), checked by the caller with nbest_ctx_beam_check, which also gave the strides; k: the head's candidate count, at least the
// largest width; out: the caller's buffers
struct NarBias {
  const pfhip::BeamUtt* utt; const pfhip_ctx_graph* const* graphs; int n_graphs; int k, beam_stride, nbest_stride; pfhip_bias_out* out;
};
// the token n-gram language model of the handle the caller holds (pfhip_set_token_lm; token_lm.cpp), or null
std::shared_ptr<const TokenLm> token_lm_of(pfhip_model* slot_or_head);
}  // namespace pfhip_impl

// One caller in the cross-request queue of a handle (pfhip_model::bq; offline_api.cpp states the queue's rules).  A Paraformer handle
// queues pfhip_offline_forward callers (out, hw, dt), a SenseVoice handle pfhip_svs_forward[_spans] callers (lid .. spans); a handle
// is one or the other, so a queue never holds both.
struct BatchReq : pfhip_impl::MergeReqBase {
  pfhip_impl::HostPcm pcm{static_cast<const float* const*>(nullptr)}; const int* n; int batch; pfhip_out* out = nullptr;
  pfhip_impl::HwSets hw{nullptr, nullptr, 0, nullptr};          // the caller's hotword sets (contextual models)
  const pfhip_detail* dt = nullptr;                 // the caller's candidate / fire-frame buffers (pfhip_offline_forward_detail), or none
  // SenseVoice: prompt ids per utterance, the caller's buffers, and — filled by the leader — where the packed forward ran: the
  // context, its forward count then and the caller's first utterance in the packed batch (the note pfhip_svs_align matches)
  const int32_t *lid = nullptr, *textnorm = nullptr;
  pfhip_svs_out* sout = nullptr;
  pfhip_svs_align_out* spans = nullptr;
  // a beam caller (pfhip_svs_set_beam_merging): its sets, per utterance the set it searches with (null: all set 0 — the
  // pfhip_svs_forward_beam form) and its result buffers; topk_k comes back: the stride of the forward's k best columns
  const pfhip_svs_beam_opts* sets = nullptr; int n_sets = 0; const int32_t* set_of = nullptr;
  pfhip_svs_beam_out* bout = nullptr;
  int topk_k = 0;
  pfhip_model* ran_on = nullptr;
  uint64_t serial = 0;
  int u0 = 0;
  long long unfused_rows = 0;
  int company = 0;                                  // the callers the packed forward served, this one included
  pfhip_status st = PFHIP_OK; std::string err;
};

namespace pfhip_impl {

// ---- model_build.cpp ----
pfhip_status build_model(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                         pfhip_model** out);
pfhip_status build_context(pfhip_model* owner, pfhip_model** out);
pfhip_status read_file(const char* path, std::vector<char>& out);

// ---- forward.cpp ----
// Sets the calling thread's launch context (kernels.h) for the kernels of one forward of `m`: its range-flag word and whether this
// is the re-run on the exact kernels.
struct ForwardCtx {
  pfhip::LaunchCtx saved;
  explicit ForwardCtx(pfhip_model* m) : saved(pfhip::launch_ctx()) {
    pfhip::launch_ctx().exact = m->exact_rerun || m->weights->always_exact;
    pfhip::launch_ctx().range_flag = m->d_range_flag;
  }
  ~ForwardCtx() { pfhip::launch_ctx() = saved; }
};
pfhip_status enqueue_locked(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
                            int B, hipStream_t s, bool feats_only);

// ---- heads.cpp ----
struct SvsHost { const int32_t *num, *ids, *frames, *fid; const float *logp, *flp; };
SvsHost svs_host(const pfhip_model* m);
pfhip_status svs_head_locked(pfhip_model* m, hipStream_t s);
pfhip_status head_locked(pfhip_model* m, hipStream_t s, bool want_logp);
pfhip_status fetch_locked(pfhip_model* m, pfhip_out* out, hipStream_t s, const pfhip_detail* dt = nullptr);
void scatter_fires(const pfhip_model* m, int32_t* dst, int max_tokens);
// the first k of the m->nbest_k candidates of every token row, utterance b at row b * max_tokens of the caller's buffers; staged
// on the host like the ids (tok rows x k x 8 bytes)
struct NbestStage {
  std::vector<int32_t> ids; std::vector<float> logp;
  pfhip_status start(pfhip_model* m, hipStream_t s) {
    ids.resize((size_t)m->ML * m->nbest_k); logp.resize(ids.size());
    HIP_TRY(hipMemcpyAsync(ids.data(), m->nb_ids.p, ids.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(logp.data(), m->nb_logp.p, logp.size() * 4, hipMemcpyDeviceToHost, s));
    return PFHIP_OK;
  }
  void scatter(const pfhip_model* m, int k, int32_t* dst_ids, float* dst_logp, int max_tokens) const {      // after the synchronise
    const int kc = m->nbest_k;
    for (int b = 0; b < m->B; ++b)
      for (int t = 0; t < m->n_fires[b]; ++t) {
        const size_t src = ((size_t)m->tok_off[b] + t) * kc, dst = ((size_t)b * max_tokens + t) * k;
        std::memcpy(dst_ids + dst, ids.data() + src, 4 * (size_t)k);
        std::memcpy(dst_logp + dst, logp.data() + src, 4 * (size_t)k);
      }
  }
};

// ---- hotwords.cpp ----
void release_hotwords(pfhip_model* m);
struct HotwordPins {          // a forward's pins end with it, whichever way it ends (after its last synchronise)
  pfhip_model* m;
  ~HotwordPins() { release_hotwords(m); }
};
pfhip_status resolve_hotwords_locked(pfhip_model* m, const float* const* emb, const int* H, int n_sets, const int* set_of_utt, int B,
                                     hipStream_t s);
std::shared_ptr<const std::vector<float>> default_hotwords(pfhip_model* m);
pfhip_status resolve_default_hotwords_locked(pfhip_model* m, int B, hipStream_t s);

// ---- offline_api.cpp ----
bool is_svs(const pfhip_model* m);
pfhip_status refuse_svs();
pfhip_status stage_pcm(pfhip_model* m, HostPcm pcm, const int* n_samples, int B, hipStream_t s,
                       std::vector<int64_t>& off);
pfhip_status stage_resampled(pfhip_model* m, HostPcm pcm, const int* n_samples, int B, int fs_in, hipStream_t s,
                             std::vector<int64_t>& off, std::vector<int>& n_out);
pfhip_status forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch,
                            const HwSets& hw, pfhip_out* out, int fs_in = 0, const pfhip_detail* dt = nullptr, const NarBias* bias = nullptr);
pfhip_model*& last_replica();       // the calling thread's tl_last_replica
// the caller joins the handle's queue; `run` executes one packed forward for everybody taken.  The slot `me` led a batch on, or null
pfhip_model* pool_submit(pfhip_model* head, BatchReq& me, void (*run)(pfhip_model*, const std::vector<BatchReq*>&));

// ---- svs_api.cpp ----
// a packed forward for merged callers: per utterance whether its greedy tokens are aligned (null: all, when there is a span buffer)
// and the host buffer for its full log-prob rows (null: none); back come the context's forward count behind this forward and the
// rows its unfused head chunks covered
struct SvsMerge { const char* span_want = nullptr; float* const* logp_rows = nullptr; uint64_t serial = 0; long long unfused_rows = 0; int topk_k = 0; };
// the note of the calling thread's last forward on `head` (what pfhip_svs_align matches): the context it ran on — looked up among
// the handle's own, null if there is none —, that context's forward count then and the caller's utterances within that forward
struct SvsNoteView { pfhip_model* ctx = nullptr; uint64_t serial = 0; int u0 = 0, batch = 0; };
SvsNoteView svs_thread_note(pfhip_model* head);
int svs_last_topk_k();                  // the stride of the k best columns in the forward that served the calling thread (0: greedy)

// ---- graph_bank.cpp ----
pfhip_status svs_pin_graphs_locked(pfhip_model* m, hipStream_t s);
void svs_release_graphs(pfhip_model* m);
void destroy_graph_bank(pfhip_model* m);
long long svs_last_unfused_rows();      // of the forward that served the calling thread's last pfhip_svs_forward
int svs_last_forward_calls();           // the callers that forward served (1: a lone or direct call)
// pfhip_svs_forward_beam: the search's options and the caller's buffers (both set, or no search).  The sets form
// (pfhip_svs_forward_beam_sets, merged beam callers): utt [batch] gives every utterance its own beams and its graph as an index
// into graphs (first_beam 0: no search; checked by the caller with ctc_prefix_beam_multi_check); opts is not read, and out's
// hypothesis stride is the largest nbest among the searching utterances (1 if none).
struct SvsBeam {
  const pfhip_svs_beam_opts* opts = nullptr; pfhip_svs_beam_out* out = nullptr;
  const pfhip::BeamUtt* utt = nullptr; const pfhip_ctx_graph* const* graphs = nullptr; int n_graphs = 0;
};
pfhip_status svs_forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid,
                                const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans = nullptr, SvsMerge* mg = nullptr,
                                const SvsBeam* beam = nullptr);

// ---- pfhip.cpp: the execution slots ----
void rebuild_slots_locked(pfhip_model* head);
pfhip_model* acquire_slot(pfhip_model* head);
void release_slot(pfhip_model* head, pfhip_model* slot);
std::vector<pfhip_model*> all_slots(pfhip_model* head);

}  // namespace pfhip_impl
