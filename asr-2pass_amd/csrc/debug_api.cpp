// Warm-up, the front end alone, and the debug and profiling read-outs of an execution context.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "offline.h"

#define g_err (pfhip_impl::last_error())

using namespace pfhip_impl;

extern "C" {

// One synthetic batch through every execution slot: the code objects are loaded, each context's workspace is sized for
// `batch` utterances of `n_samples` samples and its streams have run once, so the first real request pays none of that.
pfhip_status pfhip_warm_up(pfhip_model* m, int batch, int n_samples) {
  g_err.clear();
  if (!m || batch <= 0 || n_samples <= 0 || batch > 1024 || n_samples > 16000 * 120) return fail(PFHIP_ERR_ARG, "bad argument");
  if (m->group_head || m->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  std::vector<float> pcm((size_t)n_samples);
  uint32_t lcg = 20251114u;
  for (int i = 0; i < n_samples; ++i) {
    lcg = lcg * 1664525u + 1013904223u;
    pcm[i] = 0.15f * sinf(0.0431969f * (float)i) + 0.1f * ((float)(lcg >> 8) / 8388608.f - 1.f);
  }
  std::vector<const float*> ptrs((size_t)batch, pcm.data());
  std::vector<int> lens((size_t)batch, n_samples);
  const int max_tok = n_samples / 960 + 2;
  std::vector<int32_t> ids((size_t)batch * max_tok), tn(batch), nf(batch), fr(batch);
  std::vector<float> hw(m->weights->cfg.contextual ? (size_t)m->weights->cfg.d_model : 0, 0.f);
  if (is_svs(m)) {
    std::vector<int32_t> lid((size_t)batch, 0), tnorm((size_t)batch, 15), sids((size_t)batch * (max_tok * 2 + 8));
    for (pfhip_model* r : all_slots(m)) {
      pfhip_svs_out so{};
      so.ids = sids.data(); so.token_num = tn.data(); so.max_tokens = max_tok * 2 + 8;
      const pfhip_status st = svs_forward_direct(r, ptrs.data(), lens.data(), batch, lid.data(), tnorm.data(), &so);
      if (st) return st;
    }
    return PFHIP_OK;
  }
  for (pfhip_model* r : all_slots(m)) {
    pfhip_out out{};
    out.token_ids = ids.data(); out.token_num = tn.data(); out.n_fires = nf.data(); out.n_frames = fr.data(); out.max_tokens = max_tok;
    const float* hwp = hw.empty() ? nullptr : hw.data();
    const int one = 1;
    const pfhip_status st = forward_direct(r, ptrs.data(), lens.data(), batch, HwSets{&hwp, &one, hw.empty() ? 0 : 1, nullptr}, &out);
    if (st) return st;
  }
  return PFHIP_OK;
}

pfhip_status pfhip_extract_feats(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch,
                                 float* feats_out, size_t feats_cap_floats, int32_t* n_frames_out) {
  g_err.clear();
  if (!m || !pcm || !n_samples || batch <= 0) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->own_stream;
  m->prof_stream = s;
  std::vector<int64_t> off;
  pfhip_status st = stage_pcm(m, pcm, n_samples, batch, s, off);
  if (st) return st;
  st = enqueue_locked(m, PcmView{m->pcm.p, false}, off.data(), n_samples, batch, s, true);
  if (st) return st;
  if (n_frames_out) for (int b = 0; b < batch; ++b) n_frames_out[b] = m->T[b];
  const size_t n = (size_t)m->M * m->weights->feat_dim;
  if (feats_out) {
    if (n > feats_cap_floats) return fail(PFHIP_ERR_CAPACITY, "feats_out too small");
    if (n) HIP_TRY(hipMemcpyAsync(feats_out, m->feats.p, n * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return PFHIP_OK;
}

pfhip_status pfhip_get_tensor(pfhip_model* m, const char* name, float* dst, size_t cap_floats, size_t* n_out) {
  g_err.clear();
  if (!m || !name || !dst) return fail(PFHIP_ERR_ARG, "bad argument");
  // a group: the replica that served this thread's last offline forward holds the state being asked for
  if (!m->replicas.empty() && last_replica() && (last_replica() == m || last_replica()->group_head == m)) m = last_replica();
  const std::string nm(name);
  // the k best columns after a MERGED forward are the calling thread's own utterances' rows: its note says which context served it
  // and which of that forward's utterances are its own (the rule of pfhip_svs_align); without a valid note: this handle's last forward
  SvsNoteView own;
  if (is_svs(m) && (nm == "ctc_topk_ids" || nm == "ctc_topk_logp" || nm == "beam_lm_score")) {
    own = svs_thread_note(m);
    if (own.ctx) m = own.ctx;
  }
  // a Paraformer's biased search ran on the slot that served this thread's last forward
  if (!is_svs(m) && nm == "beam_lm_score" && last_replica() && last_replica()->group_head == m) m = last_replica();
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->prof_stream ? m->prof_stream : m->own_stream;
  const void* src = nullptr;
  size_t n = 0;
  const int d = m->weights->cfg.d_model;
  // The language model's share of every hypothesis of the last search that walked one (pfhip_set_token_lm): [batch][stride] as the
  // search's own outputs are laid out — after a merged forward the calling thread's own utterances, on their own stride
  if (nm == "beam_lm_score") {
    if (!m->beam_lm_stride || (int)m->beam_lm_nbest.size() != m->B)
      return fail(PFHIP_ERR_ARG, "beam_lm_score: the last forward here searched without a token language model");
    int u0 = 0, nu = m->B;
    if (own.ctx == m && m->svs_fwd_ok && m->svs_serial == own.serial && own.u0 >= 0 && own.batch > 0 && own.u0 + own.batch <= m->B) {
      u0 = own.u0; nu = own.batch;
    }
    int stride = 1;
    for (int u = u0; u < u0 + nu; ++u) stride = std::max(stride, m->beam_lm_nbest[(size_t)u]);
    n = (size_t)nu * stride;
    if (n_out) *n_out = n;
    if (n > cap_floats) return fail(PFHIP_ERR_CAPACITY, "dst too small");
    const int fs = m->beam_lm_stride;
    std::vector<float> all((size_t)m->B * fs);
    HIP_TRY(hipMemcpyAsync(all.data(), m->beam_lm.p, all.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int u = 0; u < nu; ++u)
      for (int j = 0; j < stride; ++j) dst[(size_t)u * stride + j] = j < fs ? all[(size_t)(u0 + u) * fs + j] : 0.f;
    return PFHIP_OK;
  }
  if (nm == "feats") { src = m->feats.p; n = (size_t)m->M * m->weights->feat_dim; }
  else if (nm == "enc") { src = m->weights->cfg.svs ? m->x.p : m->enc.p; n = (size_t)m->M * d; }      // SenseVoice: the rows after tp.norm
  else if (nm == "lse" && m->weights->cfg.svs) { src = m->svs_lse.p; n = (size_t)m->M; }             // the rows' log-sum-exp either CTC head kept
  // the k best columns of every row of the last pfhip_svs_forward_beam [M][first_beam]; the ids are int32 words in the float buffer
  else if ((nm == "ctc_topk_ids" || nm == "ctc_topk_logp") && m->weights->cfg.svs && m->svs_topk_k) {
    size_t r0 = 0, rows = (size_t)m->M;
    if (own.ctx == m && m->svs_fwd_ok && m->svs_serial == own.serial && own.u0 >= 0 && own.batch > 0 && own.u0 + own.batch <= m->B) {
      r0 = (size_t)m->row_off[own.u0];
      rows = (size_t)m->row_off[own.u0 + own.batch - 1] + (size_t)m->T[own.u0 + own.batch - 1] - r0;
    }
    src = static_cast<const char*>(nm == "ctc_topk_ids" ? m->svs_topk_ids.p : m->svs_topk_logp.p) + r0 * m->svs_topk_k * 4;
    n = rows * m->svs_topk_k;
  }
  else if (m->weights->cfg.svs) return fail(PFHIP_ERR_ARG, "a SenseVoice model has the tensors feats, enc and lse, not " + nm);
  else if (nm == "alphas") { src = m->alphas.p; n = (size_t)m->M; }
  else if (nm == "emb") { src = m->emb.p; n = (size_t)m->ML * d; }
  else if (nm == "ts_up" && m->have_ts) { src = m->ts_up.p; n = (size_t)3 * m->M * d; }            // timestamp-head stages
  else if (nm == "ts_gx" && m->have_ts) { src = m->ts_gx.p; n = (size_t)3 * m->M * 8 * d; }
  else if (nm == "ts_y" && m->have_ts) { src = m->ts_y.p; n = (size_t)3 * m->M * 2 * d; }
  else if (nm == "logp") {
    if (m->ML && !m->have_logp) { pfhip_status st = head_locked(m, s, true); if (st) return st; }
    src = m->logp.p; n = (size_t)m->ML * m->weights->cfg.vocab;
  }
  // the last forward's candidates [token rows][k] (k as it was computed); the ids are int32 words in the float buffer
  else if (nm == "nbest_ids" && m->nbest_k) { src = m->nb_ids.p; n = (size_t)m->ML * m->nbest_k; }
  else if (nm == "nbest_logp" && m->nbest_k) { src = m->nb_logp.p; n = (size_t)m->ML * m->nbest_k; }
  else if (nm == "fire_frame" && m->have_fires) {      // [token rows], compacted from the staged layout (on the host already) and converted: small integers
    if ((size_t)m->ML > cap_floats) return fail(PFHIP_ERR_CAPACITY, "dst too small");
    for (int b = 0; b < m->B && m->ML; ++b)
      for (int t = 0; t < m->n_fires[b]; ++t) dst[m->tok_off[b] + t] = (float)m->host_fires()[(size_t)m->row_off[b] + b + t];
    if (n_out) *n_out = (size_t)m->ML;
    return PFHIP_OK;
  }
  else return fail(PFHIP_ERR_ARG, "unknown tensor name " + nm);
  if (n > cap_floats) return fail(PFHIP_ERR_CAPACITY, "dst too small");
  if (n) HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n_out) *n_out = n;
  return PFHIP_OK;
}

// Test hook.  "blstm_flag" != 0: the next timestamp request finds the BLSTM error word raised (as after a step-barrier
// time-out) and must fall back to the per-step recurrence; "blstm_fallbacks" returns how often that happened (as the status).
pfhip_status pfhip_debug_poke(pfhip_model* m, const char* what, int value) {
  g_err.clear();
  if (!m || !what) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (std::string(what) == "blstm_flag") { m->debug_blstm_flag = value; return PFHIP_OK; }
  if (std::string(what) == "blstm_fallbacks") {     // read-out: how often the per-step form ran, over every context of the handle
    long long n = m->blstm_fallbacks;
    for (pfhip_model* cx : m->contexts) n += cx->blstm_fallbacks;
    for (pfhip_model* r : m->replicas) { n += r->blstm_fallbacks; for (pfhip_model* cx : r->contexts) n += cx->blstm_fallbacks; }
    return (pfhip_status)n;
  }
  if (std::string(what) == "plane_forwards") return (pfhip_status)m->plane_forwards;        // read-out: forwards on plane-image operands
  if (std::string(what) == "kvplane_forwards") return (pfhip_status)m->kvplane_forwards;     // ... whose attention took K | V as planes
  if (std::string(what) == "dec_plane_forwards") return (pfhip_status)m->dec_plane_forwards; // ... whose decoder took the plane path too
  if (std::string(what) == "static_bound") return (pfhip_status)std::min(m->weights->static_bound, 2.0e9);      // read-out: the load-time activation bound
  if (std::string(what) == "always_exact") return (pfhip_status)(m->weights->always_exact ? 1 : 0);
  if (std::string(what) == "format_splits") {         // read-out: merged batches cut short because callers of both sample formats were queued
    std::lock_guard<std::mutex> ql(m->bq.mu);
    return (pfhip_status)m->format_splits;
  }
  // SenseVoice.  A forward runs on whichever execution context is least loaded, so the switch is set on every context of the handle
  // (each one's next forward takes the unfused head once) and the counter is summed over them, as range_fallbacks is; the chunk
  // count is that of the context which served the calling thread's last forward.
  if (std::string(what) == "ctc_unfused" || std::string(what) == "ctc_unfused_forwards") {
    const bool set = std::string(what) == "ctc_unfused";
    long long n = 0;
    auto visit = [&](pfhip_model* x, bool locked) {
      std::unique_lock<std::mutex> xl(x->mu, std::defer_lock);
      if (!locked) xl.lock();
      if (set) x->debug_ctc_unfused = value;
      n += x->svs_unfused_forwards;
    };
    visit(m, true);
    for (pfhip_model* cx : m->contexts) visit(cx, false);
    for (pfhip_model* r : m->replicas) { visit(r, false); for (pfhip_model* cx : r->contexts) visit(cx, false); }
    return set ? PFHIP_OK : (pfhip_status)n;
  }
  if (std::string(what) == "svs_span_cap") {          // pfhip_svs_forward_spans: a small stand-in for PFHIP_SVS_SPAN_MAX_FLOATS, on every context
    m->debug_span_cap = value;
    for (pfhip_model* cx : m->contexts) { std::lock_guard<std::mutex> xl(cx->mu); cx->debug_span_cap = value; }
    return PFHIP_OK;
  }
  if (std::string(what) == "ctc_head_chunks") {
    // (looked up among this handle's contexts, never dereferenced before it is found there: the note may be of a handle since destroyed)
    for (pfhip_model* cx : m->contexts)
      if (cx == last_replica()) return (pfhip_status)cx->svs_head_chunks;
    return (pfhip_status)m->svs_head_chunks;
  }
  // the rows the unfused head chunks covered in the forward that served the calling thread's last pfhip_svs_forward (svs_api.cpp)
  if (std::string(what) == "svs_unfused_rows") return (pfhip_status)svs_last_unfused_rows();
  if (std::string(what) == "svs_forward_calls") return (pfhip_status)svs_last_forward_calls();      // ... and the callers that forward served
  if (std::string(what) == "svs_topk_k") return (pfhip_status)svs_last_topk_k();                    // ... and the stride of its k best columns
  if (std::string(what) == "range_flag") { m->debug_range_flag = value; return PFHIP_OK; }    // the next forward starts with its range flag raised
  if (std::string(what) == "range_fallbacks") {       // read-out: forwards redone on the exact kernels, over every context of the handle
    long long n = m->range_fallbacks;
    for (pfhip_model* cx : m->contexts) n += cx->range_fallbacks;
    for (pfhip_model* r : m->replicas) { n += r->range_fallbacks; for (pfhip_model* cx : r->contexts) n += cx->range_fallbacks; }
    return (pfhip_status)n;
  }
  return fail(PFHIP_ERR_ARG, std::string("unknown debug key ") + what);
}

pfhip_status pfhip_profile_enable(pfhip_model* m, int on) {
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  std::lock_guard<std::mutex> lk(m->mu);
  m->prof_mask = on < 0 ? 0 : (on == 1 ? 0xff : on);   // 0 off, 1 all classes, else a bit mask of classes << 0
  return PFHIP_OK;
}

pfhip_status pfhip_profile_read(pfhip_model* m, pfhip_profile* out, int reset) {
  g_err.clear();
  if (!m || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  if (m->prof_stream) HIP_TRY(hipStreamSynchronize(m->prof_stream));
  for (const ProfRec& r : m->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) m->prof.ms[r.cls] += ms;
  }
  m->prof_recs.clear();
  m->ev_used = 0;
  *out = m->prof;
  if (reset) m->prof = pfhip_profile{};
  return PFHIP_OK;
}

}  // extern "C"
