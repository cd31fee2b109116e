// SenseVoiceSmall, offline: the packed forward with its range-guard re-run, and CTC forced alignment against its rows.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "offline.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

// pfhip_svs_align: per handle (its uid), where this thread's last pfhip_svs_forward on it ran — the context's uid and that context's
// forward count then.  Handles come and go; the note is emptied when it has grown past 64 handles.
struct SvsNote { uint64_t ctx_uid, serial; };
thread_local std::map<uint64_t, SvsNote> tl_svs_notes;

pfhip_status svs_forward(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid, const int32_t* textnorm,
                                pfhip_svs_out* out) {
  g_err.clear();
  if (!head || !pcm.p || !n_samples || batch <= 0 || !lid || !textnorm || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(head)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: a Paraformer is run through pfhip_offline_forward");
  if (!head->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "multi-device groups are not built for SenseVoice (CTC) models");
  for (int b = 0; b < batch; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm.p[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    if (lid[b] < 0 || lid[b] > 15 || textnorm[b] < 0 || textnorm[b] > 15) return fail(PFHIP_ERR_ARG, "lid / textnorm outside 0..15");
  }
  pfhip_model* m = acquire_slot(head);                  // the least-loaded execution context
  last_replica() = m;
  const pfhip_status st = svs_forward_direct(m, pcm, n_samples, batch, lid, textnorm, out);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}

}  // namespace

namespace pfhip_impl {

// one packed forward on slot m, its range-guard re-run included, and the results into out
pfhip_status svs_forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid,
                                       const int32_t* textnorm, pfhip_svs_out* out) {
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->own_stream;
  m->prof_stream = s;
  const int V = m->weights->cfg.vocab;
  m->nbest_k = 0; m->want_fires = false;
  m->svs_fwd_ok = false;
  ++m->svs_serial;
  m->svs_prompt.resize((size_t)4 * batch);
  for (int b = 0; b < batch; ++b) {      // sensevoice-small.cpp:607-640: language, then the two fixed rows 1 and 2, then text normalisation
    m->svs_prompt[4 * b] = lid[b]; m->svs_prompt[4 * b + 1] = 1; m->svs_prompt[4 * b + 2] = 2; m->svs_prompt[4 * b + 3] = textnorm[b];
  }
  std::vector<int64_t> off;
  pfhip_status st = stage_pcm(m, pcm, n_samples, batch, s, off);
  if (st) return st;
  if (out->logp) {       // the row count is known on the host before anything is launched
    size_t rows = 0;
    for (int b = 0; b < batch; ++b) {
      const int F = n_samples[b] < 400 ? 0 : 1 + (n_samples[b] - 400) / 160;
      const int T = (F + m->weights->cfg.lfr_n - 1) / m->weights->cfg.lfr_n;
      rows += T > 0 ? (size_t)T + 4 : 0;
    }
    if (rows * (size_t)V > out->logp_cap_floats) return fail(PFHIP_ERR_CAPACITY, "logp_cap_floats smaller than rows x vocabulary");
  }
  m->svs_logp_host = out->logp;
  st = enqueue_locked(m, PcmView{m->pcm.p, pcm.s16}, off.data(), n_samples, batch, s, false);
  if (!st && m->M > 0 && m->range_hit && !m->weights->always_exact) {      // the guard of the fp16 two-plane domain: redone once, exact
    ++m->range_fallbacks;
    m->exact_rerun = true;
    st = enqueue_locked(m, PcmView{m->pcm.p, pcm.s16}, off.data(), n_samples, batch, s, false);
    m->exact_rerun = false;
  }
  m->svs_logp_host = nullptr;
  if (st) return st;
  m->svs_fwd_ok = true;                          // the rows and their log-sum-exp are what pfhip_svs_align reads ...
  {                                              // ... for this thread, until this context runs another forward
    if (tl_svs_notes.size() > 64) tl_svs_notes.clear();
    tl_svs_notes[(m->group_head ? m->group_head : m)->uid] = SvsNote{m->uid, ++m->svs_serial};
  }
  for (int b = 0; b < batch; ++b) {
    if (out->token_num) out->token_num[b] = m->M ? m->token_num[b] : 0;
    if (out->frame_len) out->frame_len[b] = m->T[b];
  }
  if (m->M == 0) return PFHIP_OK;
  if ((out->ids || out->tok_frame || out->tok_logp) && out->max_tokens < m->maxL)
    return fail(PFHIP_ERR_CAPACITY, "max_tokens smaller than the longest token sequence");
  const SvsHost h = svs_host(m);
  for (int b = 0; b < batch; ++b) {
    const size_t n = (size_t)m->token_num[b], src = (size_t)b * m->maxT, dst = (size_t)b * out->max_tokens;
    if (out->ids) std::memcpy(out->ids + dst, h.ids + src, n * 4);
    if (out->tok_frame) std::memcpy(out->tok_frame + dst, h.frames + src, n * 4);
    if (out->tok_logp) std::memcpy(out->tok_logp + dst, h.logp + src, n * 4);
  }
  if (out->frame_ids) std::memcpy(out->frame_ids, h.fid, (size_t)m->M * 4);
  if (out->frame_logp) std::memcpy(out->frame_logp, h.flp, (size_t)m->M * 4);
  return PFHIP_OK;
}

}  // namespace pfhip_impl

extern "C" {

// ---- SenseVoiceSmall, offline ------------------------------------------------------------------------------------------------
int pfhip_is_ctc(const pfhip_model* m) { return is_svs(m) ? 1 : 0; }
// lid_map (sensevoice-small.h:121-129), looked up as sensevoice-small.cpp:597-602 does: an unknown string keeps 0
int pfhip_svs_lid(const char* svs_lang) {
  static const struct { const char* name; int id; } kLid[] = {{"auto", 0}, {"zh", 3}, {"en", 4}, {"yue", 7}, {"ja", 11}, {"ko", 12}, {"nospeech", 13}};
  if (svs_lang)
    for (const auto& e : kLid)
      if (std::strcmp(svs_lang, e.name) == 0) return e.id;
  return 0;
}

pfhip_status pfhip_svs_forward(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                               const int32_t* textnorm, pfhip_svs_out* out) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out);
}
pfhip_status pfhip_svs_forward_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                   const int32_t* textnorm, pfhip_svs_out* out) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out);
}

// CTC forced alignment of caller-given tokens against the rows of the calling thread's last pfhip_svs_forward (ctc_align.hip): the
// emissions of blank | tokens[b] from the kept encoder rows and their log-sum-exp, the Viterbi pass, one copy back, one sync.
pfhip_status pfhip_svs_align(pfhip_model* head, const int32_t* const* tokens, const int* n_tokens, int batch, pfhip_svs_align_out* out) {
  g_err.clear();
  if (!head || !tokens || !n_tokens || batch <= 0 || !out || !out->tok_begin || !out->tok_end) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(head)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: there are no CTC rows to align against");
  // the context this thread's last forward ran on, looked up among this handle's own (matched on the uid: never a stale address)
  pfhip_model* m = nullptr;
  const auto note = tl_svs_notes.find(head->uid);
  if (note != tl_svs_notes.end()) {
    if (head->uid == note->second.ctx_uid) m = head;
    for (pfhip_model* cx : head->contexts)
      if (cx->uid == note->second.ctx_uid) m = cx;
  }
  if (!m) return fail(PFHIP_ERR_ARG, "this thread has run no pfhip_svs_forward on this handle");
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->svs_fwd_ok || m->svs_serial != note->second.serial)
    return fail(PFHIP_ERR_ARG, "the rows of this thread's last pfhip_svs_forward are gone: its execution context has run another forward since");
  if (batch != m->B) return fail(PFHIP_ERR_ARG, "batch differs from that of the last pfhip_svs_forward");
  const ModelWeights& w = *m->weights;
  const Config& c = w.cfg;
  const int V = c.vocab, d = c.d_model, B = batch;
  int longest = 0;
  size_t n_labels = 0;
  for (int b = 0; b < B; ++b) {
    if (n_tokens[b] < 0 || (n_tokens[b] > 0 && !tokens[b])) return fail(PFHIP_ERR_ARG, "bad token list");
    for (int j = 0; j < n_tokens[b]; ++j)
      if (tokens[b][j] < 0 || tokens[b][j] >= V || tokens[b][j] == c.blank_id)
        return fail(PFHIP_ERR_ARG, "a token outside 0 .. vocab - 1, or the blank");
    longest = std::max(longest, n_tokens[b]);
    n_labels += (size_t)n_tokens[b];
  }
  if (out->max_tokens < longest) return fail(PFHIP_ERR_CAPACITY, "max_tokens smaller than the longest token list");
  if (longest > pfhip::ctc_align_max_tokens()) return fail(PFHIP_ERR_UNSUPPORTED, "more tokens than the trellis kernel's LDS rows hold");
  const int maxL = std::max(longest, 1);
  // host metadata: row_off, len, lab_off, n_lab [B] | labels | e_off [B] (int64, 8-byte aligned)
  const size_t n_i32 = (4 * (size_t)B + std::max<size_t>(n_labels, 1) + 1) & ~(size_t)1;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(m->al_host.ensure(n_i32 * 4 + (size_t)B * 8));
  HIP_TRY(m->al_meta.ensure(n_i32 * 4 + (size_t)B * 8));
  int* hm = m->al_host.i();
  long long* h_eoff = reinterpret_cast<long long*>(hm + n_i32);
  size_t e_floats = 0, lo = 0;
  for (int b = 0; b < B; ++b) {
    const int N = m->T[b] > 4 ? m->T[b] - 4 : 0;                     // the speech rows: the four prompt rows are no CTC rows
    hm[b] = m->row_off[b] + 4; hm[B + b] = N; hm[2 * B + b] = (int)lo; hm[3 * B + b] = n_tokens[b];
    for (int j = 0; j < n_tokens[b]; ++j) hm[4 * B + lo + j] = tokens[b][j];
    lo += (size_t)n_tokens[b];
    h_eoff[b] = (long long)e_floats;
    e_floats += (size_t)N * (n_tokens[b] + 1);
  }
  hipStream_t s = m->own_stream;
  int* dm = m->al_meta.i();
  const long long* d_eoff = reinterpret_cast<const long long*>(dm + n_i32);
  const size_t bt = (size_t)B * maxL, n_out = 3 * bt + B;
  const size_t ws = pfhip::ctc_align_workspace_bytes(e_floats);
  HIP_TRY(m->al_E.ensure(std::max<size_t>(e_floats, 1) * 4));
  HIP_TRY(m->al_ws.ensure(std::max<size_t>(ws, 1)));
  HIP_TRY(m->al_out.ensure(n_out * 4));
  std::vector<int32_t> res(n_out);
  HIP_TRY(hipMemcpyAsync(dm, hm, n_i32 * 4 + (size_t)B * 8, hipMemcpyHostToDevice, s));
  int32_t *d_begin = m->al_out.i(), *d_end = d_begin + bt;
  float *d_logp = reinterpret_cast<float*>(d_end + bt), *d_score = d_logp + bt;
  // (no profiling Scope: pfhip_profile_read stays the forward's own time)
  if (m->M > 0) {
    if (!pfhip::launch_ctc_emissions(m->x.f(), d, w.ctc.w, d, w.ctc.b, m->svs_lse.f(), dm, dm + B, dm + 2 * B, dm + 3 * B, dm + 4 * B, d_eoff, B,
                                     d, V, c.blank_id, m->al_E.f(), s))
      return fail(PFHIP_ERR_UNSUPPORTED, "CTC emissions: d_model must be a multiple of 32");
  }
  {
    if (!pfhip::launch_ctc_align(m->al_E.f(), d_eoff, e_floats, dm + B, dm + 3 * B, dm + 4 * B, dm + 2 * B, B, maxL, d_begin, d_end, d_logp,
                                 d_score, m->al_ws.p, ws, s))
      return fail(PFHIP_ERR_ARG, "CTC alignment refused its arguments");
  }
  HIP_TRY(hipMemcpyAsync(res.data(), m->al_out.p, n_out * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  const float* r_logp = reinterpret_cast<const float*>(res.data() + 2 * bt);
  for (int b = 0; b < B; ++b) {
    const size_t dst = (size_t)b * out->max_tokens, src = (size_t)b * maxL;
    for (int j = 0; j < n_tokens[b]; ++j) {        // tok_frame's numbering: the prompt rows counted
      const int32_t tb = res[src + j], te = res[bt + src + j];
      out->tok_begin[dst + j] = tb < 0 ? -1 : tb + 4;
      out->tok_end[dst + j] = te < 0 ? -1 : te + 4;
      if (out->tok_logp) out->tok_logp[dst + j] = r_logp[src + j];
    }
    if (out->score) out->score[b] = r_logp[bt + b];
  }
  return PFHIP_OK;
}

}  // extern "C"
