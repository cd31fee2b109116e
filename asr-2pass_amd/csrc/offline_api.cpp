// The offline Paraformer entry points and the cross-request batching queue behind them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "offline.h"
#include "ctx_graph.h"

#define g_err (pfhip_impl::last_error())

// (BatchReq, the global type internal.h declares for pfhip_model::bq, is in offline.h: the SenseVoice forwards queue there too)

// ---- cross-request batching ---------------------------------------------------------------------------------
// The reference server runs `decoder-thread-num` threads that each call Forward on the shared handle with their own
// request (websocket/bin/funasr-wss-server.cpp:479-481); its dynamic batcher only groups segments of ONE request
// (audio.cpp:1056-1084).  On one MI355X a single 60-s segment fills 1/16 of the GEMM grid, so concurrent callers are
// merged here: callers queue at the handle, the one at the front leads — claims an idle execution slot, gathers company
// (PoolQueue: no wait at all when nothing else is in flight), runs ONE packed forward for the utterances it took and hands
// every caller its own slice — while the next caller in line already gathers the next batch for the next idle slot.
// Results are those of separate calls up to the near-tie statement the tests make (packed layout, per-utterance masks:
// tests/test_gpu_forward.py::test_batch_composition_invariance — a merged forward may run another kernel family than a lone one,
// the same sums in another order, 1e-6 apart in the log-probabilities).
namespace {
using namespace pfhip_impl;

// The fire frames of the calling thread's last pfhip_offline_fetch / pfhip_offline_forward_resident, for pfhip_offline_fetch_fire_frames:
// copied out of the execution slot while its lock is still held, into storage the thread owns, already laid out by that call's batch and
// max_tokens (per utterance its count and its frames).  On a shared handle another thread may take the slot the moment the lock is
// gone; what this thread reads later is its own call's, and no slot state.  Matched on the handle's uid, not its address.
struct ThreadFires {
  uint64_t head_uid = 0;
  bool recorded = false;            // the forward ran with fire frames on
  bool laid_out = false;            // ... and the call's max_tokens had room for its longest token sequence
  int max_tokens = 0;
  std::vector<int32_t> n, frames;   // [B], [B * max_tokens]
};
thread_local ThreadFires tl_fires;
// under m->mu, after a successful fetch_locked(m, out, ...)
void keep_thread_fires(const pfhip_model* head, const pfhip_model* m, const pfhip_out* out) {
  ThreadFires& t = tl_fires;
  t.head_uid = head->uid;
  t.recorded = m->want_fires;
  t.max_tokens = out->max_tokens;
  t.n.clear(); t.frames.clear();
  t.laid_out = m->ML == 0 || out->max_tokens >= m->maxL;
  if (!t.recorded || m->ML == 0 || !t.laid_out) return;
  t.n.assign(m->n_fires.begin(), m->n_fires.begin() + m->B);
  t.frames.assign((size_t)m->B * out->max_tokens, 0);
  scatter_fires(m, t.frames.data(), out->max_tokens);
}

pfhip_status offline_enqueue(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
                                    int batch, void* stream) {
  g_err.clear();
  if (is_svs(m)) return refuse_svs();
  if (!m || !sample_off || !n_samples || batch <= 0) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!d_pcm.p) return fail(PFHIP_ERR_ARG, "null device pcm");
  std::lock_guard<std::mutex> lk(m->mu);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m->own_stream;
  m->prof_stream = s;
  HIP_TRY(hipSetDevice(m->device));
  // the default hotword set: its bank entry stays pinned for as long as it is the default, so this forward's own pins can go at once
  HotwordPins pins{m};
  pfhip_status st = resolve_default_hotwords_locked(m, batch, s);
  if (st) return st;
  m->nbest_k = m->nbest_enqueue_k;         // pfhip_set_nbest
  m->want_fires = m->fires_enqueue.load() != 0;      // pfhip_set_fire_frames
  st = enqueue_locked(m, d_pcm, sample_off, n_samples, batch, s, false);
  if (st) return st;
  return head_locked(m, s, false);
}

// one packed forward on `m` for everybody in `take` (all of one sample format: forward_batched's pick splits the queue by format)
void run_batch_requests(pfhip_model* m, const std::vector<BatchReq*>& all_taken) {
  std::vector<const void*> ptrs; std::vector<int> lens;
  bool want_logp = false, want_us = false; int max_tok = 1, utts = 0;
  int kmax = 0;      // the packed forward computes the largest k among its callers; the order makes every prefix a caller's own answer
  bool want_fires = false;      // ... and records fire frames when any of them asks; each receives its own utterances' rows
  // Contextual model: the callers' hotword sets, deduplicated (one connection sends the same list with each of its segments; the
  // bank then matches by content), and for every packed utterance the index of its set.  A caller without hotwords fails alone
  // with the reference's "hw_emb is null" (paraformer.cpp:516-520); its company is served.
  std::vector<BatchReq*> take;
  std::vector<const float*> set_emb; std::vector<int> set_n, set_of;
  for (BatchReq* r : all_taken) {
    if (m->weights->cfg.contextual) {
      bool ok = r->hw.n_sets > 0 && r->hw.emb && r->hw.n;
      for (int i = 0; ok && i < r->batch; ++i) {
        const int k = r->hw.of_utt ? r->hw.of_utt[i] : 0;
        ok = k >= 0 && k < r->hw.n_sets && r->hw.emb[k] && r->hw.n[k] > 0;
      }
      if (!ok) { r->st = PFHIP_ERR_ARG; r->err = "hw_emb is null"; continue; }
      for (int i = 0; i < r->batch; ++i) {
        const int k = r->hw.of_utt ? r->hw.of_utt[i] : 0;
        size_t j = 0;
        while (j < set_emb.size() && !(set_emb[j] == r->hw.emb[k] && set_n[j] == r->hw.n[k])) ++j;
        if (j == set_emb.size()) { set_emb.push_back(r->hw.emb[k]); set_n.push_back(r->hw.n[k]); }
        set_of.push_back((int)j);
      }
    }
    take.push_back(r);
  }
  if (take.empty()) return;
  for (BatchReq* r : take) {
    for (int i = 0; i < r->batch; ++i) { ptrs.push_back(r->pcm.p[i]); lens.push_back(r->n[i]); max_tok = std::max(max_tok, r->n[i] / 960 + 2); }
    want_logp = want_logp || r->out->logp != nullptr;
    if (r->dt) { kmax = std::max(kmax, (int)r->dt->nbest_k); want_fires = want_fires || r->dt->fire_frame; }
    want_us = want_us || r->out->us_alphas || r->out->us_peaks || r->out->us_len;
    utts += r->batch;
  }
  const int V = m->weights->cfg.vocab, max_us = 3 * max_tok;
  std::vector<int32_t> ids((size_t)utts * max_tok), tn(utts), nf(utts), fr(utts), usl;
  std::vector<float> logp, usa, usp;
  if (want_logp) logp.resize((size_t)utts * max_tok * V);
  pfhip_out all{};
  all.token_ids = ids.data(); all.token_num = tn.data(); all.n_fires = nf.data(); all.n_frames = fr.data();
  all.logp = want_logp ? logp.data() : nullptr; all.max_tokens = max_tok;
  if (want_us) {
    usa.resize((size_t)utts * max_us); usp.resize((size_t)utts * max_us); usl.resize(utts);
    all.us_alphas = usa.data(); all.us_peaks = usp.data(); all.us_len = usl.data(); all.max_us = max_us;
  }
  std::vector<int32_t> nbi; std::vector<float> nbl;
  if (kmax) { nbi.resize((size_t)utts * max_tok * kmax); nbl.resize(nbi.size()); }
  std::vector<int32_t> fire_all(want_fires ? (size_t)utts * max_tok : 0);
  const pfhip_detail dt_all{kmax, kmax ? nbi.data() : nullptr, kmax ? nbl.data() : nullptr, want_fires ? fire_all.data() : nullptr};
  const HwSets sets{set_emb.data(), set_n.data(), (int)set_emb.size(), set_of.data()};
  pfhip_status st = forward_direct(m, HostPcm(ptrs.data(), take.front()->pcm.s16), lens.data(), utts, sets, &all, 0,
                                   kmax || want_fires ? &dt_all : nullptr);
  const std::string err = g_err;
  int u0 = 0;
  for (BatchReq* r : take) {
    r->st = st; r->err = err;
    for (int i = 0; i < r->batch && st == PFHIP_OK; ++i) {
      const int u = u0 + i;
      pfhip_out* o = r->out;
      if (o->token_num) o->token_num[i] = tn[u];
      if (o->n_fires) o->n_fires[i] = nf[u];
      if (o->n_frames) o->n_frames[i] = fr[u];
      const int rk = r->dt ? r->dt->nbest_k : 0;
      int32_t* rfire = r->dt ? r->dt->fire_frame : nullptr;
      if ((o->token_ids || o->logp || rk || rfire) && o->max_tokens < nf[u]) {
        r->st = PFHIP_ERR_CAPACITY; r->err = "max_tokens smaller than the longest token sequence"; break;
      }
      if (o->token_ids) std::memcpy(o->token_ids + (size_t)i * o->max_tokens, ids.data() + (size_t)u * max_tok, 4 * (size_t)nf[u]);
      if (o->logp) std::memcpy(o->logp + (size_t)i * o->max_tokens * V, logp.data() + (size_t)u * max_tok * V, 4 * (size_t)nf[u] * V);
      if (rk)
        for (int t = 0; t < nf[u]; ++t) {
          const size_t src = ((size_t)u * max_tok + t) * kmax, dst = ((size_t)i * o->max_tokens + t) * rk;
          std::memcpy(r->dt->nbest_ids + dst, nbi.data() + src, 4 * (size_t)rk);
          std::memcpy(r->dt->nbest_logp + dst, nbl.data() + src, 4 * (size_t)rk);
        }
      if (rfire && nf[u]) std::memcpy(rfire + (size_t)i * o->max_tokens, fire_all.data() + (size_t)u * max_tok, 4 * (size_t)nf[u]);
      if (o->us_alphas || o->us_peaks || o->us_len) {
        if (o->us_len) o->us_len[i] = usl[u];
        if ((o->us_alphas || o->us_peaks) && o->max_us < usl[u]) { r->st = PFHIP_ERR_CAPACITY; r->err = "max_us smaller than 3 x frames"; break; }
        if (o->us_alphas) std::memcpy(o->us_alphas + (size_t)i * o->max_us, usa.data() + (size_t)u * max_us, 4 * (size_t)usl[u]);
        if (o->us_peaks) std::memcpy(o->us_peaks + (size_t)i * o->max_us, usp.data() + (size_t)u * max_us, 4 * (size_t)usl[u]);
      }
    }
    u0 += r->batch;
  }
}

thread_local pfhip_model* tl_last_replica = nullptr;      // where this thread's last offline forward ran (debug getters)

pfhip_status forward_batched(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                    const HwSets& hw, pfhip_out* out, const pfhip_detail* dt) {
  BatchReq me;
  me.pcm = pcm; me.n = n_samples; me.batch = batch; me.out = out; me.hw = hw; me.dt = dt;
  pfhip_model* ran_on = pool_submit(head, me, run_batch_requests);
  if (ran_on) tl_last_replica = ran_on;       // the leader's own slice ran there; followers ask the handle (pfhip_get_tensor: head)
  if (me.st != PFHIP_OK) g_err = me.err;
  return me.st;
}

// dt: candidates and / or fire frames beside `out` (nbest_k = 0: no candidates), or null.  rate: the rate of `pcm`, none or the model's
// own for audio at the model's rate; another rate is resampled on the device into the slot's PCM workspace and runs alone (one rate
// pair per packed batch)
pfhip_status offline_forward_sets(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const HwSets& hw,
                                         pfhip_out* out, const pfhip_detail* dt = nullptr, std::optional<int> rate = std::nullopt) {
  g_err.clear();
  if (is_svs(head)) return refuse_svs();
  if (!head || !pcm.p || !n_samples || batch <= 0 || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (dt && dt->nbest_k && (dt->nbest_k < 1 || dt->nbest_k > pfhip::kTopkMax || dt->nbest_k > head->weights->cfg.vocab || !dt->nbest_ids ||
                            !dt->nbest_logp))
    return fail(PFHIP_ERR_ARG, "nbest: k outside 1..8 (or above the vocabulary) or a null buffer");
  for (int i = 0; i < batch; ++i)
    if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm.p[i])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
  const bool other_rate = rate && *rate != head->weights->cfg.sample_rate;
  if (other_rate) {
    std::string why;
    if (!pfhip_impl::resample_supported(*rate, head->weights->cfg.sample_rate, &why)) return fail(PFHIP_ERR_UNSUPPORTED, why);
  }
  const int fs_in = other_rate ? *rate : 0;      // forward_direct: 0 = no resampling
  // merged with whoever else is calling: plain and timestamp models always; contextual models — every caller with its own hotword
  // sets, each utterance attending to its own set in the packed forward — where pfhip_set_hotword_merging is on
  bool merge;
  {
    std::lock_guard<std::mutex> l(head->bq.mu);
    merge = !fs_in && head->batch_wait_us > 0 && batch < head->batch_max_utts && (!head->weights->cfg.contextual || head->hw_merge);
  }
  if (merge) return forward_batched(head, pcm, n_samples, batch, hw, out, dt);
  pfhip_model* m = acquire_slot(head);                  // the least-loaded execution slot (context / GPU)
  tl_last_replica = m;
  const pfhip_status st = forward_direct(m, pcm, n_samples, batch, hw, out, fs_in, dt);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}

// the hotword-set arguments of the hwsets / nbest / detail forms as the HwSets of the call; a contextual model's sets come whole
pfhip_status hw_sets_of(const pfhip_model* head, const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                        HwSets* hw) {
  if (head && head->weights->cfg.contextual && n_sets > 0 && (!hw_emb || !n_hotwords || !set_of_utt)) {
    g_err.clear();
    return fail(PFHIP_ERR_ARG, "bad argument");
  }
  *hw = HwSets{hw_emb, n_hotwords, n_sets < 0 ? 0 : n_sets, set_of_utt};
  return PFHIP_OK;
}

pfhip_status offline_forward_hwsets(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                           const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                           pfhip_out* out) {
  HwSets hw;
  if (const pfhip_status hs = hw_sets_of(head, hw_emb, n_hotwords, n_sets, set_of_utt, &hw)) return hs;
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out);
}

// pfhip_offline_forward_hwsets plus the k best candidates of every token row (an extension: GreedySearch, paraformer.cpp:386-395,
// keeps only the arg-max); nb == nullptr is pfhip_offline_forward_hwsets itself
pfhip_status offline_forward_nbest(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out, const pfhip_nbest* nb) {
  HwSets hw;
  if (const pfhip_status hs = hw_sets_of(head, hw_emb, n_hotwords, n_sets, set_of_utt, &hw)) return hs;
  if (!nb) return offline_forward_sets(head, pcm, n_samples, batch, hw, out);
  if (nb->k < 1) { g_err.clear(); return fail(PFHIP_ERR_ARG, "nbest: k outside 1..8 (or above the vocabulary) or a null buffer"); }
  const pfhip_detail dt{nb->k, nb->ids, nb->logp, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, &dt);
}

// the hwsets form with a pfhip_detail (candidates and / or fire frames) and the rate of the audio
pfhip_status offline_forward_detail(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, int sample_rate,
                                           const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                           pfhip_out* out, const pfhip_detail* dt) {
  HwSets hw;
  if (const pfhip_status hs = hw_sets_of(head, hw_emb, n_hotwords, n_sets, set_of_utt, &hw)) return hs;
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, dt, sample_rate == 0 ? std::nullopt : std::optional<int>(sample_rate));      // 0 = the model's
}

// pfhip_offline_forward with the PCM already in HBM: same routing over the execution slots, no H2D of the audio
pfhip_status offline_forward_resident(pfhip_model* head, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
                                             int batch, pfhip_out* out) {
  g_err.clear();
  if (is_svs(head)) return refuse_svs();
  if (!head || !d_pcm.p || !sample_off || !n_samples || batch <= 0 || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (head->weights->cfg.contextual && !default_hotwords(head)) return fail(PFHIP_ERR_ARG, "hw_emb is null");
  pfhip_model* m = acquire_slot(head);
  tl_last_replica = m;
  pfhip_status st;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    hipStream_t s = m->own_stream;
    m->prof_stream = s;
    HotwordPins pins{m};
    st = hipSetDevice(m->device) == hipSuccess ? PFHIP_OK : fail(PFHIP_ERR_HIP, "hipSetDevice");
    m->nbest_k = 0;
    m->want_fires = head->fires_enqueue.load() != 0;      // pfhip_set_fire_frames, on the handle the caller holds
    if (!st) st = resolve_default_hotwords_locked(m, batch, s);
    if (!st) st = enqueue_locked(m, d_pcm, sample_off, n_samples, batch, s, false);
    if (!st) st = head_locked(m, s, out->logp != nullptr);
    if (!st) st = fetch_locked(m, out, s);
    if (!st) keep_thread_fires(head, m, out);      // while the slot is still this call's: for pfhip_offline_fetch_fire_frames
  }
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}

// pfhip_offline_forward_detail plus the hotword-biased search over the head's candidates (nar_beam.hip).  Served alone, past the
// merge queue, on the least-loaded execution slot; every refusal comes before anything is staged.
pfhip_status offline_forward_bias(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, int sample_rate,
                                  const float* const* hw_emb, const int* n_hotwords, int n_hw_sets, const int* hw_set_of, pfhip_out* out,
                                  const pfhip_detail* dt, const pfhip_bias_opts* sets, int n_sets, const int32_t* set_of, pfhip_bias_out* bo) {
  g_err.clear();
  if (is_svs(head)) return refuse_svs();
  if (!head || !pcm.p || !n_samples || batch <= 0 || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!head->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "bias: not on a multi-device group");
  if (!sets || n_sets < 1 || !bo || !bo->n_hyp || !bo->n_tokens || bo->max_tokens < 0 || (bo->max_tokens > 0 && !bo->ids))
    return fail(PFHIP_ERR_ARG, "bias: sets and the n_hyp / ids / n_tokens buffers are needed");
  if (dt && dt->nbest_k && (dt->nbest_k < 1 || dt->nbest_k > pfhip::kTopkMax || dt->nbest_k > head->weights->cfg.vocab || !dt->nbest_ids ||
                            !dt->nbest_logp))
    return fail(PFHIP_ERR_ARG, "nbest: k outside 1..8 (or above the vocabulary) or a null buffer");
  const int V = head->weights->cfg.vocab;
  std::vector<pfhip::BeamUtt> utt((size_t)batch, pfhip::BeamUtt{0, 0, 0, -1});
  std::vector<const pfhip_ctx_graph*> graphs;
  int kmax = 0;
  for (int b = 0; b < batch; ++b) {
    const int k = set_of ? set_of[b] : 0;
    if (k < -1 || k >= n_sets) return fail(PFHIP_ERR_ARG, "bias: set_of outside -1 .. n_sets - 1");
    if (k < 0) continue;
    const pfhip_bias_opts& o = sets[k];
    if (o.width < 1 || o.width > pfhip::kNarWidthMax || o.width > V || o.beam < 1 || o.beam > pfhip::kBeamMax || o.nbest < 1 || o.nbest > o.beam)
      return fail(PFHIP_ERR_ARG, "bias: width outside 1..8 (or above the vocabulary), beam outside 1..16 or nbest outside 1..beam");
    if (o.graph && o.graph->vocab != V) return fail(PFHIP_ERR_ARG, "bias: the graph was built for another vocabulary");
    int gi = -1;
    if (o.graph) {
      gi = (int)(std::find(graphs.begin(), graphs.end(), o.graph) - graphs.begin());
      if (gi == (int)graphs.size()) graphs.push_back(o.graph);
    }
    utt[b] = pfhip::BeamUtt{o.width, o.beam, o.nbest, gi};
    kmax = std::max(kmax, o.width);
  }
  const int stride_k = std::max(kmax, dt ? (int)dt->nbest_k : 0);
  NarBias nb{utt.data(), graphs.data(), (int)graphs.size(), stride_k, 1, 1, bo};
  if (kmax && !pfhip::nbest_ctx_beam_check(utt.data(), batch, stride_k, nb.n_graphs, true, &nb.beam_stride, &nb.nbest_stride))
    return fail(PFHIP_ERR_ARG, "bias: the search refused its descriptors");
  HwSets hw;
  if (const pfhip_status hs = hw_sets_of(head, hw_emb, n_hotwords, n_hw_sets, hw_set_of, &hw)) return hs;
  for (int i = 0; i < batch; ++i)
    if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm.p[i])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
  const bool other_rate = sample_rate != 0 && sample_rate != head->weights->cfg.sample_rate;
  if (other_rate) {
    std::string why;
    if (!pfhip_impl::resample_supported(sample_rate, head->weights->cfg.sample_rate, &why)) return fail(PFHIP_ERR_UNSUPPORTED, why);
  }
  // "no hypothesis" everywhere first: what an utterance without a search, without rows, or a batch without any token row keeps
  for (int b = 0; b < batch; ++b) {
    bo->n_hyp[b] = 0;
    for (int j = 0; j < nb.nbest_stride; ++j) {
      const size_t o = (size_t)b * nb.nbest_stride + j;
      bo->n_tokens[o] = 0;
      if (bo->score) bo->score[o] = -INFINITY;
      if (bo->am_score) bo->am_score[o] = -INFINITY;
      if (bo->ctx_score) bo->ctx_score[o] = 0.f;
    }
  }
  pfhip_model* m = acquire_slot(head);
  tl_last_replica = m;
  const pfhip_status st = forward_direct(m, pcm, n_samples, batch, hw, out, other_rate ? sample_rate : 0, dt, kmax ? &nb : nullptr);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}

// pfhip_offline_forward at the caller's rate: resampled on the device into the slot's PCM workspace, then the same forward
pfhip_status offline_forward_rate(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, int sample_rate,
                                         const float* hw_emb, int n_hotwords, pfhip_out* out) {
  const HwSets hw{&hw_emb, &n_hotwords, hw_emb && n_hotwords > 0 ? 1 : 0, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, nullptr, sample_rate);
}

}  // namespace

namespace pfhip_impl {

// every Paraformer entry point on a SenseVoice handle
bool is_svs(const pfhip_model* m) { return m && m->weights->cfg.svs; }
pfhip_status refuse_svs() { return fail(PFHIP_ERR_UNSUPPORTED, "a SenseVoice (CTC) model is run through pfhip_svs_forward"); }

// The batch packed into the slot's PCM workspace in the caller's own format: `off` counts samples, the workspace is indexed in floats
// or in shorts accordingly (one buffer; 16-bit PCM takes half of what the same batch takes as floats).
pfhip_status stage_pcm(pfhip_model* m, HostPcm pcm, const int* n_samples, int B, hipStream_t s,
                       std::vector<int64_t>& off) {
  off.assign(B, 0);
  int64_t tot = 0;
  for (int b = 0; b < B; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm.p[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    off[b] = tot;
    tot += (n_samples[b] + 3) & ~3;
  }
  const size_t es = pcm.sample_bytes();
  HIP_TRY(m->pcm.ensure((size_t)std::max<int64_t>(tot, 4) * es));
  for (int b = 0; b < B; ++b)
    if (n_samples[b])
      HIP_TRY(hipMemcpyAsync(static_cast<char*>(m->pcm.p) + (size_t)off[b] * es, pcm.p[b], (size_t)n_samples[b] * es, hipMemcpyHostToDevice, s));
  return PFHIP_OK;
}

// The batch at the caller's rate fs_in: staged into rs_in, resampled on `s` into `pcm` at the model's rate, packed as stage_pcm
// packs it.  off / n_out receive the model-rate layout.  16-bit PCM is staged as it is and converted by the kernel's loads; what
// lands in `pcm` is f32 either way.
pfhip_status stage_resampled(pfhip_model* m, HostPcm pcm, const int* n_samples, int B, int fs_in, hipStream_t s,
                             std::vector<int64_t>& off, std::vector<int>& n_out) {
  pfhip::ResampleTable t;
  pfhip_status st = (m->weights_of ? m->weights_of : m)->rs_cache->get(m->device, fs_in, m->weights->cfg.sample_rate, &t);
  if (st) return st;
  std::vector<int64_t> in_off(B);
  off.assign(B, 0);
  n_out.assign(B, 0);
  int64_t tin = 0, tout = 0;
  for (int b = 0; b < B; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm.p[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    const int64_t no = pfhip_impl::resample_out_len(fs_in, m->weights->cfg.sample_rate, n_samples[b]);
    if (no < 0 || no > INT32_MAX) return fail(PFHIP_ERR_ARG, "resampled utterance too long");
    in_off[b] = tin;
    tin += (n_samples[b] + 3) & ~3;
    n_out[b] = (int)no;
    off[b] = tout;
    tout += (no + 3) & ~3;
  }
  const size_t es = pcm.sample_bytes();
  HIP_TRY(m->rs_in.ensure((size_t)std::max<int64_t>(tin, 4) * es));
  HIP_TRY(m->pcm.ensure((size_t)std::max<int64_t>(tout, 4) * 4));
  for (int b = 0; b < B; ++b)
    if (n_samples[b])
      HIP_TRY(hipMemcpyAsync(static_cast<char*>(m->rs_in.p) + (size_t)in_off[b] * es, pcm.p[b], (size_t)n_samples[b] * es, hipMemcpyHostToDevice, s));
  {
    Scope sc(m, s, K_FBANK, 0.0, (double)es * (double)tin + 4.0 * (double)tout);
    if (pcm.s16)
      pfhip::launch_resample(static_cast<const int16_t*>(m->rs_in.p), in_off.data(), n_samples, m->pcm.f(), off.data(), n_out.data(), B, t, s);
    else
      pfhip::launch_resample(m->rs_in.f(), in_off.data(), n_samples, m->pcm.f(), off.data(), n_out.data(), B, t, s);
  }
  HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}

// fs_in: the rate of `pcm` when it is not the model's (resampled into the slot's PCM workspace first), else 0
pfhip_status forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch,
                                   const HwSets& hw, pfhip_out* out, int fs_in, const pfhip_detail* dt, const NarBias* bias) {
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->own_stream;
  m->prof_stream = s;
  if (dt && dt->nbest_k > m->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "nbest k larger than the vocabulary");      // before any launch
  m->nbest_k = dt ? dt->nbest_k : 0;
  // the search of pfhip_offline_forward_bias: the head computes the largest k anybody reads; the slot names the search for the
  // length of this call only (a range-guard re-run inside fetch_locked reads it again)
  struct BiasScope { pfhip_model* m; ~BiasScope() { m->bias = nullptr; m->fw_lm = nullptr; } } bias_scope{m};
  m->bias = bias;
  const std::shared_ptr<const TokenLm> lm = bias ? token_lm_of(m) : nullptr;      // pfhip_set_token_lm: the search walks it too
  m->fw_lm = lm.get();
  if (bias) m->nbest_k = std::max(m->nbest_k, bias->k);
  m->want_fires = dt && dt->fire_frame;
  HotwordPins pins{m};              // held until the results (a range-guard re-run included) are back
  {
    const pfhip_status hs = resolve_hotwords_locked(m, hw.emb, hw.n, hw.n_sets, hw.of_utt, batch, s);
    if (hs) return hs;
  }
  std::vector<int64_t> off;
  std::vector<int> n_rs;
  pfhip_status st = fs_in ? stage_resampled(m, pcm, n_samples, batch, fs_in, s, off, n_rs) : stage_pcm(m, pcm, n_samples, batch, s, off);
  if (st) return st;
  // the workspace holds the caller's format, except after resampling (always f32 out)
  st = enqueue_locked(m, PcmView{m->pcm.p, pcm.s16 && !fs_in}, off.data(), fs_in ? n_rs.data() : n_samples, batch, s, false);
  if (st) return st;
  st = head_locked(m, s, out->logp != nullptr);
  if (st) return st;
  return fetch_locked(m, out, s, dt);
}

// Callers of both sample formats share the queue; a packed forward holds ONE format, the leader's: pick takes the queued callers of
// that format (in order) and leaves the others, in order, for the next leader.  Nothing is converted on the host, every caller gets
// the results of a forward in its own format, which are those of the other format bit for bit.
// Returns the slot the caller LED a batch on (null for a follower); `run` fills every taken request's result fields.
pfhip_model* pool_submit(pfhip_model* head, BatchReq& me, void (*run)(pfhip_model*, const std::vector<BatchReq*>&)) {
  int wait_us, max_utts;
  { std::lock_guard<std::mutex> l(head->bq.mu); wait_us = head->batch_wait_us; max_utts = head->batch_max_utts; }
  pfhip_model* ran_on = nullptr;
  head->bq.submit(
      me, wait_us,
      // claim (under the queue lock): an idle slot, in the device-major order of `slots`
      [&]() -> pfhip_model* {
        if (head->slots.empty()) rebuild_slots_locked(head);
        for (pfhip_model* r : head->slots)
          if (r->inflight.load() == 0) { ++r->inflight; return r; }
        return nullptr;
      },
      [&](pfhip_model* r) { --r->inflight; },
      // gather: bounded by time and by utterance count
      [&](const std::deque<BatchReq*>& q) { int u = 0; for (BatchReq* r : q) u += r->batch; return u >= max_utts; },
      [&](std::deque<BatchReq*>& q, std::vector<BatchReq*>& take) {
        int utts = 0;
        const bool s16 = q.front()->pcm.s16;
        std::deque<BatchReq*> other;                      // callers of the other sample format: they stay queued, in order
        while (!q.empty() && (take.empty() || utts + q.front()->batch <= max_utts)) {
          if (q.front()->pcm.s16 == s16) {
            utts += q.front()->batch;
            take.push_back(q.front());
          } else {
            other.push_back(q.front());
          }
          q.pop_front();
        }
        for (auto it = other.rbegin(); it != other.rend(); ++it) q.push_front(*it);
        if (!other.empty()) ++head->format_splits;        // (pfhip_debug_poke "format_splits")
      },
      [&](pfhip_model* r, std::vector<BatchReq*>& take) {
        ran_on = r;
        int utts = 0;
        for (BatchReq* q : take) utts += q->batch;
        run(r, take);
        ++r->served_forwards; r->served_calls += (int64_t)take.size(); r->served_utts += utts;
      });
  return ran_on;
}

pfhip_model*& last_replica() { return tl_last_replica; }

}  // namespace pfhip_impl

extern "C" {

pfhip_status pfhip_offline_enqueue(pfhip_model* m, const float* d_pcm, const int64_t* sample_off, const int* n_samples,
                                   int batch, void* stream) {
  return offline_enqueue(m, PcmView{d_pcm, false}, sample_off, n_samples, batch, stream);
}
// the same from a device buffer of 16-bit PCM (what Audio::LoadPcmwav, audio.cpp:787-819, would have divided by 32768 on the host)
pfhip_status pfhip_offline_enqueue_s16(pfhip_model* m, const int16_t* d_pcm, const int64_t* sample_off, const int* n_samples,
                                       int batch, void* stream) {
  return offline_enqueue(m, PcmView{d_pcm, true}, sample_off, n_samples, batch, stream);
}

pfhip_status pfhip_offline_fetch(pfhip_model* m, pfhip_out* out) {
  g_err.clear();
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  const pfhip_status st = fetch_locked(m, out, m->prof_stream ? m->prof_stream : m->own_stream);
  if (!st) keep_thread_fires(m, m, out);      // for pfhip_offline_fetch_fire_frames
  return st;
}

pfhip_status pfhip_offline_forward(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch,
                                   const float* hw_emb, int n_hotwords, pfhip_out* out) {
  // one set for all: the one-set case of pfhip_offline_forward_hwsets
  const HwSets hw{&hw_emb, &n_hotwords, hw_emb && n_hotwords > 0 ? 1 : 0, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out);
}
// pfhip_offline_forward from 16-bit PCM: the bytes Audio::LoadPcmwav (audio.cpp:787-819) reads, without its host-side / 32768
pfhip_status pfhip_offline_forward_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch,
                                       const float* hw_emb, int n_hotwords, pfhip_out* out) {
  const HwSets hw{&hw_emb, &n_hotwords, hw_emb && n_hotwords > 0 ? 1 : 0, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out);
}

pfhip_status pfhip_offline_forward_hwsets(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out) {
  return offline_forward_hwsets(head, pcm, n_samples, batch, hw_emb, n_hotwords, n_sets, set_of_utt, out);
}
pfhip_status pfhip_offline_forward_hwsets_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch,
                                              const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                              pfhip_out* out) {
  return offline_forward_hwsets(head, pcm, n_samples, batch, hw_emb, n_hotwords, n_sets, set_of_utt, out);
}

pfhip_status pfhip_offline_forward_detail(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out, const pfhip_detail* dt) {
  return offline_forward_detail(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, n_sets, set_of_utt, out, dt);
}
pfhip_status pfhip_offline_forward_detail_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch,
                                              int sample_rate, const float* const* hw_emb, const int* n_hotwords, int n_sets,
                                              const int* set_of_utt, pfhip_out* out, const pfhip_detail* dt) {
  return offline_forward_detail(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, n_sets, set_of_utt, out, dt);
}
pfhip_status pfhip_offline_forward_nbest(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch,
                                         const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                         pfhip_out* out, const pfhip_nbest* nb) {
  return offline_forward_nbest(head, pcm, n_samples, batch, hw_emb, n_hotwords, n_sets, set_of_utt, out, nb);
}
pfhip_status pfhip_offline_forward_nbest_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch,
                                             const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                             pfhip_out* out, const pfhip_nbest* nb) {
  return offline_forward_nbest(head, pcm, n_samples, batch, hw_emb, n_hotwords, n_sets, set_of_utt, out, nb);
}

pfhip_status pfhip_offline_forward_bias(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                        const float* const* hw_emb, const int* n_hotwords, int n_hw_sets, const int* hw_set_of,
                                        pfhip_out* out, const pfhip_detail* det, const pfhip_bias_opts* sets, int n_sets,
                                        const int32_t* set_of, pfhip_bias_out* bias_out) {
  return offline_forward_bias(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, n_hw_sets, hw_set_of, out, det, sets, n_sets,
                              set_of, bias_out);
}
pfhip_status pfhip_offline_forward_bias_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch, int sample_rate,
                                            const float* const* hw_emb, const int* n_hotwords, int n_hw_sets, const int* hw_set_of,
                                            pfhip_out* out, const pfhip_detail* det, const pfhip_bias_opts* sets, int n_sets,
                                            const int32_t* set_of, pfhip_bias_out* bias_out) {
  return offline_forward_bias(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, n_hw_sets, hw_set_of, out, det, sets, n_sets,
                              set_of, bias_out);
}

// device-pointer form: k candidates for the following pfhip_offline_enqueue calls of this handle (context 0); 0 = off
pfhip_status pfhip_set_nbest(pfhip_model* m, int k) {
  g_err.clear();
  if (!m || k < 0 || k > pfhip::kTopkMax || k > m->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "nbest k outside 0..8 (or above the vocabulary)");
  std::lock_guard<std::mutex> lk(m->mu);
  m->nbest_enqueue_k = k;
  return PFHIP_OK;
}

// the candidates of the forward pfhip_offline_fetch just returned (a range-guard re-run included: its head filled the buffers again)
pfhip_status pfhip_offline_fetch_nbest(pfhip_model* m, const pfhip_nbest* nb) {
  g_err.clear();
  if (!m || !nb) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (nb->k < 1 || nb->k > m->nbest_k || !nb->ids || !nb->logp)
    return fail(PFHIP_ERR_ARG, "nbest: the last forward computed fewer candidates than asked for (pfhip_set_nbest), or a null buffer");
  if (m->ML == 0) return PFHIP_OK;
  if (m->nbest_fetch_max_tokens < m->maxL) return fail(PFHIP_ERR_CAPACITY, "pfhip_offline_fetch first: its max_tokens lays out the rows");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->prof_stream ? m->prof_stream : m->own_stream;
  NbestStage nbs;
  const pfhip_status st = nbs.start(m, s);
  if (st) return st;
  HIP_TRY(hipStreamSynchronize(s));
  nbs.scatter(m, nb->k, nb->ids, nb->logp, m->nbest_fetch_max_tokens);
  return PFHIP_OK;
}

// device-pointer forms: fire frames for the following pfhip_offline_enqueue / pfhip_offline_forward_resident calls of this handle
pfhip_status pfhip_set_fire_frames(pfhip_model* m, int on) {
  g_err.clear();
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  m->fires_enqueue.store(on != 0);
  return PFHIP_OK;
}

// the fire frames of the calling thread's last pfhip_offline_fetch / pfhip_offline_forward_resident on this handle (a range-guard re-run
// included: what was kept is what the call returned): from the thread's own copy, laid out by that call's max_tokens
pfhip_status pfhip_offline_fetch_fire_frames(pfhip_model* m, int32_t* fire_frame) {
  g_err.clear();
  if (!m || !fire_frame) return fail(PFHIP_ERR_ARG, "bad argument");
  const ThreadFires& t = tl_fires;
  if (t.head_uid != m->uid) return fail(PFHIP_ERR_ARG, "this thread has fetched no forward of this handle (pfhip_offline_fetch first)");
  if (!t.recorded) return fail(PFHIP_ERR_ARG, "the last forward recorded no fire frames (pfhip_set_fire_frames)");
  if (!t.laid_out) return fail(PFHIP_ERR_CAPACITY, "that call's max_tokens was smaller than its longest token sequence");
  for (size_t b = 0; b < t.n.size(); ++b)
    if (t.n[b]) std::memcpy(fire_frame + b * t.max_tokens, t.frames.data() + b * t.max_tokens, 4 * (size_t)t.n[b]);
  return PFHIP_OK;
}

int pfhip_lfr_frame_ms(const pfhip_model* m) { return m ? m->weights->cfg.lfr_n * 10 : 0; }      // 10-ms frame shift (paraformer.cpp:24-31)

pfhip_status pfhip_offline_forward_resident(pfhip_model* head, const float* d_pcm, const int64_t* sample_off, const int* n_samples,
                                            int batch, pfhip_out* out) {
  return offline_forward_resident(head, PcmView{d_pcm, false}, sample_off, n_samples, batch, out);
}
pfhip_status pfhip_offline_forward_resident_s16(pfhip_model* head, const int16_t* d_pcm, const int64_t* sample_off,
                                                const int* n_samples, int batch, pfhip_out* out) {
  return offline_forward_resident(head, PcmView{d_pcm, true}, sample_off, n_samples, batch, out);
}

pfhip_status pfhip_offline_forward_rate(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                        const float* hw_emb, int n_hotwords, pfhip_out* out) {
  return offline_forward_rate(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, out);
}
// 16-bit PCM at the caller's rate (Audio::LoadPcmwav + WavResample, audio.cpp:787-819, 259-284): converted by the resampler's loads
pfhip_status pfhip_offline_forward_rate_s16(pfhip_model* head, const int16_t* const* pcm, const int* n_samples, int batch,
                                            int sample_rate, const float* hw_emb, int n_hotwords, pfhip_out* out) {
  return offline_forward_rate(head, pcm, n_samples, batch, sample_rate, hw_emb, n_hotwords, out);
}

pfhip_status pfhip_resample(pfhip_model* head, const float* const* pcm, const int* n_samples, int batch, int fs_in, float* const* out,
                            const int* cap, int* n_out) {
  g_err.clear();
  if (!head || !pcm || !n_samples || batch <= 0 || !out || !cap || !n_out) return fail(PFHIP_ERR_ARG, "bad argument");
  const int fs_out = head->weights->cfg.sample_rate;
  std::string why;
  if (!pfhip_impl::resample_supported(fs_in, fs_out, &why)) return fail(PFHIP_ERR_UNSUPPORTED, why);
  bool short_cap = false;
  for (int b = 0; b < batch; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    const int64_t no = pfhip_impl::resample_out_len(fs_in, fs_out, n_samples[b]);
    if (no > INT32_MAX) return fail(PFHIP_ERR_ARG, "resampled utterance too long");
    n_out[b] = (int)no;
    if (no > 0 && (cap[b] < no || !out[b])) short_cap = true;
  }
  if (short_cap) return fail(PFHIP_ERR_CAPACITY, "output buffer smaller than the resampled length (n_out holds it)");
  if (fs_in == fs_out) {        // identity: a copy, no kernel (the reference skips WavResample, audio.cpp:808-810)
    for (int b = 0; b < batch; ++b)
      if (n_samples[b]) std::memcpy(out[b], pcm[b], (size_t)n_samples[b] * 4);
    return PFHIP_OK;
  }
  pfhip_model* m = acquire_slot(head);
  pfhip_status st;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    st = [&]() -> pfhip_status {
      HIP_TRY(hipSetDevice(m->device));
      hipStream_t s = m->own_stream;
      std::vector<int64_t> off;
      std::vector<int> n_rs;
      const pfhip_status ss = stage_resampled(m, pcm, n_samples, batch, fs_in, s, off, n_rs);
      if (ss) return ss;
      for (int b = 0; b < batch; ++b)
        if (n_rs[b]) HIP_TRY(hipMemcpyAsync(out[b], m->pcm.f() + off[b], (size_t)n_rs[b] * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      return PFHIP_OK;
    }();
  }
  release_slot(head, m);
  return st;
}

}  // extern "C"
