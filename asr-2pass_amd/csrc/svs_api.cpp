// SenseVoiceSmall, offline: the packed forward with its range-guard re-run, and CTC forced alignment against its rows.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "offline.h"
#include "ctx_graph.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

// pfhip_svs_align: per handle (its uid), where this thread's last pfhip_svs_forward on it ran — the context's uid and that context's
// forward count then, and the caller's utterances within that forward: a lone caller's are all of them, a merged caller's the
// sub-range [u0, u0 + batch) of the packed batch.  Handles come and go; the note is emptied when it has grown past 64 handles.
struct SvsNote { uint64_t ctx_uid, serial; int u0, batch; };
thread_local std::map<uint64_t, SvsNote> tl_svs_notes;
// pfhip_debug_poke "svs_unfused_rows": the rows that went through the unfused head chunks in the forward which served the calling
// thread's last pfhip_svs_forward — taken while that forward still held its context, so no later forward there changes it
thread_local long long tl_unfused_rows = 0;
thread_local int tl_forward_calls = 0;      // "svs_forward_calls": the callers that same forward served
thread_local int tl_topk_k = 0;             // "svs_topk_k": the stride of its k best columns (0: the greedy head)
void keep_note(const pfhip_model* head, uint64_t ctx_uid, uint64_t serial, int u0, int batch) {
  if (tl_svs_notes.size() > 64) tl_svs_notes.clear();
  tl_svs_notes[head->uid] = SvsNote{ctx_uid, serial, u0, batch};
}

int rows_of(const pfhip_model* m, int n_samples) {      // forward_encoder's count: T + 4 prompt rows, or none at all
  const int F = n_samples < 400 ? 0 : 1 + (n_samples - 400) / 160;
  const int T = (F + m->weights->cfg.lfr_n - 1) / m->weights->cfg.lfr_n;
  return T > 0 ? T + 4 : 0;
}

// The search's descriptors for a packed batch: per utterance its beams and the index of its graph in `graphs`, where a graph
// appears once however many callers brought it — the same handle, or another handle with the same content.
struct BeamPlan {
  std::vector<pfhip::BeamUtt> utt;
  std::vector<const pfhip_ctx_graph*> graphs;
  int graph_index(const pfhip_ctx_graph* g) {
    if (!g) return -1;
    for (size_t i = 0; i < graphs.size(); ++i)
      if (graphs[i] == g) return (int)i;
    for (size_t i = 0; i < graphs.size(); ++i)
      if (graphs[i]->vocab == g->vocab && graphs[i]->packed == g->packed) return (int)i;
    graphs.push_back(g);
    return (int)graphs.size() - 1;
  }
  // a caller's utterances: set_of == nullptr: all on sets[0]; sets == nullptr: a greedy caller, no search
  void add(const pfhip_svs_beam_opts* sets, const int32_t* set_of, int batch) {
    for (int b = 0; b < batch; ++b) {
      const int k = !sets ? -1 : set_of ? set_of[b] : 0;
      if (k < 0) { utt.push_back(pfhip::BeamUtt{0, 0, 0, -1}); continue; }
      utt.push_back(pfhip::BeamUtt{sets[k].first_beam, sets[k].second_beam, sets[k].nbest, graph_index(sets[k].graph)});
    }
  }
  // the hypothesis stride of utterances [u0, u0 + n): the largest nbest among those that search (1 if none)
  int stride(int u0, int n) const {
    int s = 1;
    for (int u = u0; u < u0 + n; ++u)
      if (utt[(size_t)u].first_beam > 0) s = std::max(s, utt[(size_t)u].nbest);
    return s;
  }
};

// a beam caller alone on slot m, with its own buffers: the one-set form as ever (its graph goes up with the call), the sets form
// through the descriptors
pfhip_status beam_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid, const int32_t* textnorm,
                         pfhip_svs_out* out, const pfhip_svs_beam_opts* sets, const int32_t* set_of, pfhip_svs_beam_out* bo, SvsMerge* mg) {
  SvsBeam beam;
  beam.out = bo;
  if (!set_of) {
    beam.opts = sets;
    return svs_forward_direct(m, pcm, n_samples, batch, lid, textnorm, out, nullptr, mg, &beam);
  }
  BeamPlan plan;
  plan.add(sets, set_of, batch);
  beam.utt = plan.utt.data(); beam.graphs = plan.graphs.data(); beam.n_graphs = (int)plan.graphs.size();
  return svs_forward_direct(m, pcm, n_samples, batch, lid, textnorm, out, nullptr, mg, &beam);
}

// One packed forward on `m` for everybody in `take` (one sample format: pool_submit's pick).  Every caller keeps its own lid /
// textnorm per utterance and its own buffers; the forward's results are staged here and dealt out, a caller whose buffers are too
// small fails alone.  Full log-prob rows go from the device straight into the buffer of the caller who asked (heads.cpp runs the
// unfused chunks over those utterances' rows only); spans are formed for the utterances of the callers who brought a span buffer.
void run_svs_requests(pfhip_model* m, const std::vector<BatchReq*>& all_taken) {
  const int V = m->weights->cfg.vocab;
  std::vector<BatchReq*> take;
  for (BatchReq* r : all_taken) {
    r->ran_on = m;
    r->company = 0;
    if (r->sout->logp) {                              // known before anything is launched, as for a lone caller
      size_t rows = 0;
      for (int i = 0; i < r->batch; ++i) rows += (size_t)rows_of(m, r->n[i]);
      if (rows * (size_t)V > r->sout->logp_cap_floats) {
        r->st = PFHIP_ERR_CAPACITY; r->err = "logp_cap_floats smaller than rows x vocabulary"; continue;
      }
    }
    take.push_back(r);
  }
  if (take.empty()) return;
  for (BatchReq* r : take) r->company = (int)take.size();
  if (take.size() == 1) {                             // nobody to share with: the caller's own buffers, as without the queue
    BatchReq* r = take.front();
    SvsMerge mg;
    r->st = r->bout ? beam_direct(m, r->pcm, r->n, r->batch, r->lid, r->textnorm, r->sout, r->sets, r->set_of, r->bout, &mg)
                    : svs_forward_direct(m, r->pcm, r->n, r->batch, r->lid, r->textnorm, r->sout, r->spans, &mg);
    r->err = g_err; r->serial = mg.serial; r->u0 = 0; r->unfused_rows = mg.unfused_rows; r->topk_k = mg.topk_k;
    return;
  }
  std::vector<const void*> ptrs; std::vector<int> lens, rows; std::vector<int32_t> lid, tn;
  std::vector<char> span_want; std::vector<float*> logp_rows;
  bool any_spans = false, any_logp = false, any_beam = false;
  int cap = 1; size_t M = 0;
  BeamPlan plan;                                      // a greedy caller's utterances do not search
  for (BatchReq* r : take) {
    r->u0 = (int)lens.size();
    plan.add(r->bout ? r->sets : nullptr, r->set_of, r->batch);
    any_beam = any_beam || r->bout;
    size_t row_in_req = 0;
    for (int i = 0; i < r->batch; ++i) {
      const int T = rows_of(m, r->n[i]);
      ptrs.push_back(r->pcm.p[i]); lens.push_back(r->n[i]); rows.push_back(T); lid.push_back(r->lid[i]); tn.push_back(r->textnorm[i]);
      span_want.push_back(r->spans ? 1 : 0);
      logp_rows.push_back(r->sout->logp && T ? r->sout->logp + row_in_req * V : nullptr);
      row_in_req += (size_t)T; M += (size_t)T; cap = std::max(cap, T);
    }
    any_spans = any_spans || r->spans; any_logp = any_logp || r->sout->logp;
  }
  const int utts = (int)lens.size();
  std::vector<int32_t> ids((size_t)utts * cap), frames(ids.size()), num(utts), flen(utts), fid(std::max<size_t>(M, 1));
  std::vector<float> tlogp(ids.size()), flp(fid.size());
  pfhip_svs_out all{};
  all.ids = ids.data(); all.token_num = num.data(); all.max_tokens = cap; all.tok_frame = frames.data(); all.tok_logp = tlogp.data();
  all.frame_ids = fid.data(); all.frame_logp = flp.data(); all.frame_len = flen.data();
  std::vector<int32_t> sb, se; std::vector<float> sl, ss;
  pfhip_svs_align_out sp{};
  if (any_spans) {
    sb.assign(ids.size(), -1); se.assign(ids.size(), -1); sl.assign(ids.size(), -INFINITY); ss.assign(utts, 0.f);
    sp.tok_begin = sb.data(); sp.tok_end = se.data(); sp.tok_logp = sl.data(); sp.score = ss.data(); sp.max_tokens = cap;
  }
  SvsMerge mg;
  mg.span_want = any_spans ? span_want.data() : nullptr;
  mg.logp_rows = any_logp ? logp_rows.data() : nullptr;
  // the beam callers' hypotheses, staged at the forward's own stride (the largest nbest among the searching utterances) with room
  // for as many tokens as the longest utterance has rows; every caller is dealt its own at its own stride below
  const int bstride = plan.stride(0, utts);
  std::vector<int32_t> b_nhyp, b_ntok, b_ids;
  std::vector<float> b_score, b_ctc, b_ctx;
  pfhip_svs_beam_out ball{};
  SvsBeam beam;
  if (any_beam) {
    const size_t bn = (size_t)utts * bstride;
    b_nhyp.assign(utts, 0); b_ntok.assign(bn, 0); b_ids.assign(bn * cap, -1);
    b_score.assign(bn, -INFINITY); b_ctc.assign(bn, -INFINITY); b_ctx.assign(bn, 0.f);
    ball.n_hyp = b_nhyp.data(); ball.n_tokens = b_ntok.data(); ball.ids = b_ids.data(); ball.max_tokens = cap;
    ball.score = b_score.data(); ball.ctc_score = b_ctc.data(); ball.ctx_score = b_ctx.data();
    beam.out = &ball; beam.utt = plan.utt.data(); beam.graphs = plan.graphs.data(); beam.n_graphs = (int)plan.graphs.size();
  }
  const pfhip_status st = svs_forward_direct(m, HostPcm(ptrs.data(), take.front()->pcm.s16), lens.data(), utts, lid.data(), tn.data(), &all,
                                             any_spans ? &sp : nullptr, &mg, any_beam ? &beam : nullptr);
  const std::string err = g_err;
  std::vector<size_t> row_off(utts + 1, 0);
  for (int u = 0; u < utts; ++u) row_off[u + 1] = row_off[u] + (size_t)rows[u];
  for (BatchReq* r : take) {
    r->st = st; r->err = err; r->serial = mg.serial; r->unfused_rows = mg.unfused_rows; r->topk_k = mg.topk_k;
    if (st) continue;
    pfhip_svs_out* o = r->sout;
    int longest = 0;
    for (int i = 0; i < r->batch; ++i) {
      if (o->token_num) o->token_num[i] = num[r->u0 + i];
      if (o->frame_len) o->frame_len[i] = flen[r->u0 + i];
      longest = std::max(longest, num[r->u0 + i]);
    }
    if (r->bout) {                                    // n_hyp, the lengths and the scores also where max_tokens turns out too small
      pfhip_svs_beam_out* bo = r->bout;
      const int rs = plan.stride(r->u0, r->batch);
      int longest_hyp = 0;
      for (int i = 0; i < r->batch; ++i) {
        const int u = r->u0 + i;
        bo->n_hyp[i] = b_nhyp[u];
        for (int j = 0; j < rs; ++j) {
          const size_t src = (size_t)u * bstride + j, dst = (size_t)i * rs + j;
          bo->n_tokens[dst] = b_ntok[src];
          if (bo->score) bo->score[dst] = b_score[src];
          if (bo->ctc_score) bo->ctc_score[dst] = b_ctc[src];
          if (bo->ctx_score) bo->ctx_score[dst] = b_ctx[src];
          if (j < b_nhyp[u]) longest_hyp = std::max(longest_hyp, b_ntok[src]);
        }
      }
      if (bo->max_tokens < longest_hyp) {
        r->st = PFHIP_ERR_CAPACITY; r->err = "beam: max_tokens smaller than the longest hypothesis (n_tokens holds the lengths)"; continue;
      }
      for (int i = 0; i < r->batch; ++i)
        for (int j = 0; j < rs; ++j) {
          const size_t src = (size_t)(r->u0 + i) * bstride + j, dst = (size_t)i * rs + j;
          const int n = std::min(std::max(b_ntok[src], 0), cap);
          std::memcpy(bo->ids + dst * bo->max_tokens, b_ids.data() + src * cap, (size_t)n * 4);
        }
    }
    if ((o->ids || o->tok_frame || o->tok_logp) && o->max_tokens < longest) {
      r->st = PFHIP_ERR_CAPACITY; r->err = "max_tokens smaller than the longest token sequence"; continue;
    }
    if (r->spans && r->spans->max_tokens < longest - 4) {
      r->st = PFHIP_ERR_CAPACITY; r->err = "spans: max_tokens smaller than the longest token list"; continue;
    }
    for (int i = 0; i < r->batch; ++i) {
      const int u = r->u0 + i;
      const size_t n = (size_t)num[u], src = (size_t)u * cap, dst = (size_t)i * o->max_tokens;
      if (o->ids) std::memcpy(o->ids + dst, ids.data() + src, n * 4);
      if (o->tok_frame) std::memcpy(o->tok_frame + dst, frames.data() + src, n * 4);
      if (o->tok_logp) std::memcpy(o->tok_logp + dst, tlogp.data() + src, n * 4);
      const size_t f0 = row_off[u] - row_off[r->u0];
      if (o->frame_ids) std::memcpy(o->frame_ids + f0, fid.data() + row_off[u], (size_t)rows[u] * 4);
      if (o->frame_logp) std::memcpy(o->frame_logp + f0, flp.data() + row_off[u], (size_t)rows[u] * 4);
      if (r->spans) {
        const size_t nt = n > 4 ? n - 4 : 0, sdst = (size_t)i * r->spans->max_tokens;
        std::memcpy(r->spans->tok_begin + sdst, sb.data() + src, nt * 4);
        std::memcpy(r->spans->tok_end + sdst, se.data() + src, nt * 4);
        if (r->spans->tok_logp) std::memcpy(r->spans->tok_logp + sdst, sl.data() + src, nt * 4);
        if (r->spans->score) r->spans->score[i] = ss[u];
      }
    }
  }
}

// leader or follower, after the queue: where the forward ran, and which of its utterances are this caller's (pfhip_svs_align, the
// debug read-outs)
void note_merged(pfhip_model* head, const BatchReq& me, int batch) {
  tl_unfused_rows = me.unfused_rows;
  tl_forward_calls = me.company;
  tl_topk_k = me.topk_k;
  if (me.ran_on) {
    last_replica() = me.ran_on;
    if (me.serial) keep_note(head, me.ran_on->uid, me.serial, me.u0, batch);
  }
}

pfhip_status svs_forward(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid, const int32_t* textnorm,
                                pfhip_svs_out* out, pfhip_svs_align_out* spans = nullptr) {
  g_err.clear();
  if (!head || !pcm.p || !n_samples || batch <= 0 || !lid || !textnorm || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (spans && (!spans->tok_begin || !spans->tok_end)) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(head)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: a Paraformer is run through pfhip_offline_forward");
  if (!head->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "multi-device groups are not built for SenseVoice (CTC) models");
  for (int b = 0; b < batch; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm.p[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    if (lid[b] < 0 || lid[b] > 15 || textnorm[b] < 0 || textnorm[b] > 15) return fail(PFHIP_ERR_ARG, "lid / textnorm outside 0..15");
  }
  bool merge;
  {
    std::lock_guard<std::mutex> l(head->bq.mu);
    merge = head->batch_wait_us > 0 && batch < head->batch_max_utts;
  }
  if (merge) {                                          // pfhip_svs_set_batching: merged with whoever else is calling (offline_api.cpp)
    BatchReq me;
    me.pcm = pcm; me.n = n_samples; me.batch = batch; me.lid = lid; me.textnorm = textnorm; me.sout = out; me.spans = spans;
    pool_submit(head, me, run_svs_requests);
    note_merged(head, me, batch);
    if (me.st != PFHIP_OK) g_err = me.err;
    return me.st;
  }
  pfhip_model* m = acquire_slot(head);                  // the least-loaded execution context
  last_replica() = m;
  tl_forward_calls = 1;
  const pfhip_status st = svs_forward_direct(m, pcm, n_samples, batch, lid, textnorm, out, spans);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}

}  // namespace

namespace pfhip_impl {

long long svs_last_unfused_rows() { return tl_unfused_rows; }
int svs_last_forward_calls() { return tl_forward_calls; }
int svs_last_topk_k() { return tl_topk_k; }
SvsNoteView svs_thread_note(pfhip_model* head) {
  SvsNoteView v;
  const auto note = tl_svs_notes.find(head->uid);
  if (note == tl_svs_notes.end()) return v;
  if (head->uid == note->second.ctx_uid) v.ctx = head;
  for (pfhip_model* cx : head->contexts)
    if (cx->uid == note->second.ctx_uid) v.ctx = cx;
  v.serial = note->second.serial; v.u0 = note->second.u0; v.batch = note->second.batch;
  return v;
}

// one packed forward on slot m, its range-guard re-run included, and the results into out
pfhip_status svs_forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid,
                                       const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans, SvsMerge* mg,
                                       const SvsBeam* beam) {
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
  m->svs_span_want.assign(spans ? (size_t)batch : 0, 1);      // the head aligns the greedy tokens behind its collapse (heads.cpp)
  if (spans && mg && mg->span_want) m->svs_span_want.assign(mg->span_want, mg->span_want + batch);
  m->svs_logp_rows.clear();
  if (mg && mg->logp_rows) m->svs_logp_rows.assign(mg->logp_rows, mg->logp_rows + batch);
  m->svs_span_mt = 0;
  // the search behind the head (heads.cpp); a range-guard re-run reads the same fields, so everything then belongs to the re-run
  const bool sets = beam && beam->utt;
  m->svs_beam_fb = beam && !sets ? beam->opts->first_beam : 0;
  m->svs_beam_sb = beam && !sets ? beam->opts->second_beam : 0;
  m->svs_beam_nbest = beam && !sets ? beam->opts->nbest : 0;
  m->svs_beam_graph = beam && !sets ? beam->opts->graph : nullptr;
  m->svs_beam_utt.clear(); m->svs_beam_graphs.clear(); m->svs_graph_dev.clear();
  struct GraphPins { pfhip_model* m; ~GraphPins() { svs_release_graphs(m); m->fw_lm = nullptr; } } pins{m};      // let go after the forward's last synchronise
  const std::shared_ptr<const TokenLm> lm = beam ? token_lm_of(m) : nullptr;      // pfhip_set_token_lm: the search walks it too
  m->fw_lm = lm.get();
  int beam_stride = beam && !sets ? beam->opts->nbest : 1;
  if (sets) {
    // every utterance on its own beams: the maxima are the head's k, the node stride and the hypothesis stride (no utterance
    // searching: the greedy head, no search launch); the graphs are pinned in the device's bank before the first launch
    int kmax = 0;
    for (int b = 0; b < batch; ++b) kmax = std::max(kmax, beam->utt[b].first_beam);
    if (kmax > 0) {
      if (!pfhip::ctc_prefix_beam_multi_check(beam->utt, batch, kmax, beam->n_graphs, &m->svs_beam_sb, &m->svs_beam_nbest))
        return fail(PFHIP_ERR_ARG, "beam: a set outside its bounds");
      m->svs_beam_fb = kmax;
      beam_stride = m->svs_beam_nbest;
      m->svs_beam_utt.assign(beam->utt, beam->utt + batch);
      m->svs_beam_graphs.assign(beam->graphs, beam->graphs + beam->n_graphs);
      st = svs_pin_graphs_locked(m, s);
      if (st) return st;
    }
  }
  st = enqueue_locked(m, PcmView{m->pcm.p, pcm.s16}, off.data(), n_samples, batch, s, false);
  if (!st && m->M > 0 && m->range_hit && !m->weights->always_exact) {      // the guard of the fp16 two-plane domain: redone once, exact
    ++m->range_fallbacks;
    m->exact_rerun = true;
    st = enqueue_locked(m, PcmView{m->pcm.p, pcm.s16}, off.data(), n_samples, batch, s, false);
    m->exact_rerun = false;
  }
  m->svs_logp_host = nullptr;
  const bool searched = m->svs_beam_fb > 0;
  m->svs_beam_fb = m->svs_beam_sb = m->svs_beam_nbest = 0;
  m->svs_beam_graph = nullptr;
  m->svs_beam_utt.clear(); m->svs_beam_graphs.clear(); m->svs_graph_dev.clear();
  m->svs_span_want.clear();
  m->svs_logp_rows.clear();
  (mg ? mg->unfused_rows : tl_unfused_rows) = st || m->M == 0 ? 0 : m->svs_unfused_rows;
  (mg ? mg->topk_k : tl_topk_k) = st || m->M == 0 ? 0 : m->svs_topk_k;
  if (st) return st;
  m->svs_fwd_ok = true;                          // the rows and their log-sum-exp are what pfhip_svs_align reads ...
  ++m->svs_serial;                               // ... for this thread, until this context runs another forward
  if (mg) mg->serial = m->svs_serial;            // (merged callers: each notes its own sub-range in its own thread)
  else keep_note(m->group_head ? m->group_head : m, m->uid, m->svs_serial, 0, batch);
  for (int b = 0; b < batch; ++b) {
    if (out->token_num) out->token_num[b] = m->M ? m->token_num[b] : 0;
    if (out->frame_len) out->frame_len[b] = m->T[b];
  }
  if (m->M == 0) {                                 // no rows at all: what pfhip_svs_align answers for no tokens against no rows
    for (int b = 0; spans && spans->score && b < batch; ++b) spans->score[b] = 0.f;
    for (int b = 0; beam && b < batch; ++b) beam->out->n_hyp[b] = 0;      // CtcSearch returns "" without searching
    return PFHIP_OK;
  }
  if (beam && !searched) {                         // the sets form with no utterance searching: the greedy head ran, nothing was searched
    pfhip_svs_beam_out* bo = beam->out;
    for (int b = 0; b < batch; ++b) {
      bo->n_hyp[b] = 0; bo->n_tokens[b] = 0;
      if (bo->score) bo->score[b] = -INFINITY;
      if (bo->ctc_score) bo->ctc_score[b] = -INFINITY;
      if (bo->ctx_score) bo->ctx_score[b] = 0.f;
    }
  } else if (beam) {                               // they came in the forward's one copy, behind the spans' words
    pfhip_svs_beam_out* bo = beam->out;
    const int nb = beam_stride, mt = m->svs_beam_mt;
    const size_t bn = (size_t)batch * nb;
    const int32_t *h_nhyp = m->h_counts.i() + m->svs_beam_word, *h_ntok = h_nhyp + batch, *h_ids = h_ntok + bn;
    const float *h_score = reinterpret_cast<const float*>(h_ids + bn * mt), *h_ctc = h_score + bn, *h_ctx = h_ctc + bn;
    int longest = 0;
    for (int b = 0; b < batch; ++b) {
      bo->n_hyp[b] = h_nhyp[b];
      for (int j = 0; j < nb; ++j) {
        const size_t o = (size_t)b * nb + j;
        bo->n_tokens[o] = h_ntok[o];               // the true length: what max_tokens must hold where the call ends in PFHIP_ERR_CAPACITY
        if (bo->score) bo->score[o] = h_score[o];
        if (bo->ctc_score) bo->ctc_score[o] = h_ctc[o];
        if (bo->ctx_score) bo->ctx_score[o] = h_ctx[o];
        if (j < h_nhyp[b]) longest = std::max(longest, h_ntok[o]);
      }
    }
    if (bo->max_tokens < longest) return fail(PFHIP_ERR_CAPACITY, "beam: max_tokens smaller than the longest hypothesis (n_tokens holds the lengths)");
    for (size_t o = 0; o < bn; ++o) {
      const int n = std::min(std::max(h_ntok[o], 0), mt);
      std::memcpy(bo->ids + o * bo->max_tokens, h_ids + o * mt, (size_t)n * 4);
    }
  }
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
  if (spans) {                                     // they came in the forward's one copy, behind its results
    const int mt = m->svs_span_mt;
    const size_t sbt = (size_t)batch * mt;
    const int32_t *s_begin = m->h_counts.i() + m->svs_span_word, *s_end = s_begin + sbt;
    const float *s_logp = reinterpret_cast<const float*>(s_end + sbt), *s_score = s_logp + sbt;
    for (int b = 0; b < batch; ++b)
      if (spans->max_tokens < m->token_num[b] - 4) return fail(PFHIP_ERR_CAPACITY, "spans: max_tokens smaller than the longest token list");
    for (int b = 0; b < batch; ++b) {
      const int n = std::max(m->token_num[b] - 4, 0);
      const size_t dst = (size_t)b * spans->max_tokens, src = (size_t)b * mt;
      for (int j = 0; j < n; ++j) {                // tok_frame's numbering: the prompt rows counted; beyond the slots: refused by the kernel
        const int32_t tb = j < mt ? s_begin[src + j] : -1, te = j < mt ? s_end[src + j] : -1;
        spans->tok_begin[dst + j] = tb < 0 ? -1 : tb + 4;
        spans->tok_end[dst + j] = te < 0 ? -1 : te + 4;
        if (spans->tok_logp) spans->tok_logp[dst + j] = j < mt ? s_logp[src + j] : -INFINITY;
      }
      if (spans->score) spans->score[b] = s_score[b];
    }
  }
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

// pfhip_set_batching's sibling for a CTC handle: the same queue, the same two knobs
pfhip_status pfhip_svs_set_batching(pfhip_model* m, int wait_us, int max_utterances) {
  g_err.clear();
  if (!m || wait_us < 0 || max_utterances < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(m)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: a Paraformer handle takes pfhip_set_batching");
  if (!m->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "multi-device groups are not built for SenseVoice (CTC) models");
  std::lock_guard<std::mutex> ql(m->bq.mu);
  m->batch_wait_us = wait_us;
  m->batch_max_utts = max_utterances;
  return PFHIP_OK;
}

pfhip_status pfhip_svs_forward(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                               const int32_t* textnorm, pfhip_svs_out* out) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out);
}
pfhip_status pfhip_svs_forward_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                   const int32_t* textnorm, pfhip_svs_out* out) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out);
}
// the forward with the spans of its greedy tokens (ids[b][4:]) in the same stream work, copy and synchronise; spans == NULL: the above
pfhip_status pfhip_svs_forward_spans(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                     const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out, spans);
}
pfhip_status pfhip_svs_forward_spans_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                         const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans) {
  return svs_forward(m, pcm, n_samples, batch, lid, textnorm, out, spans);
}

// The forward with the CTC prefix beam search (and hotwords) behind its head, in the same stream work, copy and synchronise: one set
// of options for all utterances (set_of == nullptr: pfhip_svs_forward_beam) or a set per utterance (pfhip_svs_forward_beam_sets).
// The merge queue of pfhip_svs_set_batching is passed by — the caller runs alone on a slot — unless pfhip_svs_set_beam_merging is on.
static pfhip_status svs_forward_beam(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid, const int32_t* textnorm,
                                     pfhip_svs_out* out, const pfhip_svs_beam_opts* sets, int n_sets, const int32_t* set_of,
                                     pfhip_svs_beam_out* bo) {
  g_err.clear();
  if (!head || !pcm.p || !n_samples || batch <= 0 || !lid || !textnorm || !out || !sets || n_sets < 1 || !bo) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(head)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: there are no CTC rows to search");
  if (!head->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "multi-device groups are not built for SenseVoice (CTC) models");
  std::vector<char> used((size_t)n_sets, set_of ? 0 : 1);
  for (int b = 0; set_of && b < batch; ++b) {
    if (set_of[b] < -1 || set_of[b] >= n_sets) return fail(PFHIP_ERR_ARG, "beam: set_of names no set");
    if (set_of[b] >= 0) used[(size_t)set_of[b]] = 1;
  }
  for (int k = 0; k < n_sets; ++k) {
    const pfhip_svs_beam_opts* opts = sets + k;
    if (!used[(size_t)k]) continue;
    if (opts->first_beam < 1 || opts->first_beam > pfhip::kBeamMax || opts->second_beam < 1 || opts->second_beam > pfhip::kBeamMax)
      return fail(PFHIP_ERR_ARG, "beam: first_beam and second_beam must lie in 1..16");
    if (opts->nbest < 1 || opts->nbest > opts->second_beam) return fail(PFHIP_ERR_ARG, "beam: nbest must lie in 1..second_beam");
    if (opts->first_beam > head->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "beam: first_beam larger than the vocabulary");
    if (opts->graph && opts->graph->vocab != head->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "beam: the context graph was built for another vocabulary");
  }
  if (!bo->n_hyp || !bo->n_tokens || bo->max_tokens < 0 || (bo->max_tokens > 0 && !bo->ids)) return fail(PFHIP_ERR_ARG, "beam: a result buffer is missing");
  for (int b = 0; b < batch; ++b) {
    if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm.p[b])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    if (lid[b] < 0 || lid[b] > 15 || textnorm[b] < 0 || textnorm[b] > 15) return fail(PFHIP_ERR_ARG, "lid / textnorm outside 0..15");
  }
  bool merge;
  {
    std::lock_guard<std::mutex> l(head->bq.mu);
    merge = head->beam_merge && head->batch_wait_us > 0 && batch < head->batch_max_utts;
  }
  if (merge) {                                          // pfhip_svs_set_beam_merging: in the queue like a greedy caller
    BatchReq me;
    me.pcm = pcm; me.n = n_samples; me.batch = batch; me.lid = lid; me.textnorm = textnorm; me.sout = out;
    me.sets = sets; me.n_sets = n_sets; me.set_of = set_of; me.bout = bo;
    pool_submit(head, me, run_svs_requests);
    note_merged(head, me, batch);
    if (me.st != PFHIP_OK) g_err = me.err;
    return me.st;
  }
  pfhip_model* m = acquire_slot(head);
  last_replica() = m;
  tl_forward_calls = 1;
  const pfhip_status st = beam_direct(m, pcm, n_samples, batch, lid, textnorm, out, sets, set_of, bo, nullptr);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
}
pfhip_status pfhip_svs_forward_beam(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                    const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* opts, pfhip_svs_beam_out* beam) {
  return svs_forward_beam(m, pcm, n_samples, batch, lid, textnorm, out, opts, 1, nullptr, beam);
}
pfhip_status pfhip_svs_forward_beam_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                        const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* opts, pfhip_svs_beam_out* beam) {
  return svs_forward_beam(m, pcm, n_samples, batch, lid, textnorm, out, opts, 1, nullptr, beam);
}
pfhip_status pfhip_svs_forward_beam_sets(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                         const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* sets, int n_sets,
                                         const int32_t* set_of, pfhip_svs_beam_out* beam) {
  if (!set_of) return fail(PFHIP_ERR_ARG, "bad argument");
  return svs_forward_beam(m, pcm, n_samples, batch, lid, textnorm, out, sets, n_sets, set_of, beam);
}
pfhip_status pfhip_svs_forward_beam_sets_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                             const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* sets, int n_sets,
                                             const int32_t* set_of, pfhip_svs_beam_out* beam) {
  if (!set_of) return fail(PFHIP_ERR_ARG, "bad argument");
  return svs_forward_beam(m, pcm, n_samples, batch, lid, textnorm, out, sets, n_sets, set_of, beam);
}
// pfhip_set_hotword_merging's sibling: beam callers join the queue of pfhip_svs_set_batching
pfhip_status pfhip_svs_set_beam_merging(pfhip_model* m, int on) {
  g_err.clear();
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  if (!is_svs(m)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: there is no search to merge");
  std::lock_guard<std::mutex> l(m->bq.mu);
  m->beam_merge = on != 0;
  return PFHIP_OK;
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
  // the caller's utterances within that forward: all of a lone forward, its own sub-range of a merged one (never another caller's rows)
  const int u0 = note->second.u0;
  if (batch != note->second.batch || u0 < 0 || u0 + batch > m->B)
    return fail(PFHIP_ERR_ARG, "batch differs from that of the last pfhip_svs_forward");
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
    const int N = m->T[u0 + b] > 4 ? m->T[u0 + b] - 4 : 0;           // the speech rows: the four prompt rows are no CTC rows
    hm[b] = m->row_off[u0 + b] + 4; hm[B + b] = N; hm[2 * B + b] = (int)lo; hm[3 * B + b] = n_tokens[b];
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
