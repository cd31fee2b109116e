// The CTC, timestamp and vocabulary heads, and the fetch of a forward's results with the range guard's re-run.
#include <algorithm>
#include <cstring>
#include <vector>

#include "offline.h"
#include "ctx_graph.h"
#include "beam_front.h"
#include "launch_common.h"

namespace {
using namespace pfhip_impl;

constexpr int kSvsChunkRows = 2048;

// ---- a6 producer: CifPredictorV3.get_upsample_timestmap on the encoder output of the batch just run -------------------
pfhip_status ts_head_locked(pfhip_model* m, hipStream_t s, bool stepwise_only = false) {
  ForwardCtx fc(m);
  const Config& c = m->weights->cfg;
  const TimestampHead& ts = m->weights->ts;
  if (!c.timestamp) return fail(PFHIP_ERR_UNSUPPORTED, "model has no timestamp head (us_alphas / us_cif_peak outputs)");
  if (m->have_ts) return PFHIP_OK;
  const int d = c.d_model, B = m->B, M = m->M;
  if (M == 0) { m->have_ts = true; return PFHIP_OK; }
  const int Mp = round_up(M, pfhip::kTileM), R = 3 * M, Rp = 3 * Mp;
  HIP_TRY(m->ts_up.ensure((size_t)Rp * d * 4));
  HIP_TRY(m->ts_gx.ensure((size_t)Rp * 8 * d * 4));
  HIP_TRY(m->ts_y.ensure((size_t)Rp * 2 * d * 4));
  if (m->ts_hx.cap < (size_t)pfhip::kBlstmScratchFloats * 4) {
    HIP_TRY(m->ts_hx.ensure((size_t)pfhip::kBlstmScratchFloats * 4));
    HIP_TRY(hipMemsetAsync(m->ts_hx.p, 0, (size_t)pfhip::kBlstmScratchFloats * 4, s));
  }
  // the kernel's error flag is per call: a barrier time-out of an earlier request must not fail this one
  HIP_TRY(hipMemsetAsync(m->ts_hx.f() + pfhip::kBlstmFlagWord, 0, 4, s));
  if (m->debug_blstm_flag) {          // test hook (pfhip_debug_poke): this request sees the flag raised, as after a barrier time-out
    const unsigned one = 1u;
    HIP_TRY(hipMemcpyAsync(m->ts_hx.f() + pfhip::kBlstmFlagWord, &one, 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    m->debug_blstm_flag = 0;
  }
  HIP_TRY(m->ts_a2.ensure((size_t)R * 4));
  HIP_TRY(m->ts_alphas.ensure((size_t)R * 4));
  HIP_TRY(m->ts_peaks.ensure((size_t)R * 4));
  // upsampled offsets / lengths / token counts per utterance
  HIP_TRY(m->ts_meta.ensure((size_t)3 * B * 4));
  std::vector<int> hm((size_t)3 * B);
  int maxL = 0;
  for (int b = 0; b < B; ++b) {
    hm[b] = 3 * m->row_off[b]; hm[B + b] = 3 * m->T[b]; hm[2 * B + b] = m->token_num[b];
    maxL = std::max(maxL, 3 * m->T[b]);
  }
  HIP_TRY(hipMemcpyAsync(m->ts_meta.p, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));          // hm is a stack buffer
  const int* d_off = m->ts_meta.i();
  const int* d_len = d_off + B;
  const int* d_tok = d_off + 2 * B;
  // ConvTranspose1d: [M, d] x [3d, d]^T -> [M, 3d] == [3M, d]
  gemm(m, s, m->enc.f(), d, ts.up, 3 * d, d, d, m->ts_up.f(), 3 * d, nullptr, 0, nullptr, 0, M, false);
  // input projections of both directions: [3M, d] x [8d, d]^T -> [3M, 8d]
  gemm(m, s, m->ts_up.f(), d, ts.ih, 8 * d, d, d, m->ts_gx.f(), 8 * d, nullptr, 0, nullptr, 0, R, false);
  {
    Scope sc(m, s, K_OTHER, 2.0 * R * 8 * d * d, 4.0 * R * 10 * d);
    // The recurrence advances up to 32 utterances together.  First the persistent kernel (one launch, 9 us per step); if its
    // step barrier could not be served — the 32 blocks of a direction were not co-resident on one XCD because other work holds
    // CUs there — the request is NOT failed: the same recurrence is redone as one launch per step (blstm.hip), which needs no
    // co-residency and gives the same values bit for bit.  PFHIP_BLSTM_STEPWISE=1 skips the persistent attempt.
    static const bool force_stepwise = pfhip::env_is1("PFHIP_BLSTM_STEPWISE");
    auto recurrence = [&](bool stepwise, hipStream_t rs) -> pfhip_status {
      for (int b0 = 0; b0 < B; b0 += 32) {
        const int nb = std::min(32, B - b0);
        int lmax = 0;
        for (int b = b0; b < b0 + nb; ++b) lmax = std::max(lmax, 3 * m->T[b]);
        if (stepwise)
          HIP_TRY(pfhip::launch_blstm_stepwise(m->ts_gx.f(), ts.whh, m->ts_y.f(), m->ts_hx.f(), m->ts_cst.f(), d_off + b0, d_len + b0, nb,
                                               lmax, rs));
        else
          HIP_TRY(pfhip::launch_blstm(m->ts_gx.f(), ts.whh, m->ts_y.f(), m->ts_hx.f(), d_off + b0, d_len + b0, nb, lmax, rs));
      }
      return PFHIP_OK;
    };
    HIP_TRY(m->ts_cst.ensure((size_t)2 * 32 * 512 * 4));
    m->ts_persistent = false;
    if (!stepwise_only && !force_stepwise) {
      // The persistent kernel wants the 32 blocks of a direction co-resident on one XCD: two contexts of a device must not run it
      // at the same time (they would time each other out into the per-step form).  Round 3 held a host lock from the launch to the
      // end of the stream — the whole rest of the caller's forward — so the contexts of a timestamp model took turns and three
      // batches in flight were slower than one (bench.c4: 58 ms against 38).  Now every context of a device enqueues its recurrence
      // on ONE stream of that device (events tie it to the caller's stream), so the device orders them and the lock covers the
      // enqueue only; the kernel's error word travels to the host with the results (fetch_once), and a raised one redoes the
      // recurrence per step there.
      pfhip_model* owner = m->weights_of ? m->weights_of : m;
      static std::mutex blstm_mu[64];
      {
        std::lock_guard<std::mutex> bl(blstm_mu[m->device & 63]);
        if (!owner->blstm_stream) HIP_TRY(hipStreamCreateWithFlags(&owner->blstm_stream, hipStreamNonBlocking));
        if (!m->ev_ts_in) {
          HIP_TRY(hipEventCreateWithFlags(&m->ev_ts_in, hipEventDisableTiming));
          HIP_TRY(hipEventCreateWithFlags(&m->ev_ts_out, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(m->ev_ts_in, s));
        HIP_TRY(hipStreamWaitEvent(owner->blstm_stream, m->ev_ts_in, 0));
        pfhip_status st = recurrence(false, owner->blstm_stream);
        if (st) return st;
        HIP_TRY(hipEventRecord(m->ev_ts_out, owner->blstm_stream));
      }
      HIP_TRY(hipStreamWaitEvent(s, m->ev_ts_out, 0));
      m->ts_persistent = true;
    } else {
      pfhip_status st = recurrence(true, s);
      if (st) return st;
    }
    pfhip::launch_alpha2(m->ts_y.f(), 2 * d, ts.out2_w, ts.out2_b, c.smooth_factor2, c.noise_threshold2,
                         m->ts_a2.f(), R, 2 * d, s);
    pfhip::launch_us_cif(m->ts_a2.f(), d_off, d_len, d_tok, B, maxL, c.cif_threshold - 1e-4f, m->ts_alphas.f(),
                         m->ts_peaks.f(), s);
  }
  HIP_TRY(hipGetLastError());
  m->have_ts = true;
  return PFHIP_OK;
}

// ---- pfhip_offline_forward_bias: the search over the candidates the top-k head just left (nar_beam.hip) --------------------------
// Rows: utterance b's token rows [tok_off[b], + min(n_fires[b], token_num[b])) of nb_ids / nb_logp [ML][nbest_k], all three read from
// the device's own arrays (dmeta, and the CIF's counts).  Descriptors, the graph table and the graphs' images go to the front of the
// search's workspace in one copy from pinned staging.  Results: bias_res, laid out as internal.h says.
size_t bias_words(int B, int ns, int mt) { return (size_t)B + (size_t)B * ns * (4 + (size_t)mt); }
pfhip_status bias_search_locked(pfhip_model* m, hipStream_t s) {
  const NarBias& nb = *m->bias;
  const int B = m->B, ML = m->ML, k = m->nbest_k, ns = nb.nbest_stride, mt = m->maxL;
  const size_t front = pfhip::beam_front_bytes(B, nb.graphs, nb.n_graphs), nodes = pfhip::nbest_ctx_beam_workspace_bytes(ML, B, nb.beam_stride);
  const size_t words = bias_words(B, ns, mt);
  HIP_TRY(m->bias_ws.ensure(front + nodes));
  HIP_TRY(m->bias_stage.ensure(front));
  HIP_TRY(m->bias_res.ensure(words * 4));
  HIP_TRY(m->h_bias.ensure(words * 4));
  m->bias_mt = mt;
  char* const dev = static_cast<char*>(m->bias_ws.p);
  char* const stage = static_cast<char*>(m->bias_stage.p);
  std::memset(stage, 0, front);
  pfhip::beam_front_fill(stage, dev, nb.utt, B, nb.graphs, nb.n_graphs);
  HIP_TRY(hipMemcpyAsync(dev, stage, front, hipMemcpyHostToDevice, s));
  const size_t bn = (size_t)B * ns;
  int32_t *r_nhyp = m->bias_res.i(), *r_ntok = r_nhyp + B, *r_ids = r_ntok + bn;
  float *r_score = reinterpret_cast<float*>(r_ids + bn * mt), *r_am = r_score + bn, *r_ctx = r_am + bn;
  Scope sc(m, s, K_HEAD, 0, 8.0 * ML * k + 8.0 * ML * nb.beam_stride);
  m->beam_lm_stride = 0;
  if (m->fw_lm) {
    // pfhip_set_token_lm: the instantiation that walks the model, whose image lies on the device already; each hypothesis's share of
    // the total stays on the device for pfhip_get_tensor "beam_lm_score"
    HIP_TRY(m->beam_lm.ensure(std::max<size_t>(bn, 1) * 4));
    if (!pfhip::launch_nbest_ctx_beam_lm(m->nb_ids.i(), m->nb_logp.f(), k, ML, m->m_tok_off, m->m_tok_len, m->counts.i() + B, B, m->weights->cfg.vocab,
                                         reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                         reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), nb.n_graphs,
                                         m->fw_lm->dev, nb.beam_stride, ns, mt, r_nhyp, r_ids, r_ntok, r_score, r_am, r_ctx, m->beam_lm.f(),
                                         dev + front, nodes, s))
      return fail(PFHIP_ERR_ARG, "hotword beam search with a language model refused its arguments");
    m->beam_lm_stride = ns;
    m->beam_lm_nbest.resize((size_t)B);
    for (int b = 0; b < B; ++b) m->beam_lm_nbest[(size_t)b] = nb.utt[b].first_beam > 0 ? nb.utt[b].nbest : 0;
    return PFHIP_OK;
  }
  if (!pfhip::launch_nbest_ctx_beam(m->nb_ids.i(), m->nb_logp.f(), k, ML, m->m_tok_off, m->m_tok_len, m->counts.i() + B, B, m->weights->cfg.vocab,
                                    reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                    reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), nb.n_graphs,
                                    nb.beam_stride, ns, mt, r_nhyp, r_ids, r_ntok, r_score, r_am, r_ctx, dev + front, nodes, s))
    return fail(PFHIP_ERR_ARG, "hotword beam search refused its arguments");
  return PFHIP_OK;
}
// after the synchronise behind the copy of bias_res: the caller's buffers.  n_hyp, the lengths and the scores also where max_tokens
// turns out too small.
pfhip_status scatter_bias(const pfhip_model* m) {
  pfhip_bias_out* bo = m->bias->out;
  const int B = m->B, ns = m->bias->nbest_stride, mt = m->bias_mt;
  const size_t bn = (size_t)B * ns;
  const int32_t *h_nhyp = m->h_bias.i(), *h_ntok = h_nhyp + B, *h_ids = h_ntok + bn;
  const float *h_score = reinterpret_cast<const float*>(h_ids + bn * mt), *h_am = h_score + bn, *h_ctx = h_am + bn;
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    bo->n_hyp[b] = h_nhyp[b];
    for (int j = 0; j < ns; ++j) {
      const size_t o = (size_t)b * ns + j;
      bo->n_tokens[o] = h_ntok[o];
      if (bo->score) bo->score[o] = h_score[o];
      if (bo->am_score) bo->am_score[o] = h_am[o];
      if (bo->ctx_score) bo->ctx_score[o] = h_ctx[o];
      if (j < h_nhyp[b]) longest = std::max(longest, h_ntok[o]);
    }
  }
  if (bo->max_tokens < longest) return fail(PFHIP_ERR_CAPACITY, "bias: max_tokens smaller than the longest hypothesis (n_tokens holds the lengths)");
  for (size_t o = 0; o < bn; ++o) {
    const int n = std::min(std::max(h_ntok[o], 0), mt);
    if (n) std::memcpy(bo->ids + o * bo->max_tokens, h_ids + o * mt, (size_t)n * 4);
  }
  return PFHIP_OK;
}

// the range flag of the forward crosses to the host with the results (one 4-byte copy in front of the sync that is there anyway)
pfhip_status read_range_flag(pfhip_model* m, hipStream_t s, bool sync) {
  m->range_hit = 0;
  if (!m->d_range_flag) return PFHIP_OK;
  HIP_TRY(m->h_flag.ensure(32));
  *m->h_flag.i() = 0;
  HIP_TRY(hipMemcpyAsync(m->h_flag.p, m->d_range_flag, 4, hipMemcpyDeviceToHost, s));
  if (sync) HIP_TRY(hipStreamSynchronize(s));
  return PFHIP_OK;
}

pfhip_status fetch_once(pfhip_model* m, pfhip_out* out, hipStream_t s, const pfhip_detail* dt) {
  if (!out) return fail(PFHIP_ERR_ARG, "null out");
  const int nk = dt ? dt->nbest_k : 0;
  int32_t* fire = dt ? dt->fire_frame : nullptr;
  if (nk && (nk < 1 || nk > m->nbest_k || !dt->nbest_ids || !dt->nbest_logp)) return fail(PFHIP_ERR_ARG, "bad nbest argument");
  if (fire && m->M > 0 && !m->have_fires) return fail(PFHIP_ERR_ARG, "the forward recorded no fire frames");
  m->nbest_fetch_max_tokens = out->max_tokens;
  ForwardCtx fc(m);
  const int B = m->B;
  for (int b = 0; b < B; ++b) {
    if (out->token_num) out->token_num[b] = m->token_num[b];
    if (out->n_fires) out->n_fires[b] = m->n_fires[b];
    if (out->n_frames) out->n_frames[b] = m->T[b];
  }
  if (out->us_alphas || out->us_peaks || out->us_len) {
    for (int attempt = 0; attempt < 2; ++attempt) {
      pfhip_status st = ts_head_locked(m, s, attempt == 1);
      if (st) return st;
      for (int b = 0; b < B; ++b) {
        const int L = 3 * m->T[b];
        if (out->us_len) out->us_len[b] = L;
        if ((out->us_alphas || out->us_peaks) && out->max_us < L) return fail(PFHIP_ERR_CAPACITY, "max_us smaller than 3 x frames");
        if (out->us_alphas && L)
          HIP_TRY(hipMemcpyAsync(out->us_alphas + (size_t)b * out->max_us, m->ts_alphas.f() + (size_t)3 * m->row_off[b], (size_t)L * 4,
                                 hipMemcpyDeviceToHost, s));
        if (out->us_peaks && L)
          HIP_TRY(hipMemcpyAsync(out->us_peaks + (size_t)b * out->max_us, m->ts_peaks.f() + (size_t)3 * m->row_off[b], (size_t)L * 4,
                                 hipMemcpyDeviceToHost, s));
      }
      // the persistent recurrence's error word (a step barrier that timed out: its 32 blocks were not co-resident) comes back with
      // the results; raised, the request is NOT failed: the same recurrence is redone as one launch per step, bit for bit the same
      unsigned flag = 0;
      if (m->ts_persistent && m->M > 0) HIP_TRY(hipMemcpyAsync(&flag, m->ts_hx.f() + pfhip::kBlstmFlagWord, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (!flag) break;
      HIP_TRY(hipMemsetAsync(m->ts_hx.f() + pfhip::kBlstmFlagWord, 0, 4, s));
      ++m->blstm_fallbacks;
      m->have_ts = false;
    }
  }
  if (m->ML == 0) {                                  // no token at all: NaN alphas can do that too
    if (m->M > 0) {
      const pfhip_status rs = read_range_flag(m, s, true);
      if (rs) return rs;
      m->range_hit = *m->h_flag.i();
    }
    return PFHIP_OK;
  }
  if ((out->token_ids || out->logp || nk || fire) && out->max_tokens < m->maxL)
    return fail(PFHIP_ERR_CAPACITY, "max_tokens smaller than the longest token sequence");
  if (out->logp && !m->have_logp) {
    pfhip_status st = head_locked(m, s, true);
    if (st) return st;
  }
  std::vector<int32_t> ids;
  if (out->token_ids) {
    ids.resize(m->ML);
    HIP_TRY(hipMemcpyAsync(ids.data(), m->ids.p, (size_t)m->ML * 4, hipMemcpyDeviceToHost, s));
  }
  NbestStage nbs;
  if (nk) { const pfhip_status ns = nbs.start(m, s); if (ns) return ns; }
  if (m->bias) HIP_TRY(hipMemcpyAsync(m->h_bias.p, m->bias_res.p, bias_words(B, m->bias->nbest_stride, m->bias_mt) * 4, hipMemcpyDeviceToHost, s));
  const int V = m->weights->cfg.vocab;
  if (out->logp) {
    for (int b = 0; b < B; ++b)
      if (m->n_fires[b])
        HIP_TRY(hipMemcpyAsync(out->logp + (size_t)b * out->max_tokens * V, m->logp.f() + (size_t)m->tok_off[b] * V,
                               (size_t)m->n_fires[b] * V * 4, hipMemcpyDeviceToHost, s));
  }
  {
    const pfhip_status rs = read_range_flag(m, s, false);
    if (rs) return rs;
  }
  HIP_TRY(hipStreamSynchronize(s));
  m->range_hit = m->h_flag.p ? *m->h_flag.i() : 0;
  if (out->token_ids)
    for (int b = 0; b < B; ++b)
      std::memcpy(out->token_ids + (size_t)b * out->max_tokens, ids.data() + m->tok_off[b], 4 * (size_t)m->n_fires[b]);
  if (nk) nbs.scatter(m, nk, dt->nbest_ids, dt->nbest_logp, out->max_tokens);
  if (fire) scatter_fires(m, fire, out->max_tokens);
  return PFHIP_OK;
}

}  // namespace

namespace pfhip_impl {

// ---- SenseVoice: CTC head over every row of `x` (after tp.norm), collapse, ONE device-to-host copy and the forward's one sync -----
// Results on the host (h_counts): token_num [B] | ids, tok_frame, tok_logp [B][maxT] | frame ids [M] | frame log-probs [M].
// The fused head (ctc_head.hip) keeps 12 bytes per row and 128-column tile.  The unfused head — the exact re-run of the range guard,
// a caller who wants full log-prob rows, the debug switch — runs GEMM + launch_logsoftmax_argmax over chunks of kSvsChunkRows rows:
// at vocabulary 25 055 its scratch is 2 x 2048 x 25 088 x 4 B = 411 MB (logits and log-probs of one chunk), never rows x vocabulary.
SvsHost svs_host(const pfhip_model* m) {
  const int32_t* h = m->h_counts.i();
  const size_t bt = (size_t)m->B * m->maxT;
  return {h, h + m->B, h + m->B + bt, h + m->B + 3 * bt, reinterpret_cast<const float*>(h + m->B + 2 * bt),
          reinterpret_cast<const float*>(h + m->B + 3 * bt + m->M)};
}
pfhip_status svs_head_locked(pfhip_model* m, hipStream_t s) {
  const ModelWeights& w = *m->weights;
  const Config& c = w.cfg;
  const int d = c.d_model, B = m->B, M = m->M, V = c.vocab, maxT = m->maxT;
  const size_t bt = (size_t)B * maxT, n_base = (size_t)B + 3 * bt + 2 * (size_t)M;
  // pfhip_svs_forward_spans: the spans of the greedy tokens sit behind the forward's results, so they cross in the same copy.
  // Slots per utterance: no utterance keeps more tokens behind its tags than it has speech rows, and the trellis kernel takes no more
  // than its LDS rows hold (an utterance with more labels is answered as infeasible by the kernel's own check).
  const bool spans = (int)m->svs_span_want.size() == B;
  const int mt = spans ? std::min(maxT - 4, pfhip::ctc_align_max_tokens()) : 0;
  const size_t sbt = (size_t)B * mt, n_span = n_base + (mt > 0 ? 3 * sbt + B : 0);
  // pfhip_svs_forward_beam: the search's results behind those, in the same copy.  A hypothesis has no more tokens than speech rows.
  const int fb = m->svs_beam_fb, sb = m->svs_beam_sb, nb = m->svs_beam_nbest;
  const int bmt = fb ? std::max(maxT - 4, 0) : 0;
  const size_t n_beam = fb ? (size_t)B + (size_t)B * nb * (4 + (size_t)bmt) : 0, n_words = n_span + n_beam;
  m->svs_beam_mt = bmt;
  m->svs_beam_word = n_span;
  m->svs_topk_k = 0;
  if (fb) {
    HIP_TRY(m->svs_topk_ids.ensure((size_t)M * fb * 4));
    HIP_TRY(m->svs_topk_logp.ensure((size_t)M * fb * 4));
  }
  m->svs_span_mt = mt > 0 ? mt : 0;
  m->svs_span_word = n_base;
  HIP_TRY(m->counts.ensure(n_words * 4));
  HIP_TRY(m->h_counts.ensure(n_words * 4));
  int32_t* dn = m->counts.i();
  int32_t *d_ids = dn + B, *d_frames = dn + B + bt, *d_fid = dn + B + 3 * bt;
  float *d_logp = reinterpret_cast<float*>(dn + B + 2 * bt), *d_flp = reinterpret_cast<float*>(d_fid + M);
  const float* X = m->x.f();
  HIP_TRY(m->svs_lse.ensure((size_t)M * 4));                   // the rows' log-sum-exp, kept for pfhip_svs_align
  // merged callers (svs_api.cpp): per utterance the host buffer that takes its full log-prob rows, or null
  const bool per_utt = (int)m->svs_logp_rows.size() == B;
  const bool all_unfused = pfhip::launch_ctx().exact || m->debug_ctc_unfused || m->svs_logp_host;
  m->debug_ctc_unfused = 0;
  m->svs_head_chunks = 0;
  m->svs_unfused_rows = 0;
  // GEMM + log-softmax + row log-sum-exp over rows [r0, r0 + n) in chunks of kSvsChunkRows; the rows' ids, best log-probs and
  // log-sum-exp are (over)written, the full rows go to host_dst where one is given
  // (their scratch is sized ONCE, before the first launch, for the longest range this head will run: no reallocation — a
  // device-wide synchronise — between the launches of a merged batch)
  {
    int longest = 0;
    if (all_unfused && !per_utt) longest = M;
    for (int b = 0; per_utt && b < B; ++b)
      if (all_unfused || m->svs_logp_rows[b]) longest = std::max(longest, m->T[b]);
    if (longest > 0) {
      const int rows_max = std::min(kSvsChunkRows, round_up(longest, pfhip::kTileM));
      HIP_TRY(m->svs_logits.ensure((size_t)rows_max * w.vocab_pad * 4));
      HIP_TRY(m->svs_logp.ensure((size_t)rows_max * V * 4));
    }
  }
  auto unfused_rows = [&](int r0, int n, float* host_dst) -> pfhip_status {
    for (int c0 = 0; c0 < n; c0 += kSvsChunkRows) {
      const int rows = std::min(kSvsChunkRows, n - c0), q0 = r0 + c0;
      gemm(m, s, X + (size_t)q0 * d, d, w.ctc, V, d, d, m->svs_logits.f(), w.vocab_pad, nullptr, 0, nullptr, 0, rows, false);
      {
        Scope sc(m, s, K_HEAD, 0, 12.0 * rows * V);
        pfhip::launch_logsoftmax_argmax(m->svs_logits.f(), w.vocab_pad, rows, V, m->svs_logp.f(), d_fid + q0, s, m->d_range_flag);
        pfhip::launch_gather_best(m->svs_logp.f(), V, d_fid + q0, rows, d_flp + q0, s);
        pfhip::launch_row_lse(m->svs_logits.f(), w.vocab_pad, rows, V, m->svs_lse.f() + q0, s);
        if (fb && !pfhip::launch_row_topk(m->svs_logp.f(), V, rows, V, fb, m->svs_topk_ids.i() + (size_t)q0 * fb,
                                          m->svs_topk_logp.f() + (size_t)q0 * fb, s))
          return fail(PFHIP_ERR_ARG, "beam search: first_beam larger than the vocabulary");
      }
      if (host_dst) HIP_TRY(hipMemcpyAsync(host_dst + (size_t)c0 * V, m->svs_logp.p, (size_t)rows * V * 4, hipMemcpyDeviceToHost, s));
      ++m->svs_head_chunks;
      m->svs_unfused_rows += rows;
    }
    return PFHIP_OK;
  };
  if (all_unfused) ++m->svs_unfused_forwards;
  if (all_unfused && !per_utt) {
    const pfhip_status us = unfused_rows(0, M, m->svs_logp_host);
    if (us) return us;
  } else {
    if (!all_unfused && fb) {                          // the head once, in its top-k form: ids / logp / lse are the greedy head's bit for bit
      const size_t ws = pfhip::ctc_head_topk_workspace_bytes(M, V, fb);
      HIP_TRY(m->svs_ws.ensure(ws));
      Scope sc(m, s, K_GEMM, 2.0 * M * (double)V * d,
               4.0 * ((double)M * d + (double)V * d) + (12.0 + 8.0 * fb) * M * (w.vocab_pad / pfhip::kTileN));
      if (!pfhip::launch_ctc_head_topk(X, d, w.ctc.w, d, w.ctc.b, w.ctc.scale, M, V, d, fb, d_fid, d_flp, m->svs_lse.f(), m->svs_topk_ids.i(),
                                       m->svs_topk_logp.f(), m->svs_ws.p, ws, s, m->d_range_flag))
        return fail(PFHIP_ERR_UNSUPPORTED, "CTC head: d_model must be a multiple of 32 and first_beam at most the vocabulary");
    } else if (!all_unfused) {
      const size_t ws = pfhip::ctc_head_workspace_bytes(M, V);
      HIP_TRY(m->svs_ws.ensure(ws));
      Scope sc(m, s, K_GEMM, 2.0 * M * (double)V * d, 4.0 * ((double)M * d + (double)V * d) + 12.0 * M * (w.vocab_pad / pfhip::kTileN));
      if (!pfhip::launch_ctc_head(X, d, w.ctc.w, d, w.ctc.b, w.ctc.scale, M, V, d, d_fid, d_flp, m->svs_lse.f(), m->svs_ws.p, ws, s, m->d_range_flag))
        return fail(PFHIP_ERR_UNSUPPORTED, "CTC head: d_model must be a multiple of 32");
    }
    // A merged batch: the fused head has run over all rows; the unfused chunks run over the row ranges of the utterances whose
    // caller asked for log-prob rows, and only those, so that each caller gets what it would get alone.  (The exact re-run and the
    // debug switch keep sending every row through the unfused head.)
    for (int b = 0; per_utt && b < B; ++b) {
      if (m->T[b] == 0 || (!all_unfused && !m->svs_logp_rows[b])) continue;
      const pfhip_status us = unfused_rows(m->row_off[b], m->T[b], m->svs_logp_rows[b]);
      if (us) return us;
    }
  }
  {
    Scope sc(m, s, K_CIF, 0, 20.0 * M);
    if (!pfhip::launch_ctc_collapse(d_fid, d_flp, m->m_row_off, m->m_len, B, c.blank_id, maxT, d_ids, d_frames, d_logp, dn, s))
      return fail(PFHIP_ERR_ARG, "CTC collapse refused its arguments");
  }
  if (mt > 0) {
    // The greedy alignment behind the collapse, with no host round trip: the plan kernel turns the collapse's token_num into n_lab /
    // lab_off / e_off on the device (the labels are d_ids behind the four tags), then the two kernels of pfhip_svs_align on the same
    // rows.  E and the back-pointers are sized from what the host knows: n_lab[b] <= N_b, a kept token needs a frame, so
    // sum_b N_b (N_b + 1) floats, capped; an utterance that would end beyond the cap is refused by the plan kernel (n_lab -1) and comes
    // back with spans -1 and score -inf.  (No profiling Scope, as in pfhip_svs_align.)
    long long cap = 0;
    for (int b = 0; b < B; ++b) {
      const long long N = m->svs_span_want[b] && m->T[b] > 4 ? m->T[b] - 4 : 0;
      cap += N * (N + 1);
    }
    cap = std::min<long long>(cap, m->debug_span_cap > 0 ? m->debug_span_cap : (long long)PFHIP_SVS_SPAN_MAX_FLOATS);
    const size_t ws = pfhip::ctc_align_workspace_bytes((size_t)cap);
    HIP_TRY(m->al_E.ensure(std::max<size_t>((size_t)cap, 1) * 4));
    HIP_TRY(m->al_ws.ensure(std::max<size_t>(ws, 1)));
    const size_t plan_i32 = (2 * (size_t)B + 1) & ~(size_t)1;
    HIP_TRY(m->al_plan.ensure(plan_i32 * 4 + ((size_t)B + 1) * 8));
    int *d_nlab = m->al_plan.i(), *d_laboff = d_nlab + B;
    long long* d_eoff = reinterpret_cast<long long*>(d_nlab + plan_i32);
    int32_t *d_begin = dn + n_base, *d_end = d_begin + sbt;
    float *d_slogp = reinterpret_cast<float*>(d_end + sbt), *d_score = d_slogp + sbt;
    if (!pfhip::launch_ctc_greedy_plan(dn, m->m_speech_len, B, maxT, cap, d_nlab, d_laboff, d_eoff, d_eoff + B, s))
      return fail(PFHIP_ERR_ARG, "CTC greedy plan refused its arguments");
    if (!pfhip::launch_ctc_emissions(X, d, w.ctc.w, d, w.ctc.b, m->svs_lse.f(), m->m_feat_off, m->m_speech_len, d_laboff, d_nlab, d_ids, d_eoff,
                                     B, d, V, c.blank_id, m->al_E.f(), s, cap))
      return fail(PFHIP_ERR_UNSUPPORTED, "CTC emissions: d_model must be a multiple of 32");
    if (!pfhip::launch_ctc_align(m->al_E.f(), d_eoff, (size_t)cap, m->m_speech_len, d_nlab, d_ids, d_laboff, B, mt, d_begin, d_end, d_slogp,
                                 d_score, m->al_ws.p, ws, s))
      return fail(PFHIP_ERR_ARG, "CTC alignment refused its arguments");
  }
  const bool per_utt_beams = (int)m->svs_beam_utt.size() == B;
  m->beam_lm_stride = 0;                                             // "beam_lm_score" lives until the context's next forward, searching or not
  if (fb && (per_utt_beams || m->fw_lm)) {
    // The search with every utterance on its own beams and graph (pfhip_svs_forward_beam_sets, merged beam callers): fb, sb and nb
    // are the maxima — the columns' stride, the node stride and the hypothesis stride.  Descriptors, the graph table and the images
    // of the graphs the device's bank does not hold go to the front of the search's workspace in one copy from pinned staging.
    // With a token n-gram language model (pfhip_set_token_lm) the one-set form comes here too, as descriptors that all say the
    // same: the model is walked by the per-utterance kernel's own instantiation.
    std::vector<pfhip::BeamUtt> same;
    const pfhip_ctx_graph* one_graph = m->svs_beam_graph;
    if (!per_utt_beams) same.assign((size_t)B, pfhip::BeamUtt{fb, sb, nb, one_graph ? 0 : -1});
    const pfhip::BeamUtt* const utts = per_utt_beams ? m->svs_beam_utt.data() : same.data();
    const int G = per_utt_beams ? (int)m->svs_beam_graphs.size() : one_graph ? 1 : 0;
    const pfhip_ctx_graph* const* graphs = per_utt_beams ? m->svs_beam_graphs.data() : &one_graph;
    const void* const* resident = per_utt_beams && (int)m->svs_graph_dev.size() == G && G > 0 ? m->svs_graph_dev.data() : nullptr;
    // Behind them, in the same copy, the speech rows of every utterance [B] (m_speech_len holds those of the span callers only).
    const size_t lens = pfhip::beam_front_bytes(B, graphs, G, resident), front = lens + ((size_t)B * 4 + 15) / 16 * 16;
    const size_t nodes = pfhip::ctc_prefix_beam_workspace_bytes(M, B, sb);
    HIP_TRY(m->svs_beam_ws.ensure(front + nodes));
    HIP_TRY(m->svs_beam_stage.ensure(front));
    char* const dev = static_cast<char*>(m->svs_beam_ws.p);
    char* const stage = static_cast<char*>(m->svs_beam_stage.p);
    std::memset(stage, 0, front);
    pfhip::beam_front_fill(stage, dev, utts, B, graphs, G, resident);
    for (int b = 0; b < B; ++b) reinterpret_cast<int*>(stage + lens)[b] = m->T[b] > 4 ? m->T[b] - 4 : 0;
    HIP_TRY(hipMemcpyAsync(dev, stage, front, hipMemcpyHostToDevice, s));
    const size_t bn = (size_t)B * nb;
    int32_t *b_nhyp = dn + n_span, *b_ntok = b_nhyp + B, *b_ids = b_ntok + bn;
    float *b_score = reinterpret_cast<float*>(b_ids + bn * bmt), *b_ctc = b_score + bn, *b_ctx = b_ctc + bn;
    if (m->fw_lm) {
      HIP_TRY(m->beam_lm.ensure(std::max<size_t>(bn, 1) * 4));
      if (!pfhip::launch_ctc_prefix_beam_multi_lm(m->svs_topk_ids.i(), m->svs_topk_logp.f(), fb, M, m->m_feat_off, reinterpret_cast<const int*>(dev + lens),
                                                  B, V, c.blank_id, reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                                  reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), G,
                                                  m->fw_lm->dev, sb, nb, bmt, b_nhyp, b_ids, b_ntok, b_score, b_ctc, b_ctx, m->beam_lm.f(),
                                                  dev + front, nodes, s))
        return fail(PFHIP_ERR_ARG, "CTC prefix beam search with a language model refused its arguments");
      m->beam_lm_stride = nb;
      m->beam_lm_nbest.resize((size_t)B);
      for (int b = 0; b < B; ++b) m->beam_lm_nbest[(size_t)b] = utts[b].first_beam > 0 ? utts[b].nbest : 0;
    } else
    if (!pfhip::launch_ctc_prefix_beam_multi(m->svs_topk_ids.i(), m->svs_topk_logp.f(), fb, M, m->m_feat_off, reinterpret_cast<const int*>(dev + lens), B, V, c.blank_id,
                                             reinterpret_cast<const pfhip::BeamUtt*>(dev),
                                             reinterpret_cast<const pfhip::CtxGraphDev*>(dev + pfhip::beam_front_table_off(B)), G, sb, nb, bmt,
                                             b_nhyp, b_ids, b_ntok, b_score, b_ctc, b_ctx, dev + front, nodes, s))
      return fail(PFHIP_ERR_ARG, "CTC prefix beam search refused its arguments");
    m->svs_topk_k = fb;
  } else if (fb) {
    // The prefix beam search over the speech rows (the four prompt rows are no CTC rows, sensevoice-small.cpp:422): one workgroup per
    // utterance on the k best columns either head left.  The graph goes to the front of the search's workspace with this call.
    const pfhip_ctx_graph* g = m->svs_beam_graph;
    const size_t gbytes = g ? (g->packed.size() * 4 + 15) / 16 * 16 : 0;
    const size_t nodes = pfhip::ctc_prefix_beam_workspace_bytes(M, B, sb);
    HIP_TRY(m->svs_beam_ws.ensure(gbytes + nodes));
    pfhip::CtxGraphDev dev;
    if (g) {
      HIP_TRY(hipMemcpyAsync(m->svs_beam_ws.p, g->packed.data(), g->packed.size() * 4, hipMemcpyHostToDevice, s));
      const int S_ = g->n_states(), A = g->n_arcs();
      const int32_t* gw = m->svs_beam_ws.i();
      dev.n_states = S_; dev.n_arcs = A;
      dev.arc_begin = gw;
      dev.escape = reinterpret_cast<const float*>(gw + S_ + 1);
      dev.arc_label = gw + 2 * S_ + 1;
      dev.arc_next = gw + 2 * S_ + 1 + A;
      dev.arc_weight = reinterpret_cast<const float*>(gw + 2 * S_ + 1 + 2 * A);
    }
    const size_t bn = (size_t)B * nb;
    int32_t *b_nhyp = dn + n_span, *b_ntok = b_nhyp + B, *b_ids = b_ntok + bn;
    float *b_score = reinterpret_cast<float*>(b_ids + bn * bmt), *b_ctc = b_score + bn, *b_ctx = b_ctc + bn;
    if (!pfhip::launch_ctc_prefix_beam(m->svs_topk_ids.i(), m->svs_topk_logp.f(), fb, M, m->m_feat_off, m->m_speech_len, B, V, c.blank_id, fb, sb,
                                       dev, nb, bmt, b_nhyp, b_ids, b_ntok, b_score, b_ctc, b_ctx,
                                       static_cast<char*>(m->svs_beam_ws.p) + gbytes, nodes, s))
      return fail(PFHIP_ERR_ARG, "CTC prefix beam search refused its arguments");
    m->svs_topk_k = fb;
  }
  HIP_TRY(hipMemcpyAsync(m->h_counts.p, m->counts.p, n_words * 4, hipMemcpyDeviceToHost, s));
  {
    const pfhip_status rs = read_range_flag(m, s, false);
    if (rs) return rs;
  }
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  m->range_hit = m->h_flag.p ? *m->h_flag.i() : 0;
  const SvsHost h = svs_host(m);
  for (int b = 0; b < B; ++b) {
    m->token_num[b] = h.num[b];
    m->maxL = std::max(m->maxL, h.num[b]);
  }
  return PFHIP_OK;
}

pfhip_status head_locked(pfhip_model* m, hipStream_t s, bool want_logp) {
  m->beam_lm_stride = 0;                                             // "beam_lm_score" lives until the context's next forward, searching or not
  if (m->ML == 0) return PFHIP_OK;
  const int V = m->weights->cfg.vocab;
  if (want_logp) HIP_TRY(m->logp.ensure((size_t)m->ML * V * 4));
  if (m->nbest_k) {      // candidates asked for: the sibling kernel (topk.hip), which reads the row a second time for its log-sum-exp
    const int k = m->nbest_k;
    HIP_TRY(m->nb_ids.ensure((size_t)m->ML * k * 4));
    HIP_TRY(m->nb_logp.ensure((size_t)m->ML * k * 4));
    {
      Scope sc(m, s, K_HEAD, 0, 4.0 * m->ML * V * (want_logp ? 3 : 2));
      if (!pfhip::launch_logsoftmax_topk(m->logits.f(), m->weights->vocab_pad, m->ML, V, k, want_logp ? m->logp.f() : nullptr,
                                         static_cast<int32_t*>(m->ids.p), static_cast<int32_t*>(m->nb_ids.p), m->nb_logp.f(), s,
                                         m->d_range_flag))
        return fail(PFHIP_ERR_ARG, "nbest k outside 1..8 or larger than the vocabulary");
    }
    // behind the closed bracket of the top-k launch: the search has its own, so the head class counts each kernel once
    if (m->bias) { const pfhip_status bs = bias_search_locked(m, s); if (bs) return bs; }
  } else {
    Scope sc(m, s, K_HEAD, 0, 4.0 * m->ML * V * (want_logp ? 3 : 2));
    pfhip::launch_logsoftmax_argmax(m->logits.f(), m->weights->vocab_pad, m->ML, V, want_logp ? m->logp.f() : nullptr,
                                    static_cast<int32_t*>(m->ids.p), s, m->d_range_flag);
  }
  m->have_logp = want_logp;
  HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}

// The guard of the fp16 two-plane domain (kernels.h LaunchCtx): a forward whose range flag came back raised — a LayerNorm-folded
// row whose centred std is outside [2^-8, 2^11] or whose |mean| / std exceeds kLnOffsetMax, or a log-prob row that is not finite — is
// redone ONCE, inside the same context, on the exact kernels (bf16 three-plane GEMMs and attention, fp32 operands instead of plane
// images, LayerNorm kernels instead of the fold), and counted
// (pfhip_debug_poke "range_fallbacks").  The reference computes in plain fp32 (paraformer.cpp:496-541).
// dt (may be null): the caller's candidate buffers, dt->nbest_k <= m->nbest_k, and / or its fire-frame buffer; the exact re-run's head
// produces the candidates again (head_locked reads m->nbest_k) and its scan the fire frames (forward_cif reads m->want_fires), so what
// comes back belongs to the forward whose token_ids come back
pfhip_status fetch_locked(pfhip_model* m, pfhip_out* out, hipStream_t s, const pfhip_detail* dt) {
  pfhip_status st = fetch_once(m, out, s, dt);
  const bool bias = m->bias && m->ML > 0;                 // (no token row at all: the caller's buffers keep "no hypothesis")
  if (st || !m->range_hit || m->exact_rerun || m->weights->always_exact || !m->last_pcm.p || m->last_feats_only)
    return st || !bias ? st : scatter_bias(m);
  ++m->range_fallbacks;
  m->exact_rerun = true;
  const std::vector<int64_t> off = m->last_off;
  const std::vector<int> ns = m->last_n;
  st = enqueue_locked(m, m->last_pcm, off.data(), ns.data(), (int)ns.size(), s, false);      // the saved view: pointer and format
  if (!st) st = head_locked(m, s, out->logp != nullptr);
  if (!st) st = fetch_once(m, out, s, dt);
  m->exact_rerun = false;
  if (!st && m->bias && m->ML > 0) st = scatter_bias(m);
  return st;
}

// the fire frames of the last forward (on the host since forward_cif's synchronise: pfhip_model::host_fires), utterance b at row
// b * max_tokens of the caller's buffer
void scatter_fires(const pfhip_model* m, int32_t* dst, int max_tokens) {
  for (int b = 0; b < m->B; ++b)
    if (m->n_fires[b]) std::memcpy(dst + (size_t)b * max_tokens, m->host_fires() + m->row_off[b] + b, 4 * (size_t)m->n_fires[b]);
}

}  // namespace pfhip_impl
