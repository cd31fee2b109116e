// The launch sequence of the offline forward on one execution context: front end + encoder, predictor + CIF, decoder.
#include <algorithm>
#include <cmath>
#include <vector>

#include "offline.h"
#include "launch_common.h"

namespace {
using namespace pfhip_impl;

// ---- the forward ---------------------------------------------------------------------------------------
// The offline forward is enqueued in three parts, cut where its data already lives in pfhip_model: front end + encoder (up to `enc`),
// predictor + CIF + the token-count sync (n_fires, ML), decoder + vocabulary projection (`logits`).  What crosses the cuts besides
// that state are the path decisions:
struct ForwardPaths {
  bool planes = false;          // the encoder ran on plane-image operands (the decoder may only then)
};
// activation plane images: hi plane then lo plane in one workspace buffer
struct Img { unsigned char* hi; unsigned char* lo; };
Img img_of(const Buf& b, size_t plane_bytes) { return {static_cast<unsigned char*>(b.p), static_cast<unsigned char*>(b.p) + plane_bytes}; }

// d_pcm: the packed device buffer in either sample format (internal.h PcmView); sample_off counts samples of that format
pfhip_status forward_encoder(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
                             int B, hipStream_t s, bool feats_only, ForwardPaths* paths) {
  const ModelWeights& w = *m->weights;
  const Config& c = w.cfg;
  const int d = c.d_model, FD = w.feat_dim, FP = w.feat_pad;
  HIP_TRY(hipSetDevice(m->device));
  m->B = B; m->M = 0; m->ML = 0; m->maxT = 0; m->maxL = 0; m->have_logp = false; m->have_ts = false;
  m->T.assign(B, 0); m->row_off.assign(B, 0); m->n_fires.assign(B, 0); m->token_num.assign(B, 0); m->tok_off.assign(B, 0);
  std::vector<int> F(B), frame_off(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    if (n_samples[b] < 0) return fail(PFHIP_ERR_ARG, "negative sample count");
    F[b] = n_samples[b] < 400 ? 0 : 1 + (n_samples[b] - 400) / 160;        // feature-window.cc:84-87
    m->T[b] = (F[b] + c.lfr_n - 1) / c.lfr_n;                               // paraformer.cpp:425
    // SenseVoice: four prompt rows in front of the features (sensevoice-small.cpp:597-640); an utterance without frames has no rows at
    // all, as the reference returns "" before it runs the graph (:584-587)
    if (c.svs && !feats_only && m->T[b] > 0) m->T[b] += 4;
    m->row_off[b] = m->M;
    m->M += m->T[b];
    m->maxT = std::max(m->maxT, m->T[b]);
    frame_off[b + 1] = frame_off[b] + F[b];
  }
  const int M = m->M, total_frames = frame_off[B];
  if (M == 0) return PFHIP_OK;
  const int Mp = round_up(M, pfhip::kTileM);

  // ---- metadata: one pinned staging buffer, one H2D copy ---------------------------------------------
  const bool svs = c.svs && !feats_only;
  if (svs && (int)m->svs_prompt.size() != 4 * B) return fail(PFHIP_ERR_ARG, "a SenseVoice model is run through pfhip_svs_forward");
  const size_t n_ints = (size_t)2 * B /*sample_off as int64*/ + (B + 1) + 3 * (size_t)B + 2 * (size_t)M + 8 + (svs ? 6 * (size_t)B : 0);
  HIP_TRY(m->h_meta.ensure(n_ints * 4));
  HIP_TRY(m->meta.ensure(n_ints * 4));
  {
    int* hm = m->h_meta.i();
    int* dm = m->meta.i();
    size_t o = 0;
    std::memcpy(hm + o, sample_off, sizeof(int64_t) * B); m->m_sample_off = reinterpret_cast<int64_t*>(dm + o); o += 2 * (size_t)B;
    std::memcpy(hm + o, frame_off.data(), 4 * (B + 1)); m->m_frame_off = dm + o; o += B + 1;
    std::memcpy(hm + o, F.data(), 4 * B); m->m_nframes = dm + o; o += B;
    std::memcpy(hm + o, m->row_off.data(), 4 * B); m->m_row_off = dm + o; o += B;
    std::memcpy(hm + o, m->T.data(), 4 * B); m->m_len = dm + o; o += B;
    if (svs) {        // where the front end writes utterance b's features (behind its prompt rows), and the prompt ids
      for (int b = 0; b < B; ++b) hm[o + b] = m->row_off[b] + 4;
      m->m_feat_off = dm + o; o += B;
      std::memcpy(hm + o, m->svs_prompt.data(), 4 * 4 * (size_t)B); m->m_prompt = dm + o; o += 4 * (size_t)B;
      // the speech rows N_b the greedy tokens are aligned against (heads.cpp), 0 for an utterance nobody wants spans of; a beam
      // forward (pfhip_svs_forward_beam) searches the speech rows of every utterance (the sets form brings its own lengths with its
      // descriptors — heads.cpp —, since there utterances with spans and utterances with a search share a forward)
      const bool spans = (int)m->svs_span_want.size() == B, beam = m->svs_beam_fb > 0 && m->svs_beam_utt.empty();
      for (int b = 0; b < B; ++b) hm[o + b] = ((spans && m->svs_span_want[b]) || beam) && m->T[b] > 4 ? m->T[b] - 4 : 0;
      m->m_speech_len = dm + o; o += B;
    }
    if (o & 1) ++o;
    m->m_row_pos = dm + o;
    for (int b = 0; b < B; ++b) for (int t = 0; t < m->T[b]; ++t) hm[o + m->row_off[b] + t] = t;
    o += M;
    m->m_row_len = dm + o;
    for (int b = 0; b < B; ++b) for (int t = 0; t < m->T[b]; ++t) hm[o + m->row_off[b] + t] = m->T[b];
    o += M;
    // the forward's range flag (kernels.h LaunchCtx) is cleared by the same copy; a test may pre-raise it (pfhip_debug_poke)
    if (o & 1) ++o;
    hm[o] = m->debug_range_flag;
    m->debug_range_flag = 0;
    m->d_range_flag = dm + o;
    pfhip::launch_ctx().range_flag = m->d_range_flag;
    ++o;
    HIP_TRY(hipMemcpyAsync(dm, hm, o * 4, hipMemcpyHostToDevice, s));
  }
  // what a re-run on the exact kernels needs (fetch_locked)
  m->last_pcm = d_pcm;
  m->last_off.assign(sample_off, sample_off + B);
  m->last_n.assign(n_samples, n_samples + B);
  m->last_feats_only = feats_only;
  m->have_fires = false;

  // ---- workspace ---------------------------------------------------------------------------------------
  HIP_TRY(m->feats.ensure((size_t)Mp * FD * 4));
  if (!feats_only) {
    HIP_TRY(m->x0.ensure((size_t)Mp * FP * 4));
    HIP_TRY(m->x.ensure((size_t)Mp * d * 4));
    HIP_TRY(m->y.ensure((size_t)Mp * FP * 4));
    HIP_TRY(m->qkv.ensure((size_t)Mp * 3 * d * 4));
    HIP_TRY(m->mem.ensure((size_t)Mp * d * 4));
    HIP_TRY(m->ctx.ensure((size_t)Mp * d * 4));
    HIP_TRY(m->hbuf.ensure((size_t)(Mp + B + 128) * std::max(c.ffn, d) * 4));
    HIP_TRY(m->enc.ensure((size_t)Mp * d * 4));
    HIP_TRY(m->alphas.ensure((size_t)Mp * 4));
    const size_t n_counts = (size_t)2 * B + (m->want_fires ? (size_t)M + B : 0);      // + the fire frames, where asked for
    HIP_TRY(m->counts.ensure(n_counts * 4));
    HIP_TRY(m->h_counts.ensure(n_counts * 4));
  }

  // ---- a2+a3: fbank -> LFR -> CMVN -----------------------------------------------------------------------
  {
    double in_bytes = 0;
    for (int b = 0; b < B; ++b) in_bytes += (double)d_pcm.sample_bytes() * n_samples[b];
    Scope sc(m, s, K_FBANK, 0, in_bytes + 4.0 * FD * M);
    const pfhip::FbankTables tb = w.ft.fbank(w.cmvn_mean, w.cmvn_istd);
    const int* feat_off = svs ? m->m_feat_off : m->m_row_off;
    if (d_pcm.s16)
      pfhip::launch_fbank_lfr_cmvn(d_pcm.i16(), m->m_sample_off, m->m_frame_off, m->m_nframes, feat_off, B,
                                   total_frames, tb, m->feats.f(), s);
    else
      pfhip::launch_fbank_lfr_cmvn(d_pcm.f32(), m->m_sample_off, m->m_frame_off, m->m_nframes, feat_off, B,
                                   total_frames, tb, m->feats.f(), s);
    // E[lid], E[1], E[2], E[textnorm] into the four rows in front of them
    if (svs) pfhip::launch_svs_prompt_rows(w.svs_embed, FD, m->m_prompt, m->m_row_off, m->m_len, B, m->feats.f(), FD, s);
  }
  if (feats_only) { HIP_TRY(hipGetLastError()); return PFHIP_OK; }

  // ---- a4: encoder -------------------------------------------------------------------------------------------
  {
    Scope sc(m, s, K_OTHER, 0, 4.0 * M * (FD + FP));
    pfhip::launch_embed(m->feats.f(), FD, m->x0.f(), FP, m->m_row_pos, M, w.inv_ts, sqrtf((float)d), s);
  }
  const int hd = d / c.n_head;                    // 128, or 80 (the small Paraformer)
  const float att_scale = 1.0f / sqrtf((float)hd);
  double attn_pairs = 0;
  for (int b = 0; b < B; ++b) attn_pairs += (double)m->T[b] * m->T[b];
  float* x = m->x.f();
  // Large batches: the two LayerNorms of an encoder layer disappear into the GEMMs around them.  The GEMM that writes the
  // residual stream (out-projection, FFN2: N = 512 = four column tiles) leaves per-row statistics of each tile in its
  // epilogue; the GEMM that reads it (FFN1, the next layer's QKV) normalises its operand rows while staging them, with
  // gamma / beta folded into its weights (build_model).  One [M, 512] write + read and one launch per LayerNorm less.
  // (not on the exact kernels: the fold's cancellation is a property of fp32 accumulation, not of the planes — kernels.h kLnOffsetMax —
  // and the exact forward is what a batch flagged for its offset is redone on)
  const bool fuse_ln = w.enc_folded && pfhip::gemm_x6_ln_ok(M) && !pfhip::launch_ctx().exact;
  const bool mem_in_x = pfhip::attention_fsmn_is_fused(m->maxT, hd);
  if (fuse_ln) HIP_TRY(m->lnstats.ensure((size_t)Mp * 4 * 2 * 4));
  auto gemm_ln = [&](const Linear& W, const pfhip::GemmOp& op) {      // split_gemm (internal.h) with its accounting
    const int N = op.N, K = op.K;
    Scope sc(m, s, K_GEMM, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    split_gemm(s, W, op, M, d, m->lnstats.f());
  };
  // Large batches, second step: the four big GEMMs of a layer take BOTH operands as fp16 plane images staged by LDS-DMA
  // (gemm_p3.hip) — weights split once at load, activations written as planes by the kernel that produces them (the attention's
  // context, the residual stream out of the output projection and FFN2, FFN1's hidden activation).  The fp32 residual stream and
  // the QKV rows stay fp32 (residual adds, the attention's own staging).  Same arithmetic as the in-loop split of gemm_x3.hip.
  Img ctxP{nullptr, nullptr}, xP{nullptr, nullptr}, hP{nullptr, nullptr};
  // Below ~3500 rows the fp32-operand kernels stay: measured with the 64-row tile of gemm_p3.hip, 16 x 30 s = 8000 rows 16.95 ms
  // against 17.60, 8 x 30 s = 4000 rows 12.01 against 12.17, 4 x 30 s = 2000 rows 10.08 against 9.94 (PFHIP_PLANES_MIN_ROWS moves the
  // switch, PFHIP_PLANES=0 at load removes the path)
  static const int planes_min_rows = pfhip::env_int("PFHIP_PLANES_MIN_ROWS", 3500);
  const bool planes = fuse_ln && mem_in_x && w.enc_planes && M >= planes_min_rows && pfhip::gemm_f16_planes_form() &&
                      pfhip::attention_planes_ok(m->maxT, hd);
  paths->planes = planes;
  if (planes) {
    ++m->plane_forwards;
    const size_t pd = pfhip::plane_image_bytes(Mp, d), pf = pfhip::plane_image_bytes(Mp, c.ffn);
    HIP_TRY(m->ctxP.ensure(2 * pd));
    HIP_TRY(m->xP.ensure(2 * pd));
    HIP_TRY(m->hP.ensure(2 * pf));
    ctxP = img_of(m->ctxP, pd); xP = img_of(m->xP, pd); hP = img_of(m->hP, pf);
  }
  // Third step (round 4, opt-in: PFHIP_KV_PLANES=1): layers 1.. hand K and V to the attention as row-major fp16 planes written by the
  // QKV projection's epilogue (the bytes of the fp32 columns they replace) and staged without the in-loop split (attention_p3.hip); Q
  // stays fp32 in qkv.  Built for VERDICT r3 item 5, bit-identical to the fp32 hand-off, and measured: the attention launch 62-64 us
  // against 66 without the memory block but 74 against 73 with it, the whole step 26.6 ms against 26.3 — not the default.
  const bool kv_planes_on = pfhip::env_is1("PFHIP_KV_PLANES");
  const bool kv_planes = planes && kv_planes_on && c.n_head * pfhip::kHeadDim == d;
  Img kvP{nullptr, nullptr};
  if (kv_planes) {
    ++m->kvplane_forwards;
    const size_t pk = (size_t)Mp * 2 * d * 2;
    HIP_TRY(m->kvP.ensure(2 * pk));
    kvP = img_of(m->kvP, pk);
  }
  // op names C (fp32) and / or the plane images of C, N, K, bias, R1, relu, ln_colsum (the fold: statistics read from lnstats) and
  // stats_out; the operand images and the row counts are filled here
  auto gemm_pl = [&](const Img& A, const Planes& W, pfhip::PlaneGemmOp op) {
    const int N = op.N, K = op.K;
    Scope sc(m, s, K_GEMM, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    op.Ah = A.hi; op.Al = A.lo; op.rows_a = op.rows_p = Mp; op.Wh = W.hi; op.Wl = W.lo; op.rows_w = N; op.w_scale = W.scale;
    op.M = M; op.ldr1 = d; op.ln_stats = op.ln_colsum ? m->lnstats.f() : nullptr; op.ln_tiles = 4;
    pfhip::launch_gemm_p3(op, s);
  };
  // the layers' self-attention over one qkv buffer; a layer adds its memory block and, on the plane path, the images of its context
  pfhip::AttnOp self_att = qkv_attention(m->qkv.f(), d, m->ctx.f());
  self_att.q_off = self_att.kv_off = m->m_row_off; self_att.q_len = self_att.kv_len = m->m_len;
  self_att.B = B; self_att.H = c.n_head; self_att.max_q_len = m->maxT; self_att.scale = att_scale; self_att.head_dim = hd;
  // SenseVoice runs the loop on over its tp layers: after enc.after_norm the normalised rows ARE the residual stream (in `enc`; the
  // last LayerNorm, tp.norm, writes back into `x`).  Two things set a layer apart: `first` — input of the feature width and no
  // residual (enc.0 only) — and `no_stats` — no producer GEMM has left row statistics or plane images of its input, so its QKV
  // takes LayerNorm + GEMM (enc.0, and tp.0 behind the LayerNorm kernel).  From its out-projection on such a layer is on whichever
  // path the batch is on.
  const int n_layers = svs ? c.enc_layers + c.tp_layers : c.enc_layers;
  for (int i = 0; i < n_layers; ++i) {
    const EncLayer& L = w.enc[(size_t)i];
    const bool first = i == 0;
    const bool no_stats = first || i == c.enc_layers;
    if (i == c.enc_layers) {
      lnorm(m, s, x, d, m->enc.f(), d, w.enc_after, M, d, d);
      x = m->enc.f();
    }
    const float* xin = first ? m->x0.f() : x;
    const int ldin = first ? FP : d, Din = first ? FD : d, Kp = first ? FP : d;
    if (kv_planes && !no_stats) {
      // LayerNorm(x) Wqkv'^T on the plane images of x: Q as fp32 rows of qkv, K | V as row-major planes
      Scope sc(m, s, K_GEMM, 2.0 * M * (double)(3 * d) * d, 4.0 * ((double)M * d + 3.0 * d * d + (double)M * 3 * d));
      const Planes& W = L.qkv_f.img;
      pfhip::launch_gemm_p3({.Ah = xP.hi, .Al = xP.lo, .rows_a = Mp, .Wh = W.hi, .Wl = W.lo, .rows_w = 3 * d, .w_scale = W.scale, .C = m->qkv.f(),
                             .ldc = 3 * d, .Ph = kvP.hi, .Pl = kvP.lo, .rows_p = 2 * d, .row_planes_from = d, .M = M, .N = 3 * d, .K = d,
                             .bias = L.qkv_f.folded.b, .ln_stats = m->lnstats.f(), .ln_tiles = 4, .ln_colsum = L.qkv_f.colsum},
                            s);
    } else if (planes && !no_stats) {
      // LayerNorm(x) Wqkv'^T on the plane images of x that the previous layer's FFN2 left
      gemm_pl(xP, L.qkv_f.img, {.C = m->qkv.f(), .ldc = 3 * d, .N = 3 * d, .K = d, .bias = L.qkv_f.folded.b, .ln_colsum = L.qkv_f.colsum});
    } else if (fuse_ln && !no_stats) {
      gemm_ln(L.qkv_f.folded, {.A = x, .C = m->qkv.f(), .ldc = 3 * d, .N = 3 * d, .K = d, .ln_colsum = L.qkv_f.colsum});
    } else {
      lnorm(m, s, xin, ldin, m->y.f(), Kp, L.norm1, M, Din, Kp);
      gemm(m, s, m->y.f(), Kp, L.qkv, 3 * d, Kp, Din, m->qkv.f(), 3 * d, nullptr, 0, nullptr, 0, M, false);
    }
    {
      // FSMN memory of V + self-attention: one launch where the BF16 attention kernel runs (attention_x6.hip), else two
      Scope sc(m, s, K_ATTN, 4.0 * attn_pairs * d + 2.0 * 11 * M * d, 24.0 * M * d);
      // fused launch: the FSMN memory goes straight into the residual stream (x += memory; x = memory in the first layer, which
      // has no residual), so the bandwidth-bound output projection reads ONE residual
      pfhip::AttnOp att = self_att;
      att.fsmn_w = L.fsmn_w; att.mem = mem_in_x ? x : m->mem.f(); att.ldmem = d; att.mem_accumulate = mem_in_x && !first;
      if (planes) { att.planes_hi = ctxP.hi; att.planes_lo = ctxP.lo; att.plane_rows = Mp; }
      if (kv_planes && !no_stats) {      // K | V from the planes the QKV projection wrote, no fp32 context (kv_planes implies planes, mem_in_x)
        att.O = nullptr; att.ldo = 0;
        att.kv_hi = kvP.hi; att.kv_lo = kvP.lo; att.ldkv = 2 * d; att.v_col = d;
        pfhip::launch_attention_p3(att, s);
      } else {
        pfhip::launch_attention_fsmn(att, s);
      }
    }
    const bool more = i + 1 < n_layers && i + 1 != c.enc_layers;      // the next layer's QKV reads statistics / images
    if (planes) {
      // x = ctx Wo^T + b + (x + memory): fp32 for the residual stream, plane images for FFN1, row statistics for its LayerNorm
      gemm_pl(ctxP, L.out_img, {.C = x, .ldc = d, .Ph = xP.hi, .Pl = xP.lo, .N = d, .K = d, .bias = L.out.b, .R1 = x, .stats_out = m->lnstats.f()});
      gemm_pl(xP, L.ffn1_f.img, {.Ph = hP.hi, .Pl = hP.lo, .N = c.ffn, .K = d, .bias = L.ffn1_f.folded.b, .relu = true, .ln_colsum = L.ffn1_f.colsum});
      // (the last layer's output is read by the final LayerNorm only: neither images nor statistics)
      gemm_pl(hP, L.ffn2_img, {.C = x, .ldc = d, .Ph = more ? xP.hi : nullptr, .Pl = more ? xP.lo : nullptr, .N = d, .K = c.ffn, .bias = L.ffn2.b,
                               .R1 = x, .stats_out = more ? m->lnstats.f() : nullptr});
      continue;
    }
    // x = (first ? 0 : x) + ctx*Wo + b + fsmn_memory
    if (fuse_ln) {
      gemm_ln(L.out, {.A = m->ctx.f(), .C = x, .ldc = d, .N = d, .K = d, .R1 = mem_in_x ? x : m->mem.f(),
                      .R2 = mem_in_x || first ? nullptr : x, .stats_out = m->lnstats.f()});
      gemm_ln(L.ffn1_f.folded, {.A = x, .C = m->hbuf.f(), .ldc = c.ffn, .N = c.ffn, .K = d, .relu = true, .ln_colsum = L.ffn1_f.colsum});
      gemm_ln(L.ffn2, {.A = m->hbuf.f(), .C = x, .ldc = d, .N = d, .K = c.ffn, .R1 = x, .stats_out = more ? m->lnstats.f() : nullptr});
      continue;
    }
    gemm(m, s, m->ctx.f(), d, L.out, d, d, d, x, d, mem_in_x ? x : m->mem.f(), d, mem_in_x || first ? nullptr : x, d, M, false);
    lnorm(m, s, x, d, m->y.f(), d, L.norm2, M, d, d);
    gemm(m, s, m->y.f(), d, L.ffn1, c.ffn, d, d, m->hbuf.f(), c.ffn, nullptr, 0, nullptr, 0, M, true);
    gemm(m, s, m->hbuf.f(), c.ffn, L.ffn2, d, c.ffn, c.ffn, x, d, x, d, nullptr, 0, M, false);
  }
  if (svs) lnorm(m, s, x, d, m->x.f(), d, w.tp_norm, M, d, d);      // x is `enc` here: the model's output rows are in m->x
  else lnorm(m, s, x, d, m->enc.f(), d, w.enc_after, M, d, d);
  return PFHIP_OK;
}

// ---- predictor + CIF: alphas, the fired embeddings staged in `hbuf`, and the one host sync for the token counts ------------
pfhip_status forward_cif(pfhip_model* m, hipStream_t s) {
  const ModelWeights& w = *m->weights;
  const Config& c = w.cfg;
  const int d = c.d_model, B = m->B, M = m->M;
  float* col = m->qkv.f();          // [Mp, 3d] reused
  float* po = m->ctx.f();           // [Mp, d] reused
  {
    Scope sc(m, s, K_OTHER, 0, 16.0 * M * d);
    pfhip::launch_im2col3(m->enc.f(), d, col, 3 * d, m->m_row_pos, m->m_row_len, M, d, s);
  }
  gemm(m, s, col, 3 * d, w.pred.conv, d, 3 * d, 3 * d, po, d, c.pred_residual ? m->enc.f() : nullptr, d, nullptr, 0, M, true);
  {
    Scope sc(m, s, K_OTHER, 2.0 * M * d, 4.0 * M * d);
    pfhip::launch_alpha(po, d, w.pred.out_w, w.pred.out_b, c.smooth_factor, c.noise_threshold, m->alphas.f(), M, d, s);
  }
  float* stage = m->hbuf.f();       // [(M+B), d] reused
  // fire frames asked for: the sibling kernel, which also stores the step of every fire, behind the counts
  int* fire = m->want_fires ? m->counts.i() + 2 * B : nullptr;
  {
    Scope sc(m, s, K_CIF, 2.0 * M * d, 4.0 * M * d);
    pfhip::launch_cif(m->enc.f(), d, m->alphas.f(), m->m_row_off, m->m_len, B, d, c.cif_threshold, c.tail_threshold,
                      stage, m->counts.i(), m->counts.i() + B, s, fire);
  }
  m->have_fires = fire != nullptr;
  const int* h_counts = m->h_counts.i();
  HIP_TRY(hipMemcpyAsync(m->h_counts.p, m->counts.p, ((size_t)2 * B + (fire ? (size_t)M + B : 0)) * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));      // the one host sync: token counts size the decoder launch
  int ML = 0;
  for (int b = 0; b < B; ++b) {
    m->n_fires[b] = h_counts[b];
    m->token_num[b] = h_counts[B + b];
    m->tok_off[b] = ML;
    ML += m->n_fires[b];
    m->maxL = std::max(m->maxL, m->n_fires[b]);
  }
  m->ML = ML;
  if (ML == 0) HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}

// ---- decoder over the ML fired tokens + vocabulary projection ----------------------------------------------------------------
pfhip_status forward_decoder(pfhip_model* m, hipStream_t s, const ForwardPaths& paths) {
  const ModelWeights& w = *m->weights;
  const Config& c = w.cfg;
  const int d = c.d_model, B = m->B, M = m->M, ML = m->ML;
  const int Mp = round_up(M, pfhip::kTileM);
  if (c.contextual) {       // the reference logs "hw_emb is null" and returns empty results (paraformer.cpp:516-520)
    bool have = m->fw_hwkv != nullptr && (int)m->fw_hw_len.size() == B;
    for (int b = 0; have && b < B; ++b) have = m->fw_hw_len[b] > 0;
    if (!have) return fail(PFHIP_ERR_ARG, "contextual model needs hotword embeddings (pfhip_set_hotwords / hw_emb)");
  }
  const int MLp = round_up(ML, pfhip::kTileM);

  // ---- decoder-side metadata + workspace -------------------------------------------------------------
  {
    const size_t n = 4 * (size_t)B + ML;
    HIP_TRY(m->dmeta.ensure(n * 4));
    // second half of the pinned staging buffer: never overwritten while an earlier copy may be in flight
    if (m->h_meta.cap / 2 + n * 4 > m->h_meta.cap) return fail(PFHIP_ERR_CAPACITY, "internal: metadata staging too small");
    int* hm = reinterpret_cast<int*>(static_cast<char*>(m->h_meta.p) + m->h_meta.cap / 2);
    int* dm = m->dmeta.i();
    std::memcpy(hm, m->tok_off.data(), 4 * B); m->m_tok_off = dm;
    std::memcpy(hm + B, m->n_fires.data(), 4 * B); m->m_tok_len = dm + B;
    // every utterance attends to its own hotword set: first row and row count of the set's K/V rows (resolve_hotwords_locked);
    // utterances that share a set share an offset
    for (int b = 0; b < B; ++b) { hm[2 * B + b] = c.contextual ? m->fw_hw_off[b] : 0; hm[3 * B + b] = c.contextual ? m->fw_hw_len[b] : 0; }
    m->m_hw_off = dm + 2 * B; m->m_hw_len = dm + 3 * B;
    m->m_src_row = dm + 4 * B;
    for (int b = 0; b < B; ++b)
      for (int n2 = 0; n2 < m->n_fires[b]; ++n2) hm[4 * B + m->tok_off[b] + n2] = m->row_off[b] + b + n2;
    HIP_TRY(hipMemcpyAsync(dm, hm, n * 4, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(m->emb.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->xd.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->yd.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->hd.ensure((size_t)MLp * c.dec_ffn * 4));
  HIP_TRY(m->hd2.ensure((size_t)MLp * c.dec_ffn * 4));
  HIP_TRY(m->td.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->t2.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->qd.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->ctxd.ensure((size_t)MLp * d * 4));
  HIP_TRY(m->logits.ensure((size_t)MLp * w.vocab_pad * 4));
  HIP_TRY(m->ids.ensure((size_t)MLp * 4));
  if (m->nbest_k) { HIP_TRY(m->nb_ids.ensure((size_t)MLp * m->nbest_k * 4)); HIP_TRY(m->nb_logp.ensure((size_t)MLp * m->nbest_k * 4)); }
  {
    Scope sc(m, s, K_OTHER, 0, 8.0 * ML * d);
    pfhip::launch_compact(m->hbuf.f(), m->emb.f(), m->m_src_row, ML, d, s);      // the CIF's staging rows [(M+B), d]
    HIP_TRY(hipMemcpyAsync(m->xd.p, m->emb.p, (size_t)ML * d * 4, hipMemcpyDeviceToDevice, s));
  }

  float* xd = m->xd.f();
  float* kvbuf = m->qkv.f();        // [Mp, 2d] reused
  // Large batches: the K/V projections of the encoder output (16 x [M, 512] x [512, 1024]: 1000 tiles each, they fill the
  // chip) do not depend on the token side, whose launches (ML ~ 7000 rows: 220 tiles for N = 512) leave most CUs half empty.
  // They can run on a second stream into per-layer buffers; the cross-attention of layer i waits for event i.  No result
  // changes.  Measured: 40.85 -> 40.63 ms per 32 x 30 s step (-0.5 %) — the chip is clock-limited under the GEMMs, so filling the
  // idle CUs buys little — while every overlapped launch measures longer, which muddies the per-kernel roofline accounting.
  // OFF by default (PFHIP_DEC_SIDE=1 turns it on); costs 1 GB of HBM for the per-layer K/V buffers when on.
  static const bool side_on = pfhip::env_is1("PFHIP_DEC_SIDE");
  const bool side_kv = side_on && c.dec_layers > 0 && M >= 4096 && m->side_stream;
  if (side_kv) {
    HIP_TRY(m->kvside.ensure((size_t)c.dec_layers * Mp * 2 * d * 4));
    HIP_TRY(hipEventRecord(m->ev_enc_ready, s));
    HIP_TRY(hipStreamWaitEvent(m->side_stream, m->ev_enc_ready, 0));
    for (int i = 0; i < c.dec_layers; ++i) {
      gemm(m, m->side_stream, m->enc.f(), d, w.dec[(size_t)i].kv, 2 * d, d, d, m->kvside.f() + (size_t)i * Mp * 2 * d, 2 * d,
           nullptr, 0, nullptr, 0, M, false);
      HIP_TRY(hipEventRecord(m->ev_kv[(size_t)i], m->side_stream));
    }
  }
  double cross_pairs = 0;
  for (int b = 0; b < B; ++b) cross_pairs += (double)m->n_fires[b] * m->T[b];
  const int hdd = d / c.dec_n_head;               // the decoder's head width (decoder_conf.attention_heads)
  const float att_scale_d = 1.0f / sqrtf((float)hdd);
  // The decoder's FFN LayerNorms fold the same way (rows >= 4096): norm1 into FFN1 — its input is the residual stream the
  // previous layer's output projection wrote (statistics from that epilogue; the first layer's input comes from the CIF, so it
  // keeps its LayerNorm launch) — and the 2048-wide ffn_norm into FFN2 (FFN1's epilogue leaves 16 pairs per row, after its ReLU).
  const bool fuse_dec = w.dec_folded && pfhip::gemm_x6_ln_ok(ML) && !pfhip::launch_ctx().exact;
  const int ftiles = c.dec_ffn / pfhip::kTileN;
  if (fuse_dec) {
    HIP_TRY(m->lnstats.ensure((size_t)std::max(Mp, MLp) * 4 * 2 * 4));
    HIP_TRY(m->lnstats2.ensure((size_t)MLp * ftiles * 2 * 4));
  }
  // op names A, C, N, K, R1, relu, the fold (ln_stats, ln_tiles, ln_colsum) and stats_out; the rest is filled here
  auto x6ln = [&](const Linear& W, pfhip::GemmOp op) {
    const int N = op.N, K = op.K;
    Scope sc(m, s, K_GEMM, 2.0 * ML * (double)N * K, 4.0 * ((double)ML * K + (double)N * K + (double)ML * N));
    op.lda = op.ldw = K; op.W = W.w; op.bias = W.b; op.w_scale = W.scale; op.ldc = N; op.M = ML; op.ldr1 = d;
    pfhip::launch_gemm(op, pfhip::GemmKernel::SplitBySize, false, s);
  };
  bool xd_has_stats = false;          // lnstats holds the row statistics of the current xd
  // From 3500 token rows on (and only where the encoder ran on plane images: same arithmetic form) the decoder's large
  // GEMMs take plane-image operands as well (gemm_p3.hip): the K/V projection reads the images of the encoder output (one split
  // launch per forward), the cross-attention writes its context as images, the output projection leaves the token-side residual
  // stream as fp32 + images + row statistics, FFN1' (norm1 folded) reads those and leaves the hidden activation as fp32 + images +
  // the 16 statistics pairs per row that FFN2' (ffn_norm folded) merges.  The first layer's FFN (its input comes from the CIF),
  // the q projections (their input comes from the FSMN kernel), a contextual model's last layer and the vocabulary projection stay
  // on the in-loop-split kernels.
  static const int dec_planes_min_rows = pfhip::env_int("PFHIP_DEC_PLANES_MIN_ROWS", 3500);
  const bool dec_planes = paths.planes && fuse_dec && w.dec_planes && ML >= dec_planes_min_rows && pfhip::attention_planes_ok(m->maxL, hdd) &&
                          pfhip::gemm_f16_planes_form();
  Img encP{nullptr, nullptr}, xdP{nullptr, nullptr}, hdP{nullptr, nullptr}, ctxdP{nullptr, nullptr};
  bool xd_has_planes = false;
  if (dec_planes) {
    ++m->dec_plane_forwards;
    const size_t pe = pfhip::plane_image_bytes(Mp, d), pdd = pfhip::plane_image_bytes(MLp, d), pff = pfhip::plane_image_bytes(MLp, c.dec_ffn);
    HIP_TRY(m->encP.ensure(2 * pe));
    HIP_TRY(m->xdP.ensure(2 * pdd));
    HIP_TRY(m->ctxP.ensure(2 * pdd));
    HIP_TRY(m->hP.ensure(2 * pff));
    encP = img_of(m->encP, pe); xdP = img_of(m->xdP, pdd); ctxdP = img_of(m->ctxP, pdd); hdP = img_of(m->hP, pff);
    Scope sc(m, s, K_OTHER, 0, 8.0 * M * d);
    pfhip::launch_split_planes(m->enc.f(), d, M, Mp, d, 1.0f, encP.hi, encP.lo, s);
  }
  // one gemm_p3 launch over the token rows: op names the result as fp32 (C) and / or images (Ph, Pl), N, K, bias, R1, relu, the fold
  // and stats_out; the operand images (MLp rows per K-step) and the row counts are filled here
  auto dgemm_pl = [&](const Img& A, const Planes& W, pfhip::PlaneGemmOp op) {
    const int N = op.N, K = op.K;
    Scope sc(m, s, K_GEMM, 2.0 * ML * (double)N * K, 4.0 * ((double)ML * K + (double)N * K + (double)ML * N));
    op.Ah = A.hi; op.Al = A.lo; op.rows_a = op.rows_p = MLp; op.Wh = W.hi; op.Wl = W.lo; op.rows_w = N; op.w_scale = W.scale;
    op.M = ML; op.ldr1 = d;
    pfhip::launch_gemm_p3(op, s);
  };
  auto dec_ffn = [&](const DecFfn& F, const float* xin, float* out) {
    if (dec_planes && xd_has_planes && xd_has_stats) {
      // FFN1' on the images of the residual stream: hidden activation as fp32 (row statistics ride on that pass) + images
      dgemm_pl(xdP, F.ffn1_f.img, {.C = m->hd.f(), .ldc = c.dec_ffn, .Ph = hdP.hi, .Pl = hdP.lo, .N = c.dec_ffn, .K = d, .bias = F.ffn1_f.folded.b,
                                   .relu = true, .ln_stats = m->lnstats.f(), .ln_tiles = 4, .ln_colsum = F.ffn1_f.colsum,
                                   .stats_out = m->lnstats2.f()});
      dgemm_pl(hdP, F.ffn2_f.img, {.C = out, .ldc = d, .N = d, .K = c.dec_ffn, .bias = F.ffn2_f.folded.b, .ln_stats = m->lnstats2.f(),
                                   .ln_tiles = ftiles, .ln_colsum = F.ffn2_f.colsum});
      return;
    }
    if (fuse_dec) {
      if (xd_has_stats) {
        x6ln(F.ffn1_f.folded, {.A = xin, .C = m->hd.f(), .N = c.dec_ffn, .K = d, .relu = true, .ln_stats = m->lnstats.f(), .ln_tiles = 4,
                               .ln_colsum = F.ffn1_f.colsum, .stats_out = m->lnstats2.f()});
      } else {
        lnorm(m, s, xin, d, m->yd.f(), d, F.norm1, ML, d, d);
        x6ln(F.ffn1, {.A = m->yd.f(), .C = m->hd.f(), .N = c.dec_ffn, .K = d, .relu = true, .stats_out = m->lnstats2.f()});
      }
      x6ln(F.ffn2_f.folded, {.A = m->hd.f(), .C = out, .N = d, .K = c.dec_ffn, .ln_stats = m->lnstats2.f(), .ln_tiles = ftiles,
                             .ln_colsum = F.ffn2_f.colsum});
      return;
    }
    lnorm(m, s, xin, d, m->yd.f(), d, F.norm1, ML, d, d);
    gemm(m, s, m->yd.f(), d, F.ffn1, c.dec_ffn, d, d, m->hd.f(), c.dec_ffn, nullptr, 0, nullptr, 0, ML, true);
    lnorm(m, s, m->hd.f(), c.dec_ffn, m->hd2.f(), c.dec_ffn, F.ffn_norm, ML, c.dec_ffn, c.dec_ffn);
    gemm(m, s, m->hd2.f(), c.dec_ffn, F.ffn2, d, c.dec_ffn, c.dec_ffn, out, d, nullptr, 0, nullptr, 0, ML, false);
  };
  // the tokens' queries in qd against K | V [., 2d] of the given segments, context into ctxd
  auto cross_att = [&](const float* kv, const int* kv_off, const int* kv_len) {
    pfhip::AttnOp op = kv_attention(m->qd.f(), d, kv, 2 * d, m->ctxd.f());
    op.q_off = m->m_tok_off; op.q_len = m->m_tok_len; op.kv_off = kv_off; op.kv_len = kv_len;
    op.B = B; op.H = c.dec_n_head; op.max_q_len = m->maxL; op.scale = att_scale_d;
    return op;
  };
  for (int i = 0; i < c.dec_layers; ++i) {
    const DecLayer& L = w.dec[(size_t)i];
    dec_ffn(L.ffn, xd, m->td.f());
    lnorm(m, s, m->td.f(), d, m->t2.f(), d, L.norm2, ML, d, d);
    {
      Scope sc(m, s, K_FSMN, 2.0 * 11 * ML * d, 12.0 * ML * d);
      pfhip::launch_fsmn(m->t2.f(), d, L.fsmn_w, xd, d, xd, d, m->m_tok_off, m->m_tok_len, B, m->maxL, d, s);
    }
    lnorm(m, s, xd, d, m->yd.f(), d, L.norm3, ML, d, d);
    gemm(m, s, m->yd.f(), d, L.q, d, d, d, m->qd.f(), d, nullptr, 0, nullptr, 0, ML, false);
    const bool plain_layer = !(c.contextual && i == c.dec_layers - 1);
    if (side_kv) {
      kvbuf = m->kvside.f() + (size_t)i * Mp * 2 * d;
      HIP_TRY(hipStreamWaitEvent(s, m->ev_kv[(size_t)i], 0));
    } else if (dec_planes) {
      Scope sc(m, s, K_GEMM, 2.0 * M * 2.0 * d * d, 4.0 * ((double)M * d + 2.0 * d * d + 2.0 * M * d));
      const Planes& W = L.kv_img;
      pfhip::launch_gemm_p3({.Ah = encP.hi, .Al = encP.lo, .rows_a = Mp, .Wh = W.hi, .Wl = W.lo, .rows_w = 2 * d, .w_scale = W.scale, .C = kvbuf,
                             .ldc = 2 * d, .rows_p = Mp, .M = M, .N = 2 * d, .K = d, .bias = L.kv.b},
                            s);
    } else {
      gemm(m, s, m->enc.f(), d, L.kv, 2 * d, d, d, kvbuf, 2 * d, nullptr, 0, nullptr, 0, M, false);
    }
    {
      Scope sc(m, s, K_ATTN, 4.0 * cross_pairs * d, 8.0 * ML * d + 8.0 * M * d);
      pfhip::AttnOp att = cross_att(kvbuf, m->m_row_off, m->m_len);
      if (dec_planes && plain_layer) {     // the context leaves as plane images for the output projection; no fp32 context is written
        att.planes_hi = ctxdP.hi; att.planes_lo = ctxdP.lo; att.plane_rows = MLp;
        pfhip::launch_attention_x3(att, s);
      } else {
        att.head_dim = hdd;
        pfhip::launch_attention(att, s);
      }
    }
    xd_has_stats = false;
    xd_has_planes = false;
    if (dec_planes && plain_layer) {
      // xd = ctx Wo^T + b + xd: fp32 for the residual adds, images + row statistics for the next FFN1'
      dgemm_pl(ctxdP, L.out_img, {.C = xd, .ldc = d, .Ph = xdP.hi, .Pl = xdP.lo, .N = d, .K = d, .bias = L.out.b, .R1 = xd, .stats_out = m->lnstats.f()});
      xd_has_stats = true;
      xd_has_planes = true;
      continue;
    }
    if (plain_layer) {
      if (fuse_dec) {          // the output projection also leaves the statistics the next norm1 needs
        x6ln(L.out, {.A = m->ctxd.f(), .C = xd, .N = d, .K = d, .R1 = xd, .stats_out = m->lnstats.f()});
        xd_has_stats = true;
      } else {
        gemm(m, s, m->ctxd.f(), d, L.out, d, d, d, xd, d, xd, d, nullptr, 0, ML, false);
      }
      continue;
    }
    // ---- contextual last layer (UPSTREAM ContextualDecoderLayer + ContextualBiasDecoder + bias_output):
    //      x = x_self_attn + W_b [x_src_attn | cx],  cx = cross-attention of norm3_b(x_self_attn) over the hotword
    //      embeddings; xd holds x_self_attn, cat = [x_src_attn | cx] with row stride 2d.
    HIP_TRY(m->cat.ensure((size_t)MLp * 2 * d * 4));
    float* cat = m->cat.f();
    gemm(m, s, m->ctxd.f(), d, L.out, d, d, d, cat, 2 * d, nullptr, 0, nullptr, 0, ML, false);
    lnorm(m, s, xd, d, m->yd.f(), d, w.bias.norm3, ML, d, d);
    gemm(m, s, m->yd.f(), d, w.bias.q, d, d, d, m->qd.f(), d, nullptr, 0, nullptr, 0, ML, false);
    // the hotword K/V projections live in the device's hotword bank, filled once per hotword set and kept across calls
    // (resolve_hotwords_locked) — the audio-side kv workspace only holds Mp rows
    const float* hwkv = m->fw_hwkv;
    {
      double hw_pairs = 0;
      for (int b = 0; b < B; ++b) hw_pairs += (double)m->n_fires[b] * m->fw_hw_len[b];
      Scope sc(m, s, K_ATTN, 4.0 * hw_pairs * d, 8.0 * ML * d);
      pfhip::launch_attention(cross_att(hwkv, m->m_hw_off, m->m_hw_len), s);
    }
    gemm(m, s, m->ctxd.f(), d, w.bias.out, d, d, d, cat + d, 2 * d, nullptr, 0, nullptr, 0, ML, false);
    gemm(m, s, cat, 2 * d, w.bias.merge, d, 2 * d, 2 * d, xd, d, xd, d, nullptr, 0, ML, false);
  }
  dec_ffn(w.dec3, xd, m->td.f());
  lnorm(m, s, m->td.f(), d, m->yd.f(), d, w.dec_after, ML, d, d);
  gemm(m, s, m->yd.f(), d, w.dec_out, c.vocab, d, d, m->logits.f(), w.vocab_pad, nullptr, 0, nullptr, 0, ML, false);
  HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}

}  // namespace

namespace pfhip_impl {

pfhip_status enqueue_locked(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
                            int B, hipStream_t s, bool feats_only) {
  m->d_range_flag = nullptr;                          // until the metadata upload places it
  ForwardCtx fc(m);
  ForwardPaths paths;
  pfhip_status st = forward_encoder(m, d_pcm, sample_off, n_samples, B, s, feats_only, &paths);
  if (st || feats_only || m->M == 0) return st;
  if (m->weights->cfg.svs) return svs_head_locked(m, s);      // no CIF, no decoder, no second host sync
  st = forward_cif(m, s);
  if (st || m->ML == 0) return st;
  return forward_decoder(m, s, paths);
}

}  // namespace pfhip_impl
