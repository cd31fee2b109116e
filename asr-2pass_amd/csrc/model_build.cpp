// Loading a model: front-end tables, build_model, streams and events, the destructor.
#include <cmath>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "offline.h"
#include "launch_common.h"
#include "json_min.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

// ---- front-end tables, computed exactly like knf does on the host --------------------------------
void build_mel(int num_bins, float sample_freq, std::vector<int>& off, std::vector<int>& size,
               std::vector<float>& w) {
  // knf mel-computations.cc:107-196 with vtln_warp = 1, low 20 Hz, high = Nyquist (mel-computations.h:33-37)
  auto mel_scale = [](float f) { return 1127.0f * logf(1.0f + f / 700.0f); };
  const int padded = 512, num_fft_bins = padded / 2;
  const float nyquist = 0.5f * sample_freq;
  const float low_freq = 20.f, high_freq = nyquist + 0.f;
  const float fft_bin_width = sample_freq / padded;
  const float mel_low = mel_scale(low_freq), mel_high = mel_scale(high_freq);
  const float delta = (mel_high - mel_low) / (num_bins + 1);
  off.assign(num_bins, 0); size.assign(num_bins, 0); w.assign((size_t)num_bins * pfhip::kMelW, 0.f);
  for (int bin = 0; bin < num_bins; ++bin) {
    const float left = mel_low + bin * delta, center = mel_low + (bin + 1) * delta,
                right = mel_low + (bin + 2) * delta;
    int first = -1, last = -1;
    std::vector<float> tb(num_fft_bins, 0.f);
    for (int i = 0; i < num_fft_bins; ++i) {
      const float freq = fft_bin_width * i;
      const float mel = mel_scale(freq);
      if (mel > left && mel < right) {
        float weight;
        if (mel <= center) weight = (mel - left) / (center - left);
        else weight = (right - mel) / (right - center);
        tb[i] = weight;
        if (first == -1) first = i;
        last = i;
      }
    }
    off[bin] = first;
    size[bin] = last + 1 - first;
    for (int k = 0; k < size[bin] && k < pfhip::kMelW; ++k) w[(size_t)bin * pfhip::kMelW + k] = tb[first + k];
  }
}

// a tensor of the blob as the builder sees it: by name, with its host copy.  Nothing of this outlives build_model.
struct Tensor {
  const float* d = nullptr;   // device
  const float* h = nullptr;   // host
  std::vector<int> shape;
  size_t n = 0;
};

pfhip_status create_streams(pfhip_model* m) {
  HIP_TRY(hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&m->side_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_enc_ready, hipEventDisableTiming));
  m->ev_kv.resize((size_t)m->weights->cfg.dec_layers, nullptr);
  for (auto& e : m->ev_kv) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return PFHIP_OK;
}

}  // namespace

namespace pfhip_impl {

// knf tables exactly as the reference's host code computes them (feature-window.cc:33-42,
// mel-computations.cc:107-196) + the FFT twiddles of the device kernel.
pfhip_status build_frontend_tables(int n_mels, int sample_rate, FrontendTables* ft) {
  std::vector<float> win(400);
  const double a = 2.0 * M_PI / (400 - 1);
  for (int i = 0; i < 400; ++i) win[i] = (float)(0.54 - 0.46 * cos(a * (double)i));
  std::vector<double> tw(512);
  for (int k = 0; k < 256; ++k) { tw[2 * k] = cos(2.0 * M_PI * k / 512.0); tw[2 * k + 1] = -sin(2.0 * M_PI * k / 512.0); }
  std::vector<int> moff, msz; std::vector<float> mw;
  build_mel(n_mels, (float)sample_rate, moff, msz, mw);
  for (int b = 0; b < n_mels; ++b)
    if (msz[b] > pfhip::kMelW) return fail(PFHIP_ERR_UNSUPPORTED, "mel triangle wider than kMelW");
  HIP_TRY(ft->window.upload(win));
  HIP_TRY(ft->tw.upload(tw));
  HIP_TRY(ft->mel_off.upload(moff));
  HIP_TRY(ft->mel_size.upload(msz));
  HIP_TRY(ft->mel_w.upload(mw));
  return PFHIP_OK;
}

pfhip_status build_model(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                         pfhip_model** out) {
  if (!blob || !manifest_json || !out) return fail(PFHIP_ERR_ARG, "null argument");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PFHIP_ERR_ARG, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));

  pfhip::JValue man;
  try { man = pfhip::JParser(manifest_json).parse(); }
  catch (const std::exception& e) { return fail(PFHIP_ERR_FORMAT, e.what()); }
  const pfhip::JValue* jc = man.get("config");
  const pfhip::JValue* jt = man.get("tensors");
  if (!jc || !jt || jt->kind != pfhip::JValue::OBJ) return fail(PFHIP_ERR_FORMAT, "manifest needs config and tensors");

  // a return before the end gives everything back: `w` frees its allocations, `m` its streams (after it has waited for the device)
  std::shared_ptr<ModelWeights> w = std::make_shared<ModelWeights>();
  std::unique_ptr<pfhip_model> m(new pfhip_model);
  m->device = device;
  Config& c = w->cfg;
  c.d_model = (int)jc->number("d_model", c.d_model);
  c.n_head = (int)jc->number("n_head", c.n_head);
  c.dec_n_head = (int)jc->number("dec_n_head", c.n_head);       // written by the loaders only where decoder_conf differs
  c.ffn = (int)jc->number("ffn", c.ffn);
  c.enc_layers = (int)jc->number("enc_layers", c.enc_layers);
  c.dec_layers = (int)jc->number("dec_layers", c.dec_layers);
  c.dec_ffn = (int)jc->number("dec_ffn", c.dec_ffn);
  c.kernel = (int)jc->number("kernel", c.kernel);
  c.vocab = (int)jc->number("vocab", c.vocab);
  c.n_mels = (int)jc->number("n_mels", c.n_mels);
  c.lfr_m = (int)jc->number("lfr_m", c.lfr_m);
  c.lfr_n = (int)jc->number("lfr_n", c.lfr_n);
  c.sample_rate = (int)jc->number("fs", c.sample_rate);           // frontend_conf.fs (paraformer.cpp:191)
  if (c.sample_rate != 16000) return fail(PFHIP_ERR_UNSUPPORTED, "the front end is built for 16 kHz models (frontend_conf.fs)");
  c.pred_residual = (int)jc->number("pred_residual", 0);
  c.contextual = (int)jc->number("contextual", 0);
  c.timestamp = (int)jc->number("timestamp", 0);
  c.smooth_factor2 = (float)jc->number("smooth_factor2", c.smooth_factor2);
  c.noise_threshold2 = (float)jc->number("noise_threshold2", c.noise_threshold2);
  if (c.timestamp && (int)jc->number("upsample_times", 3) != 3)
    return fail(PFHIP_ERR_UNSUPPORTED, "timestamp head: upsample_times must be 3");
  c.cif_threshold = (float)jc->number("cif_threshold", c.cif_threshold);
  c.tail_threshold = (float)jc->number("tail_threshold", c.tail_threshold);
  c.smooth_factor = (float)jc->number("smooth_factor", c.smooth_factor);
  c.noise_threshold = (float)jc->number("noise_threshold", c.noise_threshold);
  if (const pfhip::JValue* kind = jc->get("kind")) {      // containers without `kind` mean what they always meant
    if (kind->str == "sensevoice") c.svs = 1;
    else if (!kind->str.empty() && kind->str != "paraformer") return fail(PFHIP_ERR_FORMAT, "unknown container kind " + kind->str);
  }
  if (c.svs) {
    c.tp_layers = (int)jc->number("tp_layers", 0);
    c.blank_id = (int)jc->number("blank_id", 0);
    if (c.dec_layers != 0 || c.contextual || c.timestamp) return fail(PFHIP_ERR_FORMAT, "a sensevoice container has no decoder, hotwords or timestamp head");
    // (without a tp layer the forward would have no place for enc.after_norm: the hand-off is the first tp layer's)
    if (c.tp_layers < 1 || c.blank_id < 0 || c.blank_id >= c.vocab) return fail(PFHIP_ERR_FORMAT, "a sensevoice container needs tp_layers >= 1 and blank_id inside the vocabulary");
    c.dec_ffn = c.ffn;
  }
  const int n_layers = c.enc_layers + c.tp_layers;
  // the weight prefix of layer i of that list
  auto layer_prefix = [&](int i) { return i < c.enc_layers ? "enc." + std::to_string(i) + "." : "tp." + std::to_string(i - c.enc_layers) + "."; };

  // what the gfx950 kernels are specialised for
  if (c.d_model <= 0 || c.n_head <= 0 || c.d_model % 64 || c.d_model % c.n_head || !pfhip::head_dim_supported(c.d_model / c.n_head))
    return fail(PFHIP_ERR_UNSUPPORTED, "attention kernel needs d_model/n_head == 128 or 80 (and d_model a multiple of 64)");
  if (c.dec_n_head <= 0 || c.d_model % c.dec_n_head || !pfhip::head_dim_supported(c.d_model / c.dec_n_head))
    return fail(PFHIP_ERR_UNSUPPORTED, "decoder attention needs d_model/dec_n_head == 128 or 80");
  if (c.d_model > 1024) return fail(PFHIP_ERR_UNSUPPORTED, "d_model > 1024");
  // the hotword decoder, the timestamp head and its BLSTM are built for head width 128 only
  if ((c.d_model / c.n_head != pfhip::kHeadDim || c.d_model / c.dec_n_head != pfhip::kHeadDim) && (c.contextual || c.timestamp))
    return fail(PFHIP_ERR_UNSUPPORTED, "contextual (hotword) and timestamp models need head width d_model/n_head == 128; this model has " +
                                           std::to_string(c.d_model / c.n_head));
  if (c.kernel != 11) return fail(PFHIP_ERR_UNSUPPORTED, "FSMN kernel size must be 11");
  if (c.n_mels != 80 || c.lfr_m != 7 || c.lfr_n != 6) return fail(PFHIP_ERR_UNSUPPORTED, "front end needs 80 mels, LFR 7/6");
  if (c.ffn % 128 || c.dec_ffn % 128 || c.ffn > 2048 || c.dec_ffn > 2048)
    return fail(PFHIP_ERR_UNSUPPORTED, "ffn width must be a multiple of 128 and <= 2048");
  if (c.enc_layers < 1 || c.dec_layers < 0) return fail(PFHIP_ERR_FORMAT, "bad layer counts");
  w->feat_dim = c.n_mels * c.lfr_m;
  w->feat_pad = round_up(w->feat_dim, pfhip::kTileK);
  w->vocab_pad = round_up(c.vocab, pfhip::kTileN);

  // ---- weights: upload the blob once; GEMM N-padding reads run into the slack at the end ----------
  const size_t slack = (size_t)pfhip::kTileN * 2048 * sizeof(float);
  HIP_TRY(w->blob.alloc(blob_bytes + slack));
  HIP_TRY(hipMemset(w->blob.p, 0, blob_bytes + slack));
  HIP_TRY(hipMemcpy(w->blob.p, blob, blob_bytes, hipMemcpyHostToDevice));
  const float* hb = static_cast<const float*>(blob);
  std::map<std::string, Tensor> t;
  for (const auto& kv : jt->obj) {
    const pfhip::JValue* sh = kv.second.get("shape");
    const pfhip::JValue* of = kv.second.get("offset");
    if (!sh || !of || sh->kind != pfhip::JValue::ARR) return fail(PFHIP_ERR_FORMAT, "tensor " + kv.first + ": shape/offset");
    Tensor tt;
    tt.n = 1;
    for (const auto& d : sh->arr) { tt.shape.push_back((int)d.num); tt.n *= (size_t)d.num; }
    const size_t off = (size_t)of->num;
    if (off % 16 || off + tt.n * 4 > blob_bytes) return fail(PFHIP_ERR_FORMAT, "tensor " + kv.first + ": out of blob");
    tt.d = w->blob.f() + off / 4;
    tt.h = hb + off / 4;
    t.emplace(kv.first, std::move(tt));
  }
  auto T = [&](const std::string& n) -> const Tensor& { return t.at(n); };
  // fp16 two-plane GEMM (gemm_x3.hip): one power-of-two scale per weight matrix (device pointer of its first element), from its
  // largest magnitude; a matrix nothing was registered for is staged with 1.0
  std::unordered_map<const void*, float> wscale;
  auto reg_scale = [&](const void* dptr, const float* host, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(host[i]));
    wscale[dptr] = pfhip::best_w_scale(mx);
  };
  auto scale_of = [&](const void* p) { auto it = wscale.find(p); return it == wscale.end() ? 1.0f : it->second; };
  for (const auto& kv : t)
    if (kv.second.shape.size() >= 2) reg_scale(kv.second.d, kv.second.h, kv.second.n);
  // required tensors / shapes
  auto need = [&](const std::string& n, std::vector<int> shape) -> bool {
    auto it = t.find(n);
    if (it == t.end()) { g_err = "missing tensor " + n; return false; }
    if (it->second.shape != shape) { g_err = "tensor " + n + " has unexpected shape"; return false; }
    return true;
  };
  const int d = c.d_model;
  bool ok = need("cmvn.mean", {w->feat_dim}) && need("cmvn.istd", {w->feat_dim});
  for (int i = 0; ok && i < n_layers; ++i) {
    const std::string p = layer_prefix(i);
    const int in = i == 0 ? w->feat_dim : d;
    ok = need(p + "norm1.g", {in}) && need(p + "norm1.b", {in}) && need(p + "qkv.w", {3 * d, in}) &&
         need(p + "qkv.b", {3 * d}) && need(p + "fsmn.w", {d, c.kernel}) && need(p + "out.w", {d, d}) &&
         need(p + "out.b", {d}) && need(p + "norm2.g", {d}) && need(p + "norm2.b", {d}) &&
         need(p + "ffn1.w", {c.ffn, d}) && need(p + "ffn1.b", {c.ffn}) && need(p + "ffn2.w", {d, c.ffn}) &&
         need(p + "ffn2.b", {d});
  }
  ok = ok && need("enc.after_norm.g", {d}) && need("enc.after_norm.b", {d});
  if (c.svs)
    ok = ok && need("svs.embed.w", {16, w->feat_dim}) && need("tp.norm.g", {d}) && need("tp.norm.b", {d}) && need("ctc.w", {c.vocab, d}) &&
         need("ctc.b", {c.vocab});
  else
    ok = ok && need("pred.conv.w", {d, d, 3}) && need("pred.conv.b", {d}) && need("pred.out.w", {1, d}) && need("pred.out.b", {1});
  auto need_ffn = [&](const std::string& p) {
    return need(p + "norm1.g", {d}) && need(p + "norm1.b", {d}) && need(p + "ffn1.w", {c.dec_ffn, d}) &&
           need(p + "ffn1.b", {c.dec_ffn}) && need(p + "ffn_norm.g", {c.dec_ffn}) &&
           need(p + "ffn_norm.b", {c.dec_ffn}) && need(p + "ffn2.w", {d, c.dec_ffn});
  };
  for (int i = 0; ok && i < c.dec_layers; ++i) {
    const std::string p = "dec." + std::to_string(i) + ".";
    ok = need_ffn(p) && need(p + "norm2.g", {d}) && need(p + "norm2.b", {d}) && need(p + "fsmn.w", {d, c.kernel}) &&
         need(p + "norm3.g", {d}) && need(p + "norm3.b", {d}) && need(p + "q.w", {d, d}) && need(p + "q.b", {d}) &&
         need(p + "kv.w", {2 * d, d}) && need(p + "kv.b", {2 * d}) && need(p + "out.w", {d, d}) && need(p + "out.b", {d});
  }
  if (!c.svs)
    ok = ok && need_ffn("dec3.") && need("dec.after_norm.g", {d}) && need("dec.after_norm.b", {d}) &&
         need("dec.out.w", {c.vocab, d}) && need("dec.out.b", {c.vocab});
  if (ok && c.contextual) {      // contextual (hotword) model: bias embedder + bias decoder
    if (c.dec_layers < 1) return fail(PFHIP_ERR_FORMAT, "contextual model needs a decoder");
    ok = need("bias.embed.w", {c.vocab, d}) && need("bias.lstm.w_ih", {4 * d, d}) && need("bias.lstm.w_hh", {4 * d, d}) &&
         need("bias.lstm.b_ih", {4 * d}) && need("bias.lstm.b_hh", {4 * d}) && need("bias.dec.norm3.g", {d}) &&
         need("bias.dec.norm3.b", {d}) && need("bias.dec.q.w", {d, d}) && need("bias.dec.q.b", {d}) &&
         need("bias.dec.kv.w", {2 * d, d}) && need("bias.dec.kv.b", {2 * d}) && need("bias.dec.out.w", {d, d}) &&
         need("bias.dec.out.b", {d}) && need("bias.out.w", {d, 2 * d});
  }
  if (ok && c.timestamp) {      // CifPredictorV3 upsampling head (SURVEY §8a row a6 producer, appendix A)
    ok = need("pred.up.w", {d, d, 3}) && need("pred.up.b", {d}) && need("pred.out2.w", {1, 2 * d}) && need("pred.out2.b", {1});
    for (const char* sfx : {"", "_r"})
      ok = ok && need(std::string("pred.blstm.w_ih") + sfx, {4 * d, d}) && need(std::string("pred.blstm.w_hh") + sfx, {4 * d, d}) &&
           need(std::string("pred.blstm.b_ih") + sfx, {4 * d}) && need(std::string("pred.blstm.b_hh") + sfx, {4 * d});
  }
  if (!ok) return PFHIP_ERR_FORMAT;

  // ---- repacks ---------------------------------------------------------------------------------------
  {
    const Tensor& w0 = T("enc.0.qkv.w");
    std::vector<float> p((size_t)3 * d * w->feat_pad, 0.f);
    for (int n = 0; n < 3 * d; ++n)
      std::memcpy(&p[(size_t)n * w->feat_pad], w0.h + (size_t)n * w->feat_dim, sizeof(float) * w->feat_dim);
    HIP_TRY(w->w0qkv.upload(p));
    reg_scale(w->w0qkv.p, p.data(), p.size());
  }
  if (!c.svs) {
    const Tensor& cw = T("pred.conv.w");
    std::vector<float> q((size_t)d * 3 * d);
    for (int n = 0; n < d; ++n)
      for (int ci = 0; ci < d; ++ci)
        for (int j = 0; j < 3; ++j) q[(size_t)n * 3 * d + (size_t)j * d + ci] = cw.h[((size_t)n * d + ci) * 3 + j];
    HIP_TRY(w->predconv.upload(q));
    reg_scale(w->predconv.p, q.data(), q.size());
  }
  {
    // The static half of the fp16-domain guard (kernels.h LaunchCtx).  Everything the two-plane kernels multiply besides the
    // residual stream is the output of a Linear on a LayerNorm-ed row (q, k, v, the FFN hidden layer, the decoder's q / k / v,
    // the logits' input) or an average of such rows (attention context, CIF embeddings), and a LayerNorm-ed row has norm
    // sqrt(K) before gamma:   |LN(x) w_n + b_n| <= sqrt(K) * ||w_n o gamma||_2 + |b_n + w_n . beta|   for ANY input.
    // A model whose bound reaches 32768 (no trained model's does: weights of norm ~1 give a few hundred) runs on the exact
    // kernels altogether; the residual stream itself is checked per forward.
    double worst = 0.0;
    auto ln_linear = [&](const std::string& wn, const std::string& bn, const std::string& ln) {
      if (!t.count(wn) || !t.count(ln + ".g")) return;
      const Tensor& wt = T(wn);
      const float* bb = !bn.empty() && t.count(bn) ? T(bn).h : nullptr;
      const float* g = T(ln + ".g").h; const float* be = T(ln + ".b").h;
      const int N = wt.shape[0], K = wt.shape[1];
      for (int n = 0; n < N; ++n) {
        double ss = 0.0, dot = bb ? bb[n] : 0.0;
        for (int k = 0; k < K; ++k) {
          const double wg = (double)wt.h[(size_t)n * K + k] * (double)g[k];
          ss += wg * wg;
          dot += (double)wt.h[(size_t)n * K + k] * (double)be[k];
        }
        worst = std::max(worst, std::sqrt((double)K) * std::sqrt(ss) + std::fabs(dot));
      }
    };
    for (int i = 0; i < n_layers; ++i) {
      const std::string ep = layer_prefix(i);
      ln_linear(ep + "qkv.w", ep + "qkv.b", ep + "norm1");
      ln_linear(ep + "ffn1.w", ep + "ffn1.b", ep + "norm2");
    }
    {
      const float* g = T("enc.after_norm.g").h; const float* be = T("enc.after_norm.b").h;
      double gm = 0.0, bm = 0.0;
      for (int k = 0; k < d; ++k) { gm = std::max(gm, (double)std::fabs(g[k])); bm = std::max(bm, (double)std::fabs(be[k])); }
      worst = std::max(worst, std::sqrt((double)d) * gm + bm);                 // |enc| (keys / values source, CIF embeddings)
    }
    for (int i = 0; i < c.dec_layers; ++i) {
      const std::string dp = "dec." + std::to_string(i) + ".";
      ln_linear(dp + "ffn1.w", dp + "ffn1.b", dp + "norm1");
      ln_linear(dp + "ffn2.w", "", dp + "ffn_norm");
      ln_linear(dp + "q.w", dp + "q.b", dp + "norm3");
      ln_linear(dp + "kv.w", dp + "kv.b", "enc.after_norm");
    }
    ln_linear("dec3.ffn1.w", "dec3.ffn1.b", "dec3.norm1");
    ln_linear("dec3.ffn2.w", "", "dec3.ffn_norm");
    ln_linear("dec.out.w", "dec.out.b", "dec.after_norm");
    ln_linear("ctc.w", "ctc.b", "tp.norm");
    if (c.contextual) ln_linear("bias.dec.q.w", "bias.dec.q.b", "bias.dec.norm3");
    w->static_bound = worst;
    w->always_exact = !(worst < 32768.0);
  }

  // ---- the typed tables: what is read straight from the blob -------------------------------------------
  auto lin = [&](const std::string& wn, const std::string& bn) {
    const float* wd = T(wn).d;
    return Linear{wd, bn.empty() ? nullptr : T(bn).d, scale_of(wd)};
  };
  auto norm = [&](const std::string& p) { return Norm{T(p + ".g").d, T(p + ".b").d}; };
  auto dec_ffn = [&](const std::string& p) {
    DecFfn f;
    f.norm1 = norm(p + "norm1"); f.ffn_norm = norm(p + "ffn_norm");
    f.ffn1 = lin(p + "ffn1.w", p + "ffn1.b"); f.ffn2 = lin(p + "ffn2.w", "");
    return f;
  };
  w->cmvn_mean = T("cmvn.mean").d; w->cmvn_istd = T("cmvn.istd").d;
  w->enc.resize((size_t)n_layers);
  for (int i = 0; i < n_layers; ++i) {
    const std::string p = layer_prefix(i);
    EncLayer& L = w->enc[(size_t)i];
    L.norm1 = norm(p + "norm1"); L.norm2 = norm(p + "norm2");
    L.qkv = lin(p + "qkv.w", p + "qkv.b"); L.out = lin(p + "out.w", p + "out.b");
    L.ffn1 = lin(p + "ffn1.w", p + "ffn1.b"); L.ffn2 = lin(p + "ffn2.w", p + "ffn2.b");
    L.fsmn_w = T(p + "fsmn.w").d;
  }
  w->enc[0].qkv.w = w->w0qkv.f(); w->enc[0].qkv.scale = scale_of(w->w0qkv.p);
  w->enc_after = norm("enc.after_norm");
  if (c.svs) {
    w->tp_norm = norm("tp.norm");
    w->svs_embed = T("svs.embed.w").d;
  } else {
    w->pred.conv = Linear{w->predconv.f(), T("pred.conv.b").d, scale_of(w->predconv.p)};
    w->pred.out_w = T("pred.out.w").d; w->pred.out_b = T("pred.out.b").d;
  }
  w->dec.resize((size_t)c.dec_layers);
  for (int i = 0; i < c.dec_layers; ++i) {
    const std::string p = "dec." + std::to_string(i) + ".";
    DecLayer& L = w->dec[(size_t)i];
    L.ffn = dec_ffn(p);
    L.norm2 = norm(p + "norm2"); L.norm3 = norm(p + "norm3");
    L.fsmn_w = T(p + "fsmn.w").d;
    L.q = lin(p + "q.w", p + "q.b"); L.kv = lin(p + "kv.w", p + "kv.b"); L.out = lin(p + "out.w", p + "out.b");
  }
  if (!c.svs) {
    w->dec3 = dec_ffn("dec3.");
    w->dec_after = norm("dec.after_norm");
  }
  if (c.contextual) {
    Contextual& b = w->bias;
    b.embed_w = T("bias.embed.w").d;
    b.lstm_ih = lin("bias.lstm.w_ih", "bias.lstm.b_ih"); b.lstm_hh = lin("bias.lstm.w_hh", "bias.lstm.b_hh");
    b.norm3 = norm("bias.dec.norm3");
    b.q = lin("bias.dec.q.w", "bias.dec.q.b"); b.kv = lin("bias.dec.kv.w", "bias.dec.kv.b"); b.out = lin("bias.dec.out.w", "bias.dec.out.b");
    b.merge = lin("bias.out.w", "");
  }

  if (d == 4 * pfhip::kTileN) {   // LN-on-load needs the residual stream to be exactly four 128-column tiles wide
    // W' = W * gamma[k], b' = b + W beta: LayerNorm's affine part folded into the GEMM that consumes it (offline path,
    // large batches: forward_encoder).  Products in double, rounded once.
    auto foldk = [&](const std::string& wn, const std::string& bn, const std::string& ln, int N, int K, float* dw, float* db, float* ds) {
      const float* wh = T(wn).h; const float* bb = bn.empty() ? nullptr : T(bn).h;
      const float* g = T(ln + ".g").h; const float* be = T(ln + ".b").h;
      for (int n = 0; n < N; ++n) {
        double acc = bb ? bb[n] : 0.0, cs = 0.0;
        for (int k = 0; k < K; ++k) {
          const float wf = (float)((double)wh[(size_t)n * K + k] * (double)g[k]);
          dw[(size_t)n * K + k] = wf;
          cs += (double)wf;                         // column sum of the weights AS STORED: what the matrix cores will multiply
          acc += (double)wh[(size_t)n * K + k] * (double)be[k];
        }
        db[n] = (float)acc;
        ds[n] = (float)cs;
      }
    };
    // entry i of a stack of folded weights [i][N][K] / [i][N]
    auto folded = [&](const DevMem& fw, const DevMem& fb, const DevMem& fs, int i, int N, int K) {
      const float* wd = fw.f() + (size_t)i * N * K;
      return FoldLin{Linear{wd, fb.f() + (size_t)i * N, scale_of(wd)}, fs.f() + (size_t)i * N, Planes{}};
    };
    // a plane image [rows][cols] of `src` (scale baked in) at `at`, hi plane then lo plane; returns the image's bytes
    auto split = [&](const Linear& src, int rows, int cols, const unsigned char* at, Planes* img) {
      const size_t half = pfhip::plane_image_bytes(rows, cols);
      unsigned char* hi = const_cast<unsigned char*>(at);
      pfhip::launch_split_planes(src.w, cols, rows, rows, cols, src.scale, hi, hi + half, nullptr);
      *img = Planes{hi, hi + half, src.scale};
      return 2 * half;
    };
    const int L = n_layers;
    {
      std::vector<float> wq((size_t)L * 3 * d * d + (size_t)pfhip::kTileN * d, 0.f), bq((size_t)L * 3 * d + pfhip::kTileN, 0.f);
      std::vector<float> wf((size_t)L * c.ffn * d + (size_t)pfhip::kTileN * d, 0.f), bf((size_t)L * c.ffn + pfhip::kTileN, 0.f);
      std::vector<float> sq(bq.size(), 0.f), sf(bf.size(), 0.f);
      for (int i = 0; i < L; ++i) {
        const std::string ep = layer_prefix(i);
        if (i > 0) foldk(ep + "qkv.w", ep + "qkv.b", ep + "norm1", 3 * d, d, &wq[(size_t)i * 3 * d * d], &bq[(size_t)i * 3 * d], &sq[(size_t)i * 3 * d]);
        foldk(ep + "ffn1.w", ep + "ffn1.b", ep + "norm2", c.ffn, d, &wf[(size_t)i * c.ffn * d], &bf[(size_t)i * c.ffn], &sf[(size_t)i * c.ffn]);
      }
      HIP_TRY(w->lnw_qkv.upload(wq)); HIP_TRY(w->lnb_qkv.upload(bq));
      HIP_TRY(w->lnw_ffn1.upload(wf)); HIP_TRY(w->lnb_ffn1.upload(bf));
      HIP_TRY(w->lns_qkv.upload(sq)); HIP_TRY(w->lns_ffn1.upload(sf));
      for (int i = 0; i < L; ++i) {
        reg_scale(w->lnw_qkv.f() + (size_t)i * 3 * d * d, &wq[(size_t)i * 3 * d * d], (size_t)3 * d * d);
        reg_scale(w->lnw_ffn1.f() + (size_t)i * c.ffn * d, &wf[(size_t)i * c.ffn * d], (size_t)c.ffn * d);
        if (i > 0) w->enc[(size_t)i].qkv_f = folded(w->lnw_qkv, w->lnb_qkv, w->lns_qkv, i, 3 * d, d);
        w->enc[(size_t)i].ffn1_f = folded(w->lnw_ffn1, w->lnb_ffn1, w->lns_ffn1, i, c.ffn, d);
      }
      w->enc_folded = true;
    }
    // The same four weights of every layer once more as fp16 plane images, pre-multiplied by their scale (gemm_p3.hip): on large
    // batches the encoder's GEMMs stage both operands by LDS-DMA — the activations arrive as plane images from the kernel that
    // produced them (forward_encoder).  Same bytes as the fp32 copies (0.6 GB for Paraformer-large); PFHIP_PLANES=0 skips them.
    static const bool planes_on = pfhip::env_on("PFHIP_PLANES");
    if (planes_on && c.ffn % pfhip::kTileN == 0) {
      const size_t per_layer = 2 * (pfhip::plane_image_bytes(3 * d, d) + pfhip::plane_image_bytes(d, d) + pfhip::plane_image_bytes(c.ffn, d) +
                                    pfhip::plane_image_bytes(d, c.ffn));
      // no room for the images (+70 % on the weight set): the fp32-operand kernels serve every batch size, nothing is lost
      if (w->wplanes.alloc(per_layer * (size_t)L) != hipSuccess) (void)hipGetLastError();
      for (int i = 0; i < L && w->wplanes.p; ++i) {
        EncLayer& E = w->enc[(size_t)i];
        const unsigned char* at = w->wplanes.as<unsigned char>() + per_layer * (size_t)i;
        if (i > 0) split(E.qkv_f.folded, 3 * d, d, at, &E.qkv_f.img);
        at += 2 * pfhip::plane_image_bytes(3 * d, d);
        at += split(E.out, d, d, at, &E.out_img);
        at += split(E.ffn1_f.folded, c.ffn, d, at, &E.ffn1_f.img);
        split(E.ffn2, d, c.ffn, at, &E.ffn2_img);
      }
      if (w->wplanes.p) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        w->enc_planes = true;
      }
    }
    if (!c.svs && c.dec_ffn % pfhip::kTileN == 0) {          // decoder FFNs: layers 0..dec_layers-1 and dec3 (the last entry)
      const int DL = c.dec_layers + 1, f = c.dec_ffn;
      std::vector<float> w1((size_t)DL * f * d + (size_t)pfhip::kTileN * d, 0.f), b1((size_t)DL * f + pfhip::kTileN, 0.f), s1(b1.size(), 0.f);
      std::vector<float> w2((size_t)DL * d * f + (size_t)pfhip::kTileN * f, 0.f), b2((size_t)DL * d + pfhip::kTileN, 0.f), s2(b2.size(), 0.f);
      std::vector<float> w3((size_t)DL * d * d + (size_t)pfhip::kTileN * d, 0.f), b3((size_t)DL * d + pfhip::kTileN, 0.f), s3(b3.size(), 0.f);
      for (int i = 0; i < DL; ++i) {
        const std::string dp = i < c.dec_layers ? "dec." + std::to_string(i) + "." : std::string("dec3.");
        foldk(dp + "ffn1.w", dp + "ffn1.b", dp + "norm1", f, d, &w1[(size_t)i * f * d], &b1[(size_t)i * f], &s1[(size_t)i * f]);
        foldk(dp + "ffn2.w", "", dp + "ffn_norm", d, f, &w2[(size_t)i * d * f], &b2[(size_t)i * d], &s2[(size_t)i * d]);
        if (i < c.dec_layers) foldk(dp + "q.w", dp + "q.b", dp + "norm3", d, d, &w3[(size_t)i * d * d], &b3[(size_t)i * d], &s3[(size_t)i * d]);
      }
      HIP_TRY(w->dlnw3.upload(w3)); HIP_TRY(w->dlnb3.upload(b3)); HIP_TRY(w->dlns3.upload(s3));
      HIP_TRY(w->dlnw1.upload(w1)); HIP_TRY(w->dlnb1.upload(b1)); HIP_TRY(w->dlns1.upload(s1));
      HIP_TRY(w->dlnw2.upload(w2)); HIP_TRY(w->dlnb2.upload(b2)); HIP_TRY(w->dlns2.upload(s2));
      for (int i = 0; i < DL; ++i) {
        reg_scale(w->dlnw1.f() + (size_t)i * f * d, &w1[(size_t)i * f * d], (size_t)f * d);
        reg_scale(w->dlnw2.f() + (size_t)i * d * f, &w2[(size_t)i * d * f], (size_t)d * f);
        reg_scale(w->dlnw3.f() + (size_t)i * d * d, &w3[(size_t)i * d * d], (size_t)d * d);
        DecFfn& F = i < c.dec_layers ? w->dec[(size_t)i].ffn : w->dec3;
        F.ffn1_f = folded(w->dlnw1, w->dlnb1, w->dlns1, i, f, d);
        F.ffn2_f = folded(w->dlnw2, w->dlnb2, w->dlns2, i, d, f);
        if (i < c.dec_layers) w->dec[(size_t)i].q_f = folded(w->dlnw3, w->dlnb3, w->dlns3, i, d, d);
      }
      w->dec_folded = true;
      // The decoder's large weights as plane images too (gemm_p3.hip; +0.2 GB for Paraformer-large): FFN1' / FFN2' with
      // their LayerNorms folded in, the K/V projection of the encoder output and the output projection of the cross-attention
      if (w->enc_planes) {
        const size_t per = 2 * (pfhip::plane_image_bytes(f, d) + pfhip::plane_image_bytes(d, f) + pfhip::plane_image_bytes(2 * d, d) +
                                pfhip::plane_image_bytes(d, d));
        if (w->dwplanes.alloc(per * (size_t)DL) != hipSuccess) (void)hipGetLastError();
        for (int i = 0; i < DL && w->dwplanes.p; ++i) {
          DecFfn& F = i < c.dec_layers ? w->dec[(size_t)i].ffn : w->dec3;
          const unsigned char* at = w->dwplanes.as<unsigned char>() + per * (size_t)i;
          at += split(F.ffn1_f.folded, f, d, at, &F.ffn1_f.img);
          at += split(F.ffn2_f.folded, d, f, at, &F.ffn2_f.img);
          if (i < c.dec_layers) {
            at += split(w->dec[(size_t)i].kv, 2 * d, d, at, &w->dec[(size_t)i].kv_img);
            split(w->dec[(size_t)i].out, d, d, at, &w->dec[(size_t)i].out_img);
          }
        }
        if (w->dwplanes.p) {
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipDeviceSynchronize());
          w->dec_planes = true;
        }
      }
    }
  }
  if (c.dec_layers > 0) {     // streaming latency path: all layers' K/V projections of a window in one launch (stream.cpp)
    std::vector<float> kw((size_t)c.dec_layers * 2 * d * d + (size_t)pfhip::kTileN * d, 0.f), kb((size_t)c.dec_layers * 2 * d + pfhip::kTileN, 0.f);
    for (int i = 0; i < c.dec_layers; ++i) {
      const std::string dp = "dec." + std::to_string(i) + ".";
      std::memcpy(&kw[(size_t)i * 2 * d * d], T(dp + "kv.w").h, sizeof(float) * 2 * d * d);
      std::memcpy(&kb[(size_t)i * 2 * d], T(dp + "kv.b").h, sizeof(float) * 2 * d);
    }
    HIP_TRY(w->kv_all_w.upload(kw));
    HIP_TRY(w->kv_all_b.upload(kb));
    reg_scale(w->kv_all_w.p, kw.data(), kw.size());
    w->kv_all = Linear{w->kv_all_w.f(), w->kv_all_b.f(), scale_of(w->kv_all_w.p)};
  }
  {
    const char* head = c.svs ? "ctc" : "dec.out";
    std::vector<float> vb((size_t)w->vocab_pad, 0.f);
    std::memcpy(vb.data(), T(std::string(head) + ".b").h, sizeof(float) * c.vocab);
    HIP_TRY(w->vocab_bias.upload(vb));
    const float* hw = T(std::string(head) + ".w").d;
    (c.svs ? w->ctc : w->dec_out) = Linear{hw, w->vocab_bias.f(), scale_of(hw)};
  }
  if (c.timestamp) {
    // ConvTranspose1d(d, d, k = stride = 3): out[3t + j][co] = b[co] + sum_ci x[t][ci] * w[ci][co][j]  ==  one GEMM with
    // the weight laid out [j*d + co][ci]; its [T, 3d] result IS the [3T, d] upsampled sequence.
    const Tensor& uw = T("pred.up.w");
    std::vector<float> w2((size_t)3 * d * d), b2((size_t)3 * d);
    for (int ci = 0; ci < d; ++ci)
      for (int co = 0; co < d; ++co)
        for (int j = 0; j < 3; ++j) w2[((size_t)j * d + co) * d + ci] = uw.h[((size_t)ci * d + co) * 3 + j];
    for (int j = 0; j < 3; ++j) std::memcpy(&b2[(size_t)j * d], T("pred.up.b").h, sizeof(float) * d);
    HIP_TRY(w->up_w.upload(w2));
    HIP_TRY(w->up_b.upload(b2));
    reg_scale(w->up_w.p, w2.data(), w2.size());
    // both directions' input projections in one GEMM (N = 8d), b_ih + b_hh folded; recurrent weights [2][4d][d]
    std::vector<float> wih((size_t)8 * d * d), bih((size_t)8 * d), whh((size_t)8 * d * d);
    int dir = 0;
    for (const char* sfx : {"", "_r"}) {
      std::memcpy(&wih[(size_t)dir * 4 * d * d], T(std::string("pred.blstm.w_ih") + sfx).h, sizeof(float) * 4 * d * d);
      std::memcpy(&whh[(size_t)dir * 4 * d * d], T(std::string("pred.blstm.w_hh") + sfx).h, sizeof(float) * 4 * d * d);
      // blstm.hip stages W_hh times 2^10 as two fp16 planes: its header states |w| < 32 (beyond, the low plane loses bits, then
      // the high plane overflows).  Refused here, where the weights are still named.
      for (size_t k = 0; k < (size_t)4 * d * d; ++k) {
        const float v = whh[(size_t)dir * 4 * d * d + k];
        if (!(std::fabs(v) < 32.0f))
          return fail(PFHIP_ERR_UNSUPPORTED, std::string("timestamp head: pred.blstm.w_hh") + sfx + " holds " + std::to_string(v) + " at element " +
                                                 std::to_string(k) + "; the recurrence kernel takes |w_hh| < 32 (finite)");
      }
      const float* bi = T(std::string("pred.blstm.b_ih") + sfx).h;
      const float* bh = T(std::string("pred.blstm.b_hh") + sfx).h;
      for (int k = 0; k < 4 * d; ++k) bih[(size_t)dir * 4 * d + k] = bi[k] + bh[k];
      ++dir;
    }
    HIP_TRY(w->wih.upload(wih));
    HIP_TRY(w->bih.upload(bih));
    HIP_TRY(w->whh.upload(whh));
    reg_scale(w->wih.p, wih.data(), wih.size());
    TimestampHead& ts = w->ts;
    ts.up = Linear{w->up_w.f(), w->up_b.f(), scale_of(w->up_w.p)};
    ts.ih = Linear{w->wih.f(), w->bih.f(), scale_of(w->wih.p)};
    ts.whh = w->whh.f();
    ts.out2_w = T("pred.out2.w").d;
    ts.out2_b = T("pred.out2.b").h[0];
  }
  // ---- front-end tables ------------------------------------------------------------------------------
  {
    pfhip_status st = pfhip_impl::build_frontend_tables(c.n_mels, c.sample_rate, &w->ft);
    if (st) return st;
    const int half = w->feat_dim / 2;
    std::vector<float> inv(half);
    // paraformer-online.cpp:247-252: float scale, exp() in double of a float argument, stored to float
    const float scale = w->feat_dim == 560 ? -0.0330119726594128f : (float)(-std::log(10000.0) / (half - 1));
    for (int i = 0; i < half; ++i) inv[i] = (float)exp((double)(i * scale));
    HIP_TRY(w->inv_ts_mem.upload(inv));
    w->inv_ts = w->inv_ts_mem.f();
  }
  m->weights = std::move(w);
  {
    pfhip_status st = create_streams(m.get());
    if (st) return st;
  }
  *out = m.release();
  return PFHIP_OK;
}

// An execution context on `owner`'s device: the reference's decoder threads share ONE session (paraformer.cpp:35-41,541); here
// they share one weight set, and what a forward needs for itself — workspace, streams, events, the state of its last batch —
// is a context.  Costs a few KB until its first forward sizes the workspace.
pfhip_status build_context(pfhip_model* owner, pfhip_model** out) {
  HIP_TRY(hipSetDevice(owner->device));
  std::unique_ptr<pfhip_model> m(new pfhip_model);
  m->device = owner->device;
  m->weights = owner->weights;
  m->weights_of = owner;
  pfhip_status st = create_streams(m.get());
  if (st) return st;
  *out = m.release();
  return PFHIP_OK;
}

pfhip_status read_file(const char* path, std::vector<char>& out) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return fail(PFHIP_ERR_ARG, std::string("cannot open ") + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  out.resize((size_t)n);
  if (n && !f.read(out.data(), n)) return fail(PFHIP_ERR_ARG, std::string("cannot read ") + path);
  return PFHIP_OK;
}

}  // namespace pfhip_impl

// Everything pfhip_destroy does: the device is set and idle before any member gives its memory back; the workspace, the pinned
// staging, the hotword bank's book-keeping and the (shared) weights are then freed by their own destructors.
pfhip_model::~pfhip_model() {
  for (pfhip_model* r : replicas) delete r;
  for (pfhip_model* cx : contexts) delete cx;
  (void)hipSetDevice(device);
  (void)hipDeviceSynchronize();
  if (hwbank) {               // the device's hotword bank (unused on a context)
    HwBankDev& D = *hwbank;
    for (size_t i = 0; i < D.bank.id_count(); ++i)
      if (D.bank.entry((int)i).ready) (void)hipEventDestroy(static_cast<hipEvent_t>(D.bank.entry((int)i).ready));
    if (D.arena) (void)hipFree(D.arena);
  }
  pfhip_impl::destroy_graph_bank(this);      // the device's bank of context graphs (SenseVoice; unused on a context)
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
  if (own_stream) (void)hipStreamDestroy(own_stream);
  if (side_stream) (void)hipStreamDestroy(side_stream);
  if (ev_enc_ready) (void)hipEventDestroy(ev_enc_ready);
  if (ev_ts_in) (void)hipEventDestroy(ev_ts_in);
  if (ev_ts_out) (void)hipEventDestroy(ev_ts_out);
  if (blstm_stream) (void)hipStreamDestroy(blstm_stream);
  for (hipEvent_t e : ev_kv) if (e) (void)hipEventDestroy(e);
}
