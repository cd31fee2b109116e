// C-ABI implementation (include/pfhip.h): model container + launch sequence of the offline
// Paraformer forward on one MI355X.  Layout in HBM:
//   * all utterances of a batch are PACKED row-major with no padding rows: utterance b owns LFR rows
//     [row_off[b], row_off[b]+T_b) of every [M, *] activation matrix (M = sum T_b); the reference's
//     GPU flavour zero-pads to Tmax instead (onnxruntime/src/paraformer-torch.cpp:342-347);
//   * decoder-side matrices are packed the same way over the CIF-fired tokens (ML = sum fires);
//   * weights stay in the blob's torch [out,in] layout = the K-contiguous B operand of the GEMM.
#include "../../include/pfhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <optional>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "internal.h"
#include "launch_common.h"
#include "json_min.h"

namespace pfhip_impl {
std::atomic<uint64_t>& buf_epoch() {
  static std::atomic<uint64_t> e{1};
  return e;
}
std::string& last_error() {
  thread_local std::string e;
  return e;
}
}  // namespace pfhip_impl

namespace {
using namespace pfhip_impl;
#define g_err (pfhip_impl::last_error())

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
}  // namespace pfhip_impl

namespace {
using namespace pfhip_impl;

pfhip_status create_streams(pfhip_model* m);

// a tensor of the blob as the builder sees it: by name, with its host copy.  Nothing of this outlives build_model.
struct Tensor {
  const float* d = nullptr;   // device
  const float* h = nullptr;   // host
  std::vector<int> shape;
  size_t n = 0;
};

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

pfhip_status create_streams(pfhip_model* m) {
  HIP_TRY(hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&m->side_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_enc_ready, hipEventDisableTiming));
  m->ev_kv.resize((size_t)m->weights->cfg.dec_layers, nullptr);
  for (auto& e : m->ev_kv) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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

}  // namespace

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
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
  if (own_stream) (void)hipStreamDestroy(own_stream);
  if (side_stream) (void)hipStreamDestroy(side_stream);
  if (ev_enc_ready) (void)hipEventDestroy(ev_enc_ready);
  if (ev_ts_in) (void)hipEventDestroy(ev_ts_in);
  if (ev_ts_out) (void)hipEventDestroy(ev_ts_out);
  if (blstm_stream) (void)hipStreamDestroy(blstm_stream);
  for (hipEvent_t e : ev_kv) if (e) (void)hipEventDestroy(e);
}

namespace {
using namespace pfhip_impl;

pfhip_status read_file(const char* path, std::vector<char>& out) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return fail(PFHIP_ERR_ARG, std::string("cannot open ") + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  out.resize((size_t)n);
  if (n && !f.read(out.data(), n)) return fail(PFHIP_ERR_ARG, std::string("cannot read ") + path);
  return PFHIP_OK;
}

// ---- the forward ---------------------------------------------------------------------------------------
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
pfhip_status forward_encoder(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples, int B, hipStream_t s,
                             bool feats_only, ForwardPaths* paths);
pfhip_status forward_cif(pfhip_model* m, hipStream_t s);
pfhip_status forward_decoder(pfhip_model* m, hipStream_t s, const ForwardPaths& paths);
pfhip_status svs_head_locked(pfhip_model* m, hipStream_t s);
pfhip_status read_range_flag(pfhip_model* m, hipStream_t s, bool sync);

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
  const size_t n_ints = (size_t)2 * B /*sample_off as int64*/ + (B + 1) + 3 * (size_t)B + 2 * (size_t)M + 8 + (svs ? 5 * (size_t)B : 0);
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

// ---- SenseVoice: CTC head over every row of `x` (after tp.norm), collapse, ONE device-to-host copy and the forward's one sync -----
// Results on the host (h_counts): token_num [B] | ids, tok_frame, tok_logp [B][maxT] | frame ids [M] | frame log-probs [M].
// The fused head (ctc_head.hip) keeps 12 bytes per row and 128-column tile.  The unfused head — the exact re-run of the range guard,
// a caller who wants full log-prob rows, the debug switch — runs GEMM + launch_logsoftmax_argmax over chunks of kSvsChunkRows rows:
// at vocabulary 25 055 its scratch is 2 x 2048 x 25 088 x 4 B = 411 MB (logits and log-probs of one chunk), never rows x vocabulary.
constexpr int kSvsChunkRows = 2048;
struct SvsHost { const int32_t *num, *ids, *frames, *fid; const float *logp, *flp; };
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
  const size_t bt = (size_t)B * maxT, n_words = (size_t)B + 3 * bt + 2 * (size_t)M;
  HIP_TRY(m->counts.ensure(n_words * 4));
  HIP_TRY(m->h_counts.ensure(n_words * 4));
  int32_t* dn = m->counts.i();
  int32_t *d_ids = dn + B, *d_frames = dn + B + bt, *d_fid = dn + B + 3 * bt;
  float *d_logp = reinterpret_cast<float*>(dn + B + 2 * bt), *d_flp = reinterpret_cast<float*>(d_fid + M);
  const float* X = m->x.f();
  HIP_TRY(m->svs_lse.ensure((size_t)M * 4));                   // the rows' log-sum-exp, kept for pfhip_svs_align
  const bool unfused = pfhip::launch_ctx().exact || m->debug_ctc_unfused || m->svs_logp_host;
  m->debug_ctc_unfused = 0;
  m->svs_head_chunks = 0;
  if (unfused) {
    ++m->svs_unfused_forwards;
    const int rows_max = std::min(kSvsChunkRows, round_up(M, pfhip::kTileM));
    HIP_TRY(m->svs_logits.ensure((size_t)rows_max * w.vocab_pad * 4));
    HIP_TRY(m->svs_logp.ensure((size_t)rows_max * V * 4));
    for (int r0 = 0; r0 < M; r0 += kSvsChunkRows) {
      const int rows = std::min(kSvsChunkRows, M - r0);
      gemm(m, s, X + (size_t)r0 * d, d, w.ctc, V, d, d, m->svs_logits.f(), w.vocab_pad, nullptr, 0, nullptr, 0, rows, false);
      {
        Scope sc(m, s, K_HEAD, 0, 12.0 * rows * V);
        pfhip::launch_logsoftmax_argmax(m->svs_logits.f(), w.vocab_pad, rows, V, m->svs_logp.f(), d_fid + r0, s, m->d_range_flag);
        pfhip::launch_gather_best(m->svs_logp.f(), V, d_fid + r0, rows, d_flp + r0, s);
        pfhip::launch_row_lse(m->svs_logits.f(), w.vocab_pad, rows, V, m->svs_lse.f() + r0, s);
      }
      if (m->svs_logp_host)
        HIP_TRY(hipMemcpyAsync(m->svs_logp_host + (size_t)r0 * V, m->svs_logp.p, (size_t)rows * V * 4, hipMemcpyDeviceToHost, s));
      ++m->svs_head_chunks;
    }
  } else {
    const size_t ws = pfhip::ctc_head_workspace_bytes(M, V);
    HIP_TRY(m->svs_ws.ensure(ws));
    Scope sc(m, s, K_GEMM, 2.0 * M * (double)V * d, 4.0 * ((double)M * d + (double)V * d) + 12.0 * M * (w.vocab_pad / pfhip::kTileN));
    if (!pfhip::launch_ctc_head(X, d, w.ctc.w, d, w.ctc.b, w.ctc.scale, M, V, d, d_fid, d_flp, m->svs_lse.f(), m->svs_ws.p, ws, s, m->d_range_flag))
      return fail(PFHIP_ERR_UNSUPPORTED, "CTC head: d_model must be a multiple of 32");
  }
  {
    Scope sc(m, s, K_CIF, 0, 20.0 * M);
    if (!pfhip::launch_ctc_collapse(d_fid, d_flp, m->m_row_off, m->m_len, B, c.blank_id, maxT, d_ids, d_frames, d_logp, dn, s))
      return fail(PFHIP_ERR_ARG, "CTC collapse refused its arguments");
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

pfhip_status head_locked(pfhip_model* m, hipStream_t s, bool want_logp) {
  if (m->ML == 0) return PFHIP_OK;
  const int V = m->weights->cfg.vocab;
  if (want_logp) HIP_TRY(m->logp.ensure((size_t)m->ML * V * 4));
  if (m->nbest_k) {      // candidates asked for: the sibling kernel (topk.hip), which reads the row a second time for its log-sum-exp
    const int k = m->nbest_k;
    HIP_TRY(m->nb_ids.ensure((size_t)m->ML * k * 4));
    HIP_TRY(m->nb_logp.ensure((size_t)m->ML * k * 4));
    Scope sc(m, s, K_HEAD, 0, 4.0 * m->ML * V * (want_logp ? 3 : 2));
    if (!pfhip::launch_logsoftmax_topk(m->logits.f(), m->weights->vocab_pad, m->ML, V, k, want_logp ? m->logp.f() : nullptr,
                                       static_cast<int32_t*>(m->ids.p), static_cast<int32_t*>(m->nb_ids.p), m->nb_logp.f(), s,
                                       m->d_range_flag))
      return fail(PFHIP_ERR_ARG, "nbest k outside 1..8 or larger than the vocabulary");
  } else {
    Scope sc(m, s, K_HEAD, 0, 4.0 * m->ML * V * (want_logp ? 3 : 2));
    pfhip::launch_logsoftmax_argmax(m->logits.f(), m->weights->vocab_pad, m->ML, V, want_logp ? m->logp.f() : nullptr,
                                    static_cast<int32_t*>(m->ids.p), s, m->d_range_flag);
  }
  m->have_logp = want_logp;
  HIP_TRY(hipGetLastError());
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

pfhip_status fetch_once(pfhip_model* m, pfhip_out* out, hipStream_t s, const pfhip_detail* dt);
// The guard of the fp16 two-plane domain (kernels.h LaunchCtx): a forward whose range flag came back raised — a LayerNorm-folded
// row whose centred std is outside [2^-8, 2^11] or whose |mean| / std exceeds kLnOffsetMax, or a log-prob row that is not finite — is
// redone ONCE, inside the same context, on the exact kernels (bf16 three-plane GEMMs and attention, fp32 operands instead of plane
// images, LayerNorm kernels instead of the fold), and counted
// (pfhip_debug_poke "range_fallbacks").  The reference computes in plain fp32 (paraformer.cpp:496-541).
// dt (may be null): the caller's candidate buffers, dt->nbest_k <= m->nbest_k, and / or its fire-frame buffer; the exact re-run's head
// produces the candidates again (head_locked reads m->nbest_k) and its scan the fire frames (forward_cif reads m->want_fires), so what
// comes back belongs to the forward whose token_ids come back
pfhip_status fetch_locked(pfhip_model* m, pfhip_out* out, hipStream_t s, const pfhip_detail* dt = nullptr) {
  pfhip_status st = fetch_once(m, out, s, dt);
  if (st || !m->range_hit || m->exact_rerun || m->weights->always_exact || !m->last_pcm.p || m->last_feats_only) return st;
  ++m->range_fallbacks;
  m->exact_rerun = true;
  const std::vector<int64_t> off = m->last_off;
  const std::vector<int> ns = m->last_n;
  st = enqueue_locked(m, m->last_pcm, off.data(), ns.data(), (int)ns.size(), s, false);      // the saved view: pointer and format
  if (!st) st = head_locked(m, s, out->logp != nullptr);
  if (!st) st = fetch_once(m, out, s, dt);
  m->exact_rerun = false;
  return st;
}

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
// the fire frames of the last forward (on the host since forward_cif's synchronise: pfhip_model::host_fires), utterance b at row
// b * max_tokens of the caller's buffer
void scatter_fires(const pfhip_model* m, int32_t* dst, int max_tokens) {
  for (int b = 0; b < m->B; ++b)
    if (m->n_fires[b]) std::memcpy(dst + (size_t)b * max_tokens, m->host_fires() + m->row_off[b] + b, 4 * (size_t)m->n_fires[b]);
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

// ---- hotword bank (internal.h HwBankDev, hotword_bank.h) ----------------------------------------------------------------
pfhip_model* bank_owner(pfhip_model* m) { return m->weights_of ? m->weights_of : m; }

// sizes the arena at first use; the bank mutex is held
void ensure_bank_locked(pfhip_model* owner) {
  HwBankDev& D = *owner->hwbank;
  if (D.configured) return;
  if (D.bound_bytes < 0) {
    const char* e = getenv("PFHIP_HOTWORD_BANK_MB");
    const long mb = e && *e ? atol(e) : 64;
    D.bound_bytes = (int64_t)std::max(0L, mb) << 20;
  }
  // Slabs are whole GEMM row tiles: the projection of an H-row set may write round_up(H, kTileM) rows (gemm pads M to the tile),
  // all of them inside the set's own slab; the attention kernels clamp their key rows to the segment they are given
  const int d = owner->weights->cfg.d_model;
  const int64_t gran_bytes = (int64_t)pfhip::kTileM * 2 * d * 4;
  int granules = (int)std::min<int64_t>(D.bound_bytes / gran_bytes, INT32_MAX / pfhip::kTileM);
  if (granules > 0 && hipMalloc((void**)&D.arena, (size_t)granules * gran_bytes) != hipSuccess) {
    (void)hipGetLastError();          // no room for the arena: every set is served from the per-call buffers
    D.arena = nullptr;
    granules = 0;
  }
  D.bank.configure(pfhip::kTileM, d, granules);
  D.default_id = -1;
  D.configured = true;
}

// K/V projection of the bias decoder's cross-attention for one hotword set: [H, d] host rows -> staging rows of `m->hw` ->
// dst [round_up(H, 128), 2d].  Enqueued on `s`, nothing waits.
pfhip_status project_hotwords(pfhip_model* m, const float* host, int H, int stage_row, float* dst, hipStream_t s) {
  const int d = m->weights->cfg.d_model;
  float* A = m->hw.f() + (size_t)stage_row * d;
  HIP_TRY(hipMemcpyAsync(A, host, (size_t)H * d * 4, hipMemcpyHostToDevice, s));
  gemm(m, s, A, d, m->weights->bias.kv, 2 * d, d, d, dst, 2 * d, nullptr, 0, nullptr, 0, H, false);
  return PFHIP_OK;
}

// a bank miss: the entry's rows go up and are projected straight into its slab; the event tells other streams when.  Bank mutex held.
pfhip_status fill_slab_locked(pfhip_model* m, HwBankDev& D, int id, int stage_row, hipStream_t s) {
  HotwordBank::Entry& e = D.bank.entry(id);
  pfhip_status st = project_hotwords(m, e.host.data(), e.H, stage_row, D.arena + (size_t)D.bank.row_off(id) * 2 * m->weights->cfg.d_model, s);
  if (st) return st;
  if (!e.ready) {
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e.ready = ev;
  }
  HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(e.ready), s));
  e.ready_on = s;
  return PFHIP_OK;
}

void release_hotwords(pfhip_model* m) {
  if (m->fw_pins.empty()) return;
  HwBankDev& D = *bank_owner(m)->hwbank;
  std::lock_guard<std::mutex> l(D.mu);
  for (int id : m->fw_pins) D.bank.release(id);
  m->fw_pins.clear();
}
struct HotwordPins {          // a forward's pins end with it, whichever way it ends (after its last synchronise)
  pfhip_model* m;
  ~HotwordPins() { release_hotwords(m); }
};

// Before a contextual forward: every utterance gets the first row and the row count of ITS hotword set (set_of_utt, nullptr = all
// set 0).  Sets the device's bank holds are found by content and cost nothing; missing ones are uploaded and projected into
// their slabs on `s` — all of a call's misses through one staging buffer, no synchronise.  The entries stay pinned until
// release_hotwords.  A call with a set the bank cannot take (larger than its bound, or no room beside pinned slabs) projects
// its sets into this context's own buffers, as every call did before the bank.
pfhip_status resolve_hotwords_locked(pfhip_model* m, const float* const* emb, const int* H, int n_sets, const int* set_of_utt, int B,
                                     hipStream_t s) {
  m->fw_hw_off.assign((size_t)B, 0);
  m->fw_hw_len.assign((size_t)B, 0);
  m->fw_hwkv = nullptr;
  if (!m->weights->cfg.contextual) return PFHIP_OK;          // plain models ignore hw_emb (paraformer.cpp:515: use_hotword == false)
  if (n_sets <= 0 || !emb || !H) return fail(PFHIP_ERR_ARG, "hw_emb is null");          // paraformer.cpp:516-520
  std::vector<char> used((size_t)n_sets, 0);
  for (int b = 0; b < B; ++b) {
    const int k = set_of_utt ? set_of_utt[b] : 0;
    if (k < 0 || k >= n_sets) return fail(PFHIP_ERR_ARG, "set_of_utt names no hotword set");
    used[(size_t)k] = 1;
  }
  for (int k = 0; k < n_sets; ++k)
    if (used[(size_t)k] && (!emb[k] || H[k] <= 0)) return fail(PFHIP_ERR_ARG, "hw_emb is null");
  const int d = m->weights->cfg.d_model;
  HwBankDev& D = *bank_owner(m)->hwbank;
  std::vector<int> row((size_t)n_sets, 0);
  bool per_call = false;
  {
    std::lock_guard<std::mutex> l(D.mu);
    ensure_bank_locked(bank_owner(m));
    std::vector<int> ids((size_t)n_sets, -1), stage((size_t)n_sets, -1);
    int stage_rows = 0;
    for (int k = 0; k < n_sets && !per_call; ++k) {
      if (!used[(size_t)k]) continue;
      bool hit = false;
      ids[(size_t)k] = D.bank.acquire(emb[k], H[k], &hit);
      if (ids[(size_t)k] < 0) { per_call = true; break; }
      m->fw_pins.push_back(ids[(size_t)k]);
      if (!hit) { stage[(size_t)k] = stage_rows; stage_rows += round_up(H[k], pfhip::kTileM); }
    }
    if (per_call) {
      // the hits are let go; a set that was just entered keeps its pin and has its slab filled below, for whoever finds it later
      m->fw_pins.clear();
      for (size_t k = 0; k < ids.size(); ++k) {
        if (ids[k] < 0) continue;
        if (stage[k] >= 0) m->fw_pins.push_back(ids[k]);
        else D.bank.release(ids[k]);
      }
    }
    // an upload that fails leaves no entry behind that claims rows it does not hold
    auto give_up = [&](int from_k, pfhip_status st) {
      for (int k = from_k; k < n_sets; ++k)
        if (stage[(size_t)k] >= 0) {
          m->fw_pins.erase(std::find(m->fw_pins.begin(), m->fw_pins.end(), ids[(size_t)k]));
          D.bank.discard(ids[(size_t)k]);
        }
      return st;
    };
    if (stage_rows && m->hw.ensure((size_t)stage_rows * d * 4) != hipSuccess)
      return give_up(0, fail(PFHIP_ERR_HIP, "hipMalloc of the hotword staging buffer failed"));
    std::vector<int> distinct;
    for (int k = 0; k < n_sets; ++k) {
      if (ids[(size_t)k] < 0) continue;
      const int id = ids[(size_t)k];
      HotwordBank::Entry& e = D.bank.entry(id);
      if (stage[(size_t)k] >= 0) {
        const pfhip_status st = fill_slab_locked(m, D, id, stage[(size_t)k], s);
        if (st) return give_up(k, st);
      } else if (!per_call && !e.settled && e.ready && e.ready_on != s) {
        HIP_TRY(hipStreamWaitEvent(s, static_cast<hipEvent_t>(e.ready), 0));      // filled on another context's stream
      }
      row[(size_t)k] = D.bank.row_off(id);
      if (std::find(distinct.begin(), distinct.end(), id) == distinct.end()) distinct.push_back(id);
    }
    if (!per_call) {
      ++D.forwards;
      D.sets_total += (int64_t)distinct.size();
      D.sets_max = std::max<int64_t>(D.sets_max, (int64_t)distinct.size());
      m->fw_hwkv = D.arena;
    }
  }
  if (per_call) {
    int rows = 0, n_used = 0;
    for (int k = 0; k < n_sets; ++k)
      if (used[(size_t)k]) { row[(size_t)k] = rows; rows += round_up(H[k], pfhip::kTileM); ++n_used; }
    HIP_TRY(m->hw.ensure((size_t)rows * d * 4));
    HIP_TRY(m->hwkv.ensure((size_t)rows * 2 * d * 4));
    for (int k = 0; k < n_sets; ++k) {
      if (!used[(size_t)k]) continue;
      const pfhip_status st = project_hotwords(m, emb[k], H[k], row[(size_t)k], m->hwkv.f() + (size_t)row[(size_t)k] * 2 * d, s);
      if (st) return st;
    }
    m->fw_hwkv = m->hwkv.f();
    std::lock_guard<std::mutex> l(D.mu);
    ++D.forwards; ++D.percall_forwards;
    D.sets_total += n_used;
    D.sets_max = std::max<int64_t>(D.sets_max, n_used);
  }
  for (int b = 0; b < B; ++b) {
    const int k = set_of_utt ? set_of_utt[b] : 0;
    m->fw_hw_off[(size_t)b] = row[(size_t)k];
    m->fw_hw_len[(size_t)b] = H[k];
  }
  HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}

// the default set (pfhip_set_hotwords) for calls that bring none
std::shared_ptr<const std::vector<float>> default_hotwords(pfhip_model* m) {
  pfhip_model* head = m->group_head ? m->group_head : m;
  std::lock_guard<std::mutex> l(head->bq.mu);
  return head->hw_default;
}
pfhip_status resolve_default_hotwords_locked(pfhip_model* m, int B, hipStream_t s) {
  if (!m->weights->cfg.contextual) return resolve_hotwords_locked(m, nullptr, nullptr, 0, nullptr, B, s);
  const std::shared_ptr<const std::vector<float>> hw = default_hotwords(m);
  if (!hw || hw->empty()) return fail(PFHIP_ERR_ARG, "hw_emb is null");
  const float* e = hw->data();
  const int H = (int)(hw->size() / (size_t)m->weights->cfg.d_model);
  return resolve_hotwords_locked(m, &e, &H, 1, nullptr, B, s);
}

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

}  // namespace

// =================================================================================================
extern "C" {

const char* pfhip_last_error(void) { return g_err.c_str(); }

static pfhip_status apply_env_inflight(pfhip_model** out);

pfhip_status pfhip_create_group(const void* blob, size_t blob_bytes, const char* manifest_json, const int* devices, int n_devices,
                                pfhip_model** out) {
  g_err.clear();
  if (!devices || n_devices < 1 || !out) return fail(PFHIP_ERR_ARG, "bad device list");
  pfhip_model* head = nullptr;
  try {
    pfhip_status st = build_model(blob, blob_bytes, manifest_json, devices[0], &head);
    if (st) return st;
    for (int i = 1; i < n_devices; ++i) {
      pfhip_model* r = nullptr;
      st = build_model(blob, blob_bytes, manifest_json, devices[i], &r);
      if (st) { const std::string why = g_err; pfhip_destroy(head); g_err = why; return st; }
      r->group_head = head;
      head->replicas.push_back(r);
    }
  } catch (const std::exception& e) {
    if (head) pfhip_destroy(head);
    return fail(PFHIP_ERR_FORMAT, e.what());
  }
  *out = head;
  return apply_env_inflight(out);
}

// PFHIP_DEVICES="0,1,2,..." turns every model created through pfhip_create / pfhip_create_from_memory into a group with one
// replica per listed device (the `device` argument is then ignored): the unchanged server with its one shared handle and
// `decoder-thread-num` threads (funasr-wss-server.cpp:479-481) uses all of them.
static bool env_devices(std::vector<int>& devs) {
  const char* e = std::getenv("PFHIP_DEVICES");
  if (!e || !*e) return false;
  devs.clear();
  std::stringstream ss(e);
  std::string tok;
  while (std::getline(ss, tok, ',')) {
    if (tok.empty()) continue;
    char* end = nullptr;
    const long v = std::strtol(tok.c_str(), &end, 10);
    if (end == tok.c_str() || *end != '\0' || v < 0) return false;
    devs.push_back((int)v);
  }
  return !devs.empty();
}

// PFHIP_INFLIGHT=n: every handle is created with n execution contexts per device (pfhip_set_inflight)
static pfhip_status apply_env_inflight(pfhip_model** out) {
  const char* e = std::getenv("PFHIP_INFLIGHT");
  if (!e || !*e) return PFHIP_OK;
  const int n = std::atoi(e);
  if (n < 1 || n > 16) return PFHIP_OK;
  const pfhip_status st = pfhip_set_inflight(*out, n);
  if (st) { const std::string why = g_err; pfhip_destroy(*out); *out = nullptr; g_err = why; }
  return st;
}

pfhip_status pfhip_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                                      pfhip_model** out) {
  g_err.clear();
  std::vector<int> devs;
  if (env_devices(devs)) return pfhip_create_group(blob, blob_bytes, manifest_json, devs.data(), (int)devs.size(), out);
  try {
    const pfhip_status st = build_model(blob, blob_bytes, manifest_json, device, out);
    return st ? st : apply_env_inflight(out);
  } catch (const std::exception& e) { return fail(PFHIP_ERR_FORMAT, e.what()); }
}

int pfhip_group_size(const pfhip_model* m) { return m ? 1 + (int)m->replicas.size() : 0; }

pfhip_status pfhip_group_stats(pfhip_model* m, int* devices, int64_t* calls, int64_t* utterances, int* open_streams, int cap) {
  g_err.clear();
  if (!m || cap < 1 + (int)m->replicas.size()) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> l(m->bq.mu);             // pfhip_set_inflight grows `contexts` under this lock
  for (int i = 0; i <= (int)m->replicas.size(); ++i) {
    const pfhip_model* r = i == 0 ? m : m->replicas[(size_t)i - 1];
    if (devices) devices[i] = r->device;
    int64_t nc = r->served_calls.load(), nu = r->served_utts.load();
    for (const pfhip_model* cx : r->contexts) { nc += cx->served_calls.load(); nu += cx->served_utts.load(); }
    if (calls) calls[i] = nc;
    if (utterances) utterances[i] = nu;
    if (open_streams) open_streams[i] = r->live_streams.load();
  }
  return PFHIP_OK;
}

pfhip_status pfhip_create(const char* weight_blob_path, const char* manifest_json_path, int device, pfhip_model** out) {
  g_err.clear();
  if (!weight_blob_path || !manifest_json_path || !out) return fail(PFHIP_ERR_ARG, "null argument");
  std::vector<char> blob, man;
  pfhip_status st = read_file(weight_blob_path, blob);
  if (st) return st;
  st = read_file(manifest_json_path, man);
  if (st) return st;
  man.push_back('\0');
  return pfhip_create_from_memory(blob.data(), blob.size(), man.data(), device, out);
}

void pfhip_destroy(pfhip_model* m) { delete m; }

int pfhip_sample_rate(const pfhip_model* m) { return m ? m->weights->cfg.sample_rate : 0; }
int pfhip_vocab_size(const pfhip_model* m) { return m ? m->weights->cfg.vocab : 0; }
int pfhip_feat_dim(const pfhip_model* m) { return m ? m->weights->feat_dim : 0; }
int pfhip_d_model(const pfhip_model* m) { return m ? m->weights->cfg.d_model : 0; }
int pfhip_head_dim(const pfhip_model* m) { return m && m->weights->cfg.n_head > 0 ? m->weights->cfg.d_model / m->weights->cfg.n_head : 0; }

// The fire frames of the calling thread's last pfhip_offline_fetch / pfhip_offline_forward_resident, for pfhip_offline_fetch_fire_frames:
// copied out of the execution slot while its lock is still held, into storage the thread owns, already laid out by that call's batch and
// max_tokens (per utterance its count and its frames).  On a shared handle another thread may take the slot the moment the lock is
// gone; what this thread reads later is its own call's, and no slot state.  Matched on the handle's uid, not its address.
namespace {
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
}  // namespace

// every Paraformer entry point on a SenseVoice handle
static bool is_svs(const pfhip_model* m) { return m && m->weights->cfg.svs; }
static pfhip_status refuse_svs() { return fail(PFHIP_ERR_UNSUPPORTED, "a SenseVoice (CTC) model is run through pfhip_svs_forward"); }

static pfhip_status offline_enqueue(pfhip_model* m, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
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

// fs_in: the rate of `pcm` when it is not the model's (resampled into the slot's PCM workspace first), else 0
// hotword sets of a call: n_sets sets (emb[k]: [n[k], d]) and, per utterance, which one it attends to (of_utt == nullptr: all set 0)
struct HwSets { const float* const* emb; const int* n; int n_sets; const int* of_utt; };

static pfhip_status forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch,
                                   const HwSets& hw, pfhip_out* out, int fs_in = 0, const pfhip_detail* dt = nullptr) {
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->own_stream;
  m->prof_stream = s;
  if (dt && dt->nbest_k > m->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "nbest k larger than the vocabulary");      // before any launch
  m->nbest_k = dt ? dt->nbest_k : 0;
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

// ---- execution slots -----------------------------------------------------------------------------------------------
// A handle fronts one or more execution slots: the contexts of its device (pfhip_set_inflight) and of every replica device
// (pfhip_create_group).  `slots` on the head lists them device-major per round (context 0 of every device, then context 1 of
// every device, ...), so that filling them in order spreads calls over the GPUs before it stacks them on one.
static void rebuild_slots_locked(pfhip_model* head) {
  head->slots.clear();
  std::vector<pfhip_model*> devs{head};
  for (pfhip_model* r : head->replicas) devs.push_back(r);
  size_t rounds = 0;
  for (pfhip_model* d : devs) rounds = std::max(rounds, d->contexts.size() + 1);
  for (size_t k = 0; k < rounds; ++k)
    for (pfhip_model* d : devs) {
      if ((int)k >= head->ctx_limit) continue;
      if (k == 0) head->slots.push_back(d);
      else if (k - 1 < d->contexts.size()) head->slots.push_back(d->contexts[k - 1]);
    }
}

// least-loaded slot (ties: round-robin); used by calls that bypass the queue
static pfhip_model* acquire_slot(pfhip_model* head) {
  std::lock_guard<std::mutex> l(head->bq.mu);
  if (head->slots.empty()) rebuild_slots_locked(head);
  const size_t n = head->slots.size();
  const unsigned start = head->rr.fetch_add(1);
  pfhip_model* best = nullptr;
  int best_load = 0;
  for (size_t k = 0; k < n; ++k) {
    pfhip_model* r = head->slots[(start + k) % n];
    const int load = r->inflight.load();
    if (!best || load < best_load) { best = r; best_load = load; }
  }
  ++best->inflight;
  return best;
}
static void release_slot(pfhip_model* head, pfhip_model* slot) {
  --slot->inflight;
  head->bq.slot_freed();
}

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
struct BatchReq : pfhip_impl::MergeReqBase {
  HostPcm pcm{static_cast<const float* const*>(nullptr)}; const int* n; int batch; pfhip_out* out;
  HwSets hw{nullptr, nullptr, 0, nullptr};          // the caller's hotword sets (contextual models)
  const pfhip_detail* dt = nullptr;                 // the caller's candidate / fire-frame buffers (pfhip_offline_forward_detail), or none
  pfhip_status st = PFHIP_OK; std::string err;
};

// one packed forward on `m` for everybody in `take` (all of one sample format: forward_batched's pick splits the queue by format)
static void run_batch_requests(pfhip_model* m, const std::vector<BatchReq*>& all_taken) {
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

namespace { thread_local pfhip_model* tl_last_replica = nullptr; }      // where this thread's last offline forward ran (debug getters)
// pfhip_svs_align: per handle (its uid), where this thread's last pfhip_svs_forward on it ran — the context's uid and that context's
// forward count then.  Handles come and go; the note is emptied when it has grown past 64 handles.
namespace {
struct SvsNote { uint64_t ctx_uid, serial; };
thread_local std::map<uint64_t, SvsNote> tl_svs_notes;
}

// Callers of both sample formats share the queue; a packed forward holds ONE format, the leader's: pick takes the queued callers of
// that format (in order) and leaves the others, in order, for the next leader.  Nothing is converted on the host, every caller gets
// the results of a forward in its own format, which are those of the other format bit for bit.
static pfhip_status forward_batched(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                    const HwSets& hw, pfhip_out* out, const pfhip_detail* dt) {
  BatchReq me;
  me.pcm = pcm; me.n = n_samples; me.batch = batch; me.out = out; me.hw = hw; me.dt = dt;
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
        run_batch_requests(r, take);
        ++r->served_forwards; r->served_calls += (int64_t)take.size(); r->served_utts += utts;
      });
  if (ran_on) tl_last_replica = ran_on;       // the leader's own slice ran there; followers ask the handle (pfhip_get_tensor: head)
  if (me.st != PFHIP_OK) g_err = me.err;
  return me.st;
}

// dt: candidates and / or fire frames beside `out` (nbest_k = 0: no candidates), or null.  rate: the rate of `pcm`, none or the model's
// own for audio at the model's rate; another rate is resampled on the device into the slot's PCM workspace and runs alone (one rate
// pair per packed batch)
static pfhip_status offline_forward_sets(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const HwSets& hw,
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

static pfhip_status offline_forward_hwsets(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                           const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                           pfhip_out* out) {
  if (head && head->weights->cfg.contextual && n_sets > 0 && (!hw_emb || !n_hotwords || !set_of_utt)) {
    g_err.clear();
    return fail(PFHIP_ERR_ARG, "bad argument");
  }
  const HwSets hw{hw_emb, n_hotwords, n_sets < 0 ? 0 : n_sets, set_of_utt};
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

// pfhip_offline_forward_hwsets plus the k best candidates of every token row (an extension: GreedySearch, paraformer.cpp:386-395,
// keeps only the arg-max); nb == nullptr is pfhip_offline_forward_hwsets itself
static pfhip_status offline_forward_nbest(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out, const pfhip_nbest* nb) {
  if (head && head->weights->cfg.contextual && n_sets > 0 && (!hw_emb || !n_hotwords || !set_of_utt)) {
    g_err.clear();
    return fail(PFHIP_ERR_ARG, "bad argument");
  }
  const HwSets hw{hw_emb, n_hotwords, n_sets < 0 ? 0 : n_sets, set_of_utt};
  if (!nb) return offline_forward_sets(head, pcm, n_samples, batch, hw, out);
  if (nb->k < 1) { g_err.clear(); return fail(PFHIP_ERR_ARG, "nbest: k outside 1..8 (or above the vocabulary) or a null buffer"); }
  const pfhip_detail dt{nb->k, nb->ids, nb->logp, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, &dt);
}

// the hwsets form with a pfhip_detail (candidates and / or fire frames) and the rate of the audio
static pfhip_status offline_forward_detail(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, int sample_rate,
                                           const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                           pfhip_out* out, const pfhip_detail* dt) {
  if (head && head->weights->cfg.contextual && n_sets > 0 && (!hw_emb || !n_hotwords || !set_of_utt)) {
    g_err.clear();
    return fail(PFHIP_ERR_ARG, "bad argument");
  }
  const HwSets hw{hw_emb, n_hotwords, n_sets < 0 ? 0 : n_sets, set_of_utt};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, dt, sample_rate == 0 ? std::nullopt : std::optional<int>(sample_rate));      // 0 = the model's
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

// pfhip_offline_forward with the PCM already in HBM: same routing over the execution slots, no H2D of the audio
static pfhip_status offline_forward_resident(pfhip_model* head, PcmView d_pcm, const int64_t* sample_off, const int* n_samples,
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
pfhip_status pfhip_offline_forward_resident(pfhip_model* head, const float* d_pcm, const int64_t* sample_off, const int* n_samples,
                                            int batch, pfhip_out* out) {
  return offline_forward_resident(head, PcmView{d_pcm, false}, sample_off, n_samples, batch, out);
}
pfhip_status pfhip_offline_forward_resident_s16(pfhip_model* head, const int16_t* d_pcm, const int64_t* sample_off,
                                                const int* n_samples, int batch, pfhip_out* out) {
  return offline_forward_resident(head, PcmView{d_pcm, true}, sample_off, n_samples, batch, out);
}

// pfhip_offline_forward at the caller's rate: resampled on the device into the slot's PCM workspace, then the same forward
static pfhip_status offline_forward_rate(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, int sample_rate,
                                         const float* hw_emb, int n_hotwords, pfhip_out* out) {
  const HwSets hw{&hw_emb, &n_hotwords, hw_emb && n_hotwords > 0 ? 1 : 0, nullptr};
  return offline_forward_sets(head, pcm, n_samples, batch, hw, out, nullptr, sample_rate);
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

pfhip_status pfhip_set_batching(pfhip_model* m, int wait_us, int max_utterances) {
  g_err.clear();
  if (!m || wait_us < 0 || max_utterances < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  if (is_svs(m)) return fail(PFHIP_ERR_UNSUPPORTED, "merging concurrent callers is not built for SenseVoice (CTC) models");
  std::lock_guard<std::mutex> ql(m->bq.mu);
  m->batch_wait_us = wait_us;
  m->batch_max_utts = max_utterances;
  return PFHIP_OK;
}

// every execution slot of the handle, for calls that configure all of them
static std::vector<pfhip_model*> all_slots(pfhip_model* head) {
  std::lock_guard<std::mutex> l(head->bq.mu);
  if (head->slots.empty()) rebuild_slots_locked(head);
  return head->slots;
}

pfhip_status pfhip_set_inflight(pfhip_model* head, int n) {
  g_err.clear();
  if (!head || n < 1 || n > 16) return fail(PFHIP_ERR_ARG, "in-flight count outside 1..16");
  if (head->group_head || head->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  std::vector<pfhip_model*> devs{head};
  for (pfhip_model* r : head->replicas) devs.push_back(r);
  for (pfhip_model* d : devs) {
    while ((int)d->contexts.size() + 1 < n) {
      pfhip_model* cx = nullptr;
      pfhip_status st = build_context(d, &cx);
      if (st) return st;
      cx->group_head = head;
      cx->ctx_index = (int)d->contexts.size() + 1;
      std::lock_guard<std::mutex> l(head->bq.mu);
      d->contexts.push_back(cx);
    }
  }
  // fewer than before: the extra contexts stay allocated (a call may be running on one) but leave the slot list
  std::lock_guard<std::mutex> l(head->bq.mu);
  head->ctx_limit = n;
  rebuild_slots_locked(head);
  return PFHIP_OK;
}

int pfhip_get_inflight(const pfhip_model* m) {
  if (!m) return 0;
  pfhip_model* head = const_cast<pfhip_model*>(m);
  std::lock_guard<std::mutex> l(head->bq.mu);
  if (head->slots.empty()) rebuild_slots_locked(head);
  int n = 0;
  for (pfhip_model* sl : head->slots) n = std::max(n, sl->ctx_index + 1);
  return n;
}

pfhip_status pfhip_inflight_stats(pfhip_model* head, pfhip_slot_stats* out, int cap, int* n_out) {
  g_err.clear();
  if (!head || !n_out) return fail(PFHIP_ERR_ARG, "bad argument");
  const std::vector<pfhip_model*> sl = all_slots(head);
  *n_out = (int)sl.size();
  if (!out || cap < (int)sl.size()) return fail(PFHIP_ERR_CAPACITY, "slot array too small");
  for (size_t i = 0; i < sl.size(); ++i) {
    out[i].device = sl[i]->device; out[i].context = sl[i]->ctx_index;
    out[i].forwards = sl[i]->served_forwards.load(); out[i].calls = sl[i]->served_calls.load();
    out[i].utterances = sl[i]->served_utts.load();
  }
  return PFHIP_OK;
}

// The default set becomes (or stays) a pinned entry of the device's bank: filled on the owner's stream and waited for, the previous
// default let go.  owner->mu is held.  A set the bank cannot take stays a host copy and is projected per call.
static pfhip_status pin_default_hotwords(pfhip_model* owner, const float* hw_emb, int H) {
  HIP_TRY(hipSetDevice(owner->device));
  HIP_TRY(hipDeviceSynchronize());            // a forward enqueued with the previous default (pfhip_offline_enqueue) has finished
  HwBankDev& D = *owner->hwbank;
  std::lock_guard<std::mutex> l(D.mu);
  ensure_bank_locked(owner);
  const int old = D.default_id;
  D.default_id = -1;
  if (hw_emb && H > 0) {
    bool hit = false;
    const int id = D.bank.acquire(hw_emb, H, &hit);
    if (id >= 0 && !hit) {
      HIP_TRY(owner->hw.ensure((size_t)round_up(H, pfhip::kTileM) * owner->weights->cfg.d_model * 4));
      const pfhip_status st = fill_slab_locked(owner, D, id, 0, owner->own_stream);
      if (st) return st;
      HIP_TRY(hipStreamSynchronize(owner->own_stream));
      D.bank.entry(id).settled = true;          // complete: nobody needs to wait for its event
    }
    D.default_id = id;
  }
  if (old >= 0) D.bank.release(old);
  return PFHIP_OK;
}

static std::vector<pfhip_model*> device_owners(pfhip_model* head) {
  std::lock_guard<std::mutex> l(head->bq.mu);
  std::vector<pfhip_model*> devs{head};
  for (pfhip_model* r : head->replicas) devs.push_back(r);
  return devs;
}

pfhip_status pfhip_set_hotwords(pfhip_model* m, const float* hw_emb, int n_hotwords) {
  g_err.clear();
  if (!m || !hw_emb || n_hotwords <= 0) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!m->weights->cfg.contextual) return fail(PFHIP_ERR_UNSUPPORTED, "model has no bias decoder (use_hotword == false)");
  if (m->group_head || m->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  for (pfhip_model* r : device_owners(m)) {          // one bank per device, shared by its contexts
    std::lock_guard<std::mutex> lk(r->mu);
    const pfhip_status st = pin_default_hotwords(r, hw_emb, n_hotwords);
    if (st) return st;
  }
  auto copy = std::make_shared<const std::vector<float>>(hw_emb, hw_emb + (size_t)n_hotwords * m->weights->cfg.d_model);
  std::lock_guard<std::mutex> l(m->bq.mu);
  m->hw_default = std::move(copy);
  return PFHIP_OK;
}

pfhip_status pfhip_set_hotword_merging(pfhip_model* m, int on) {
  g_err.clear();
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  std::lock_guard<std::mutex> l(m->bq.mu);
  m->hw_merge = on != 0;
  return PFHIP_OK;
}

pfhip_status pfhip_set_hotword_bank_bytes(pfhip_model* m, int64_t bytes) {
  g_err.clear();
  if (!m || bytes < 0) return fail(PFHIP_ERR_ARG, "bad argument");
  if (m->group_head || m->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  const std::shared_ptr<const std::vector<float>> def = default_hotwords(m);
  for (pfhip_model* r : device_owners(m)) {
    std::lock_guard<std::mutex> lk(r->mu);
    HIP_TRY(hipSetDevice(r->device));
    HwBankDev& D = *r->hwbank;
    {
      std::lock_guard<std::mutex> l(D.mu);
      for (size_t i = 0; i < D.bank.id_count(); ++i) {
        const HotwordBank::Entry& e = D.bank.entry((int)i);
        if (e.live && e.pins > ((int)i == D.default_id ? 1 : 0))
          return fail(PFHIP_ERR_ARG, "hotword bank in use: set its bound while no forward is in flight");
      }
      HIP_TRY(hipDeviceSynchronize());
      if (D.arena) HIP_TRY(hipFree(D.arena));
      D.arena = nullptr;
      D.bound_bytes = bytes;
      D.configured = false;
      ensure_bank_locked(r);
    }
    if (def && !def->empty()) {
      const pfhip_status st = pin_default_hotwords(r, def->data(), (int)(def->size() / (size_t)m->weights->cfg.d_model));
      if (st) return st;
    }
  }
  return PFHIP_OK;
}

pfhip_status pfhip_hotword_bank_stats(pfhip_model* m, pfhip_hwbank_stats* out) {
  g_err.clear();
  if (!m || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  *out = pfhip_hwbank_stats{};
  const int64_t row_bytes = (int64_t)2 * m->weights->cfg.d_model * 4;
  for (pfhip_model* r : device_owners(m)) {
    HwBankDev& D = *r->hwbank;
    std::lock_guard<std::mutex> l(D.mu);
    out->hits += D.bank.hits; out->misses += D.bank.misses; out->evictions += D.bank.evictions;
    out->refused += D.bank.refused;
    out->bytes_in_use += (int64_t)D.bank.used_granules() * D.bank.granule_rows() * row_bytes;
    out->bytes_capacity += (int64_t)D.bank.capacity_granules() * D.bank.granule_rows() * row_bytes;
    out->sets_resident += D.bank.live_entries();
    out->forwards += D.forwards; out->per_call_forwards += D.percall_forwards;
    out->sets_in_forwards += D.sets_total;
    out->max_sets_in_forward = std::max(out->max_sets_in_forward, D.sets_max);
  }
  return PFHIP_OK;
}

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

// one packed forward on slot m, its range-guard re-run included, and the results into out
static pfhip_status svs_forward_direct(pfhip_model* m, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid,
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

static pfhip_status svs_forward(pfhip_model* head, HostPcm pcm, const int* n_samples, int batch, const int32_t* lid, const int32_t* textnorm,
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
  tl_last_replica = m;
  const pfhip_status st = svs_forward_direct(m, pcm, n_samples, batch, lid, textnorm, out);
  ++m->served_forwards; ++m->served_calls; m->served_utts += batch;
  release_slot(head, m);
  return st;
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

int pfhip_is_contextual(const pfhip_model* m) { return m ? m->weights->cfg.contextual : 0; }
int pfhip_has_timestamp_head(const pfhip_model* m) { return m ? m->weights->cfg.timestamp : 0; }

// model_eb.onnx Run + row selection (paraformer.cpp:656-685): Embedding -> 1-layer LSTM over the 10 padded positions,
// output of hotword j taken at step lengths[j]-1.
pfhip_status pfhip_hotword_embed(pfhip_model* m, const int32_t* hotword_matrix, const int32_t* lengths, int n_hotwords,
                                 float* out) {
  g_err.clear();
  if (!m || !hotword_matrix || !lengths || n_hotwords <= 0 || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!m->weights->cfg.contextual) return fail(PFHIP_ERR_UNSUPPORTED, "model has no hotword embedder (use_hotword == false)");
  const int H = n_hotwords, L = 10, d = m->weights->cfg.d_model;
  for (int j = 0; j < H; ++j) {
    if (lengths[j] < 1 || lengths[j] > L) return fail(PFHIP_ERR_ARG, "hotword length outside 1..10");
    for (int t = 0; t < L; ++t)
      if (hotword_matrix[j * L + t] < 0 || hotword_matrix[j * L + t] >= m->weights->cfg.vocab) return fail(PFHIP_ERR_ARG, "hotword id outside the vocabulary");
  }
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->own_stream;
  const int R = L * H, Rp = round_up(R, pfhip::kTileM), Hp = round_up(H, pfhip::kTileM);
  const Contextual& bias = m->weights->bias;
  Buf ids, lens, X, GX, G, hc;
  HIP_TRY(ids.ensure((size_t)R * 4)); HIP_TRY(lens.ensure((size_t)H * 4));
  HIP_TRY(X.ensure((size_t)Rp * d * 4)); HIP_TRY(GX.ensure((size_t)(Rp + pfhip::kTileM) * 4 * d * 4)); HIP_TRY(G.ensure((size_t)Hp * 4 * d * 4));
  HIP_TRY(hc.ensure((size_t)3 * Hp * d * 4));
  // time-major ids: row t*H + j = token t of hotword j
  std::vector<int32_t> tm((size_t)R);
  for (int j = 0; j < H; ++j) for (int t = 0; t < L; ++t) tm[(size_t)t * H + j] = hotword_matrix[j * L + t];
  HIP_TRY(hipMemcpyAsync(ids.p, tm.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(lens.p, lengths, (size_t)H * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(hc.p, 0, (size_t)3 * Hp * d * 4, s));
  float* h = hc.f(); float* cst = h + (size_t)Hp * d; float* sel = cst + (size_t)Hp * d;
  pfhip::launch_gather_rows(static_cast<const int32_t*>(ids.p), bias.embed_w, d, X.f(), R, s);
  gemm(m, s, X.f(), d, bias.lstm_ih, 4 * d, d, d, GX.f(), 4 * d, nullptr, 0, nullptr, 0, R, false);
  for (int t = 0; t < L; ++t) {
    gemm(m, s, h, d, bias.lstm_hh, 4 * d, d, d, G.f(), 4 * d, GX.f() + (size_t)t * H * 4 * d, 4 * d, nullptr, 0, H, false);
    pfhip::launch_lstm_cell(G.f(), cst, h, static_cast<const int32_t*>(lens.p), t, sel, H, d, s);
  }
  HIP_TRY(hipMemcpyAsync(out, sel, (size_t)H * d * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
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
  if (!m->replicas.empty() && tl_last_replica && (tl_last_replica == m || tl_last_replica->group_head == m)) m = tl_last_replica;
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->prof_stream ? m->prof_stream : m->own_stream;
  const std::string nm(name);
  const void* src = nullptr;
  size_t n = 0;
  const int d = m->weights->cfg.d_model;
  if (nm == "feats") { src = m->feats.p; n = (size_t)m->M * m->weights->feat_dim; }
  else if (nm == "enc") { src = m->weights->cfg.svs ? m->x.p : m->enc.p; n = (size_t)m->M * d; }      // SenseVoice: the rows after tp.norm
  else if (nm == "lse" && m->weights->cfg.svs) { src = m->svs_lse.p; n = (size_t)m->M; }             // the rows' log-sum-exp either CTC head kept
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
  if (std::string(what) == "ctc_head_chunks") {
    // (looked up among this handle's contexts, never dereferenced before it is found there: the note may be of a handle since destroyed)
    for (pfhip_model* cx : m->contexts)
      if (cx == tl_last_replica) return (pfhip_status)cx->svs_head_chunks;
    return (pfhip_status)m->svs_head_chunks;
  }
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
