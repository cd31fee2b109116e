// What a model holds that is read-only after load: one ModelWeights per device, built by build_model (model_build.cpp), shared by the
// weight owner and its execution contexts through a shared_ptr and freed by its destructor when the last of them goes.  Every
// pointer a forward needs is a resolved field of the typed tables below; names and host pointers exist only inside the builder.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "kernels.h"

namespace pfhip_impl {

// A device allocation made once at load (weights, tables): exact size, move-only, freed by its destructor.
struct DevMem {
  void* p = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevMem& operator=(DevMem&& o) noexcept { std::swap(p, o.p); return *this; }
  ~DevMem() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 1)); }
  hipError_t upload(const void* src, size_t bytes) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess || !bytes ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
  }
  template <typename T> hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size() * sizeof(T)); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
  float* f() const { return as<float>(); }
};

struct Config {
  int d_model = 512, n_head = 4, ffn = 2048, enc_layers = 50, dec_layers = 16, dec_ffn = 2048;
  int dec_n_head = 0;          // decoder_conf.attention_heads when it differs from the encoder's; pfhip_create resolves 0 to n_head
  int kernel = 11, vocab = 8404, n_mels = 80, lfr_m = 7, lfr_n = 6, pred_residual = 0, contextual = 0, timestamp = 0;
  float smooth_factor2 = 0.25f, noise_threshold2 = 0.01f;      // CifPredictorV3 timestamp head
  float cif_threshold = 1.0f, tail_threshold = 0.45f, smooth_factor = 1.0f, noise_threshold = 0.0f;
  int sample_rate = 16000;
  // config.kind == "sensevoice" (SenseVoiceSmall, sensevoice-small.cpp): the SAN-M encoder is followed by tp_layers more layers of
  // the same kind, tp.norm and a CTC head over every row; no predictor, no decoder.  Widths and wiring recalled from upstream FunASR.
  int svs = 0, tp_layers = 0, blank_id = 0;
};

struct FrontendTables {
  DevMem window, tw, mel_off, mel_size, mel_w;
  // the front-end kernels' view, with a model's CMVN vectors
  pfhip::FbankTables fbank(const float* cmvn_mean, const float* cmvn_istd) const {
    return {window.as<float>(), tw.as<double>(), mel_off.as<int>(), mel_size.as<int>(), mel_w.as<float>(), cmvn_mean, cmvn_istd};
  }
};

// fp32 weight in the torch [out, in] layout, its bias (may be null) and the power-of-two scale the fp16 two-plane GEMM stages the
// weight with (kernels.h best_w_scale: fixed at load from its largest magnitude)
struct Linear { const float* w = nullptr; const float* b = nullptr; float scale = 1.0f; };
struct Norm { const float* g = nullptr; const float* b = nullptr; };
// fp16 plane image of a weight (gemm_p3.hip), scale baked in; null when the images were not built
struct Planes { const unsigned char* hi = nullptr; const unsigned char* lo = nullptr; float scale = 1.0f; };
// a Linear with the LayerNorm in front of it folded in (gemm_x6.hip LN-on-load): W * gamma, b + W beta, the column sums of the
// folded weight as stored, and its plane image; folded.w is null where the fold was not built
struct FoldLin { Linear folded; const float* colsum = nullptr; Planes img; };

struct EncLayer {
  Norm norm1, norm2;
  Linear qkv, out, ffn1, ffn2;          // layer 0: qkv.w is the copy K-padded to feat_pad
  const float* fsmn_w = nullptr;
  FoldLin qkv_f, ffn1_f;                // norm1 -> qkv (layers >= 1), norm2 -> ffn1
  Planes out_img, ffn2_img;
};
struct DecFfn { Norm norm1, ffn_norm; Linear ffn1, ffn2; FoldLin ffn1_f, ffn2_f; };
struct DecLayer {
  DecFfn ffn;
  Norm norm2, norm3;
  const float* fsmn_w = nullptr;
  Linear q, kv, out;
  FoldLin q_f;                          // norm3 -> q (streaming latency path)
  Planes kv_img, out_img;
};
struct Predictor { Linear conv; const float* out_w = nullptr; const float* out_b = nullptr; };      // conv.w: [d][3d] im2col order
// contextual model: hotword embedder (Embedding + LSTM) and the bias decoder of the last layer
struct Contextual { const float* embed_w = nullptr; Linear lstm_ih, lstm_hh; Norm norm3; Linear q, kv, out, merge; };
// timestamp head: ConvTranspose1d as one GEMM [3d][d] + tiled bias, both LSTM directions' input weights [8d][d] + summed biases,
// recurrent weights [2][4d][d], the second alpha head
struct TimestampHead { Linear up, ih; const float* whh = nullptr; const float* out2_w = nullptr; float out2_b = 0.f; };

struct ModelWeights {
  Config cfg;
  int feat_dim = 560, feat_pad = 576, vocab_pad = 8448;
  double static_bound = 0.0;          // load-time bound on |Linear(LayerNorm(x))| over the model's layers
  bool always_exact = false;          // that bound reaches fp16's range: every forward runs the exact kernels
  bool enc_folded = false, dec_folded = false;      // the LayerNorm folds were built (d_model == 512; decoder: dec_ffn % 128 == 0)
  bool enc_planes = false, dec_planes = false;      // ... and the plane images on top of them

  FrontendTables ft;
  const float* cmvn_mean = nullptr; const float* cmvn_istd = nullptr;
  const float* inv_ts = nullptr;                    // position-encoding timescales
  std::vector<EncLayer> enc;          // a SenseVoice container: enc.0 .. enc.{enc_layers-1}, then tp.0 .. tp.{tp_layers-1}
  Norm enc_after;
  Norm tp_norm;                       // cfg.svs: after the last tp layer
  const float* svs_embed = nullptr;   // cfg.svs: the prompt embedding [16][feat_dim]
  Linear ctc;                         // cfg.svs: ctc.w [vocab][d], b: ctc.b padded to vocab_pad
  Predictor pred;
  std::vector<DecLayer> dec;
  DecFfn dec3;
  Norm dec_after;
  Linear dec_out;                     // b: dec.out.b padded to vocab_pad
  Linear kv_all;                      // every decoder layer's kv stacked [layers * 2d][d]: one launch projects a streaming window
  Contextual bias;                    // cfg.contextual
  TimestampHead ts;                   // cfg.timestamp

  // the allocations behind the pointers above
  DevMem blob, w0qkv, predconv, vocab_bias, kv_all_w, kv_all_b, inv_ts_mem;
  DevMem lnw_qkv, lnb_qkv, lns_qkv, lnw_ffn1, lnb_ffn1, lns_ffn1;                         // encoder folds [layers][N][d] / [layers][N]
  DevMem dlnw1, dlnb1, dlns1, dlnw2, dlnb2, dlns2, dlnw3, dlnb3, dlns3;                   // decoder folds, [dec_layers + 1] entries (dec3 last)
  DevMem wplanes, dwplanes;           // plane images per layer: { qkv' | out | ffn1' | ffn2 }, { ffn1' | ffn2' | kv | out }
  DevMem up_w, up_b, wih, bih, whh;
};

}  // namespace pfhip_impl
