// DNSMOS speech-quality scores on MI355X — the C ABI's pfhip_mos_* family.  Replaces ComputeScore of the reference tree's
// utils/dnsmos_local.py:24-104: the two onnxruntime sessions (sig_bak_ovr.onnx: P.835 signal / background / overall; model_v8.onnx:
// P.808), the librosa mel input of the second, the clip loop and the polynomial maps.  Kernels: conv3x3.hip, dnsmos.hip.
//
// At load (pfhip_mos_create_from_memory; _from_files reads the two .onnx files through mos_files.cpp into the same container) every
// weight goes to the device ONCE: the convolution kernels of the Cin >= 32 layers as their two fp16 plane images times a power-of-two
// scale fixed from the kernel's largest magnitude — a weight that is not finite, or whose scaled magnitude leaves 32768, is refused
// here, as the range guard of the GEMMs does at load —, the STFT kernels as the transposed table, the mel front end's tables built in
// double.  A call packs the windows of all its clips along N and runs them in slabs of pfhip_mos_set_workspace bytes of activations
// (two ping-pong buffers; the call's samples and the 16 bytes of results per window lie outside the cap).  Every kernel works per
// window in a fixed order: a window's numbers do not depend on the slab it falls into or on what else the call holds.
// The clip loop is dnsmos_local.py:59-77 with its double arithmetic, polynomials and means on the host in double.
#include <memory>

#include "internal.h"
#include "json_min.h"
#include "model_files.h"

using namespace pfhip_impl;

namespace {
constexpr int kFs = 16000;
constexpr double kInputLength = 9.01;
constexpr int kLenSamples = 144160;               // int(9.01 * 16000)
constexpr int kFrames = 900, kBins = 161;

struct ConvLayer {
  int cin = 0, cout = 0, pool = 0;
  const float* w = nullptr;                       // fp32 ONNX layout (Cin == 1 only)
  const float* b = nullptr;
  const void* hi = nullptr;                       // plane images (Cin >= 32)
  const void* lo = nullptr;
  float scale = 1.0f;
};
struct MosNet {
  std::vector<ConvLayer> convs;
  const float* dw[3] = {nullptr, nullptr, nullptr};
  const float* db[3] = {nullptr, nullptr, nullptr};
  int din[3] = {0, 0, 0}, dout[3] = {0, 0, 0};
  int H0 = 0, W0 = 0;
  size_t max_floats = 0;                          // the largest activation tensor of one window
};
}  // namespace

struct pfhip_mos {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  bool has_p808 = false;
  MosNet net[2];
  const float* stft_tab = nullptr;
  float floor_v = 0.f, denom = 1.f;
  const float* mel_tab = nullptr;
  const float* mel_T = nullptr;
  size_t workspace = (size_t)2 << 30;
  std::vector<DevMem> owned;
  ~pfhip_mos() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

double polyval(const double* c, int n, double x) {
  double y = 0.0;
  for (int i = 0; i < n; ++i) y = y * x + c[i];
  return y;
}
// get_polyfit_val (dnsmos_local.py:35-49), highest power first
const double kOvr[3] = {-0.06766283, 1.11546468, 0.04602535}, kSig[3] = {-0.08397278, 1.22083953, 0.0052439},
             kBak[3] = {-0.13166888, 1.60915514, -0.39604546};
const double kOvrP[4] = {-0.00533021, 0.005101, 1.18058466, -0.11236046}, kSigP[4] = {-0.01019296, 0.02751166, 1.19576786, -0.24348726},
             kBakP[4] = {-0.04976499, 0.44276479, -0.1644611, 0.96883132};

// the layers of one net on `n` windows: in -> (ping-pong a / b) -> out [n][D3]
bool run_net(const pfhip_mos* h, const MosNet& net, const float* in, float* a, float* b, int n, float* out) {
  int H = net.H0, W = net.W0;
  const float* cur = in;
  float* dst = a;
  for (const ConvLayer& c : net.convs) {
    const bool ok = c.cin == 1 ? pfhip::launch_conv3x3_c1_relu(cur, c.w, c.b, dst, n, H, W, c.cout, c.pool != 0, h->stream)
                               : pfhip::launch_conv3x3_relu(cur, c.hi, c.lo, c.scale, c.b, dst, n, H, W, c.cin, c.cout, c.pool != 0, h->stream);
    if (!ok) return false;
    if (c.pool) { H /= 2; W /= 2; }
    cur = dst;
    dst = dst == a ? b : a;
  }
  return pfhip::launch_globalmax_mlp(cur, n, H * W, net.din[0], net.dw[0], net.db[0], net.dout[0], net.dw[1], net.db[1], net.dout[1], net.dw[2],
                                     net.db[2], net.dout[2], out, h->stream);
}

// The clip loop and the forward.  raw [windows][4] = (p808, sig, bak, ovr); p808 NaN without the second net.
template <typename Sample>
pfhip_status score_windows(pfhip_mos* h, const Sample* const* pcm, const int64_t* n_samples, int n_clips, std::vector<int>& hops,
                           std::vector<int>& scored, std::vector<float>& raw) {
  if (!h || (n_clips > 0 && (!pcm || !n_samples)) || n_clips < 0) return fail(PFHIP_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  HIP_TRY(hipSetDevice(h->device));
  std::vector<Sample> host;
  std::vector<int64_t> offs;
  hops.assign(n_clips, 0);
  scored.assign(n_clips, 0);
  for (int c = 0; c < n_clips; ++c) {
    if (!pcm[c] || n_samples[c] < 1) return fail(PFHIP_ERR_ARG, "clip " + std::to_string(c) + " is empty: it has no score");
    // a clip shorter than one window is appended to itself until it is not (dnsmos_local.py:61-62)
    int64_t len = n_samples[c];
    while (len < kLenSamples) len *= 2;
    const size_t base = host.size();
    host.resize(base + (size_t)len);
    for (int64_t at = 0; at < len; at += n_samples[c]) std::copy(pcm[c], pcm[c] + n_samples[c], host.begin() + base + at);
    const int num_hops = (int)(std::floor((double)len / kFs) - kInputLength) + 1;
    hops[c] = num_hops;
    for (int idx = 0; idx < num_hops; ++idx) {
      const int64_t b = (int64_t)((double)idx * kFs), e = (int64_t)(((double)idx + kInputLength) * kFs);
      if (std::min(e, len) - std::min(b, len) < kLenSamples) continue;      // the double arithmetic left it one sample short
      offs.push_back((int64_t)base + b);
      ++scored[c];
    }
  }
  const size_t nw = offs.size();
  raw.assign(nw * 4, std::nanf(""));
  if (!nw) return PFHIP_OK;
  size_t max_floats = h->net[0].max_floats;
  if (h->has_p808) max_floats = std::max(max_floats, h->net[1].max_floats);
  const size_t slab = std::max<size_t>(1, std::min<size_t>({nw, (size_t)4096, h->workspace / (2 * max_floats * sizeof(float))}));
  DevMem d_pcm, d_off, d_a, d_b, d_out, d_max;
  HIP_TRY(d_pcm.upload(host.data(), host.size() * sizeof(Sample)));
  HIP_TRY(d_off.upload(offs.data(), nw * sizeof(int64_t)));
  HIP_TRY(d_a.alloc(slab * max_floats * sizeof(float)));
  HIP_TRY(d_b.alloc(slab * max_floats * sizeof(float)));
  HIP_TRY(d_out.alloc(nw * 4 * sizeof(float)));
  HIP_TRY(d_max.alloc(slab * sizeof(unsigned)));
  std::vector<float> o3(nw * 3), o1(nw);
  for (size_t i = 0; i < nw; i += slab) {
    const int n = (int)std::min(slab, nw - i);
    // the front end writes into b, the first convolution into a
    bool ok = pfhip::launch_dnsmos_logpow(d_pcm.as<Sample>(), d_off.as<int64_t>() + i, n, h->stft_tab, kFrames, h->floor_v, h->denom, d_b.f(),
                                          h->stream) &&
              run_net(h, h->net[0], d_b.f(), d_a.f(), d_b.f(), n, d_out.f() + i * 3);
    if (ok && h->has_p808)
      ok = pfhip::launch_dnsmos_melspec(d_pcm.as<Sample>(), d_off.as<int64_t>() + i, n, h->mel_tab, h->mel_T, d_b.f(), d_max.as<unsigned>(),
                                        h->stream) &&
           run_net(h, h->net[1], d_b.f(), d_a.f(), d_b.f(), n, d_out.f() + nw * 3 + i);
    if (!ok) return fail(PFHIP_ERR_UNSUPPORTED, "a DNSMOS kernel refused its launch");
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(o3.data(), d_out.f(), nw * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (h->has_p808) HIP_TRY(hipMemcpyAsync(o1.data(), d_out.f() + nw * 3, nw * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < nw; ++i) {
    if (h->has_p808) raw[4 * i] = o1[i];
    raw[4 * i + 1] = o3[3 * i];
    raw[4 * i + 2] = o3[3 * i + 1];
    raw[4 * i + 3] = o3[3 * i + 2];
  }
  return PFHIP_OK;
}

template <typename Sample>
pfhip_status score(pfhip_mos* h, const Sample* const* pcm, const int64_t* n_samples, int n_clips, int personalized, pfhip_mos_result* res) {
  last_error().clear();
  if (n_clips > 0 && !res) return fail(PFHIP_ERR_ARG, "null argument");
  std::vector<int> hops, scored;
  std::vector<float> raw;
  const pfhip_status st = score_windows(h, pcm, n_samples, n_clips, hops, scored, raw);
  if (st) return st;
  const int np = personalized ? 4 : 3;
  const double *cs = personalized ? kSigP : kSig, *cb = personalized ? kBakP : kBak, *co = personalized ? kOvrP : kOvr;
  size_t at = 0;
  for (int c = 0; c < n_clips; ++c) {
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < scored[c]; ++k, ++at) {
      const double p = raw[4 * at], sg = raw[4 * at + 1], bk = raw[4 * at + 2], ov = raw[4 * at + 3];
      s[0] += p; s[1] += sg; s[2] += bk; s[3] += ov;
      s[4] += polyval(cs, np, sg); s[5] += polyval(cb, np, bk); s[6] += polyval(co, np, ov);
    }
    const double n = scored[c] ? (double)scored[c] : std::nan("");
    res[c].num_hops = hops[c];
    res[c].n_scored = scored[c];
    res[c].p808 = s[0] / n; res[c].sig_raw = s[1] / n; res[c].bak_raw = s[2] / n; res[c].ovr_raw = s[3] / n;
    res[c].sig = s[4] / n; res[c].bak = s[5] / n; res[c].ovr = s[6] / n;
  }
  return PFHIP_OK;
}

template <typename Sample>
pfhip_status windows_out(pfhip_mos* h, const Sample* const* pcm, const int64_t* n_samples, int n_clips, int32_t* num_hops, int32_t* n_scored,
                         float* raw_out, size_t cap_windows, size_t* n_windows) {
  last_error().clear();
  if (!n_windows || (n_clips > 0 && (!num_hops || !n_scored))) return fail(PFHIP_ERR_ARG, "null argument");
  std::vector<int> hops, scored;
  std::vector<float> raw;
  const pfhip_status st = score_windows(h, pcm, n_samples, n_clips, hops, scored, raw);
  if (st) return st;
  for (int c = 0; c < n_clips; ++c) { num_hops[c] = hops[c]; n_scored[c] = scored[c]; }
  *n_windows = raw.size() / 4;
  if (*n_windows > cap_windows || (*n_windows && !raw_out)) return fail(PFHIP_ERR_CAPACITY, "raw holds fewer windows than were scored");
  if (!raw.empty()) std::memcpy(raw_out, raw.data(), raw.size() * sizeof(float));
  return PFHIP_OK;
}

}  // namespace

extern "C" {

pfhip_status pfhip_mos_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device, pfhip_mos** out) {
  last_error().clear();
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
  const pfhip::JValue* jk = jc->get("kind");
  if (!jk || jk->kind != pfhip::JValue::STR || jk->str != "dnsmos") return fail(PFHIP_ERR_FORMAT, "the container's kind is not \"dnsmos\"");
  std::unique_ptr<pfhip_mos> p(new pfhip_mos);
  p->device = device;
  p->has_p808 = jc->number("has_p808", 0) != 0;
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  const float* hb = static_cast<const float*>(blob);
  auto get = [&](const std::string& name, const std::vector<int>& shape, const float** ptr) -> bool {
    const pfhip::JValue* t = jt->get(name);
    if (!t) { last_error() = "missing tensor " + name; return false; }
    const pfhip::JValue* sh = t->get("shape");
    const pfhip::JValue* of = t->get("offset");
    if (!sh || !of || sh->arr.size() != shape.size()) { last_error() = "tensor " + name + " malformed"; return false; }
    size_t n = 1;
    for (size_t i = 0; i < shape.size(); ++i) {
      if ((int)sh->arr[i].num != shape[i]) { last_error() = "tensor " + name + " has unexpected shape"; return false; }
      n *= (size_t)shape[i];
    }
    const double offd = of->num;
    if (!(offd >= 0) || offd > (double)blob_bytes) { last_error() = "tensor " + name + " out of blob"; return false; }
    const size_t off = (size_t)offd;
    if (off % 4 || off + n * 4 > blob_bytes) { last_error() = "tensor " + name + " out of blob"; return false; }
    *ptr = hb + off / 4;
    return true;
  };
  auto dev_copy = [&](const float* src, size_t n, const float** dst) -> pfhip_status {
    DevMem mem;
    HIP_TRY(mem.upload(src, n * 4));
    *dst = mem.f();
    p->owned.push_back(std::move(mem));
    return PFHIP_OK;
  };
  pfhip_status st;
  for (int k = 0; k < (p->has_p808 ? 2 : 1); ++k) {
    const std::string pre = k ? "p808" : "primary";
    MosNet& net = p->net[k];
    net.H0 = kFrames;
    net.W0 = k ? pfhip::kDnsmosMels : kBins;
    const pfhip::JValue* jv = jc->get(pre + "_convs");
    const pfhip::JValue* jd = jc->get(pre + "_dense");
    if (!jv || jv->kind != pfhip::JValue::ARR || jv->arr.empty() || jv->arr.size() % 3 || jv->arr.size() > 3 * 64 || !jd ||
        jd->kind != pfhip::JValue::ARR || jd->arr.size() != 6)
      return fail(PFHIP_ERR_FORMAT, "config needs " + pre + "_convs (triples) and " + pre + "_dense (three pairs)");
    int H = net.H0, W = net.W0, prev = 1;
    for (size_t i = 0; i < jv->arr.size() / 3; ++i) {
      ConvLayer c;
      c.cout = (int)jv->arr[3 * i].num; c.cin = (int)jv->arr[3 * i + 1].num; c.pool = jv->arr[3 * i + 2].num != 0;
      const std::string name = pre + ".conv" + std::to_string(i);
      if (c.cin != prev || c.cout < 1 || c.cout > 4096 || (c.cin != 1 && !(c.cin == 32 || (c.cin >= 64 && c.cin % 64 == 0 && c.cin <= 4096))) ||
          (c.cin != 1 && c.cout != 32 && c.cout != 64) || c.cout % 4)
        return fail(PFHIP_ERR_UNSUPPORTED, name + ": the convolution kernels take Cin 1, 32 or a multiple of 64 following the layer before, "
                                                  "and behind the first layer Cout 32 or 64 (got " + std::to_string(c.cin) + " -> " +
                                                  std::to_string(c.cout) + ")");
      const float *w = nullptr, *b = nullptr;
      if (!get(name + ".w", {c.cout, c.cin, 3, 3}, &w) || !get(name + ".b", {c.cout}, &b)) return PFHIP_ERR_FORMAT;
      const size_t nwts = (size_t)c.cout * c.cin * 9;
      float mx = 0.f;
      for (size_t j = 0; j < nwts; ++j) {
        if (!std::isfinite(w[j])) return fail(PFHIP_ERR_UNSUPPORTED, name + ".w holds a value that is not finite");
        mx = std::max(mx, std::fabs(w[j]));
      }
      if ((st = dev_copy(b, c.cout, &c.b))) return st;
      const float* dw = nullptr;
      if ((st = dev_copy(w, nwts, &dw))) return st;
      if (c.cin == 1) {
        c.w = dw;
      } else {
        // the fp16 two-plane domain of the weights, asserted once: max |w| * scale <= 32768
        c.scale = pfhip::best_w_scale(mx);
        if (!(mx * c.scale <= 32768.0f)) return fail(PFHIP_ERR_UNSUPPORTED, name + ".w leaves the fp16 two-plane range (max |w| " + std::to_string(mx) + ")");
        DevMem hi, lo;
        HIP_TRY(hi.alloc(pfhip::conv3x3_plane_bytes(c.cin, c.cout)));
        HIP_TRY(lo.alloc(pfhip::conv3x3_plane_bytes(c.cin, c.cout)));
        if (!pfhip::launch_conv3x3_pack(dw, c.cin, c.cout, c.scale, hi.p, lo.p, p->stream)) return fail(PFHIP_ERR_UNSUPPORTED, name + ": cannot pack");
        HIP_TRY(hipStreamSynchronize(p->stream));
        c.hi = hi.p; c.lo = lo.p;
        p->owned.push_back(std::move(hi));
        p->owned.push_back(std::move(lo));
      }
      net.max_floats = std::max(net.max_floats, (size_t)H * W * c.cin);
      if (c.pool) { H /= 2; W /= 2; }
      if (H < 1 || W < 1) return fail(PFHIP_ERR_UNSUPPORTED, name + ": nothing is left to pool");
      net.max_floats = std::max(net.max_floats, (size_t)H * W * c.cout);
      prev = c.cout;
      net.convs.push_back(c);
    }
    for (int i = 0; i < 3; ++i) {
      net.din[i] = (int)jd->arr[2 * i].num; net.dout[i] = (int)jd->arr[2 * i + 1].num;
      if (net.din[i] != prev || net.din[i] < 1 || net.din[i] > 256 || net.dout[i] < 1 || net.dout[i] > 256)
        return fail(PFHIP_ERR_UNSUPPORTED, pre + ".dense" + std::to_string(i) + ": widths must chain and stay within 256");
      const float *w = nullptr, *b = nullptr;
      const std::string name = pre + ".dense" + std::to_string(i);
      if (!get(name + ".w", {net.din[i], net.dout[i]}, &w) || !get(name + ".b", {net.dout[i]}, &b)) return PFHIP_ERR_FORMAT;
      if ((st = dev_copy(w, (size_t)net.din[i] * net.dout[i], &net.dw[i])) || (st = dev_copy(b, net.dout[i], &net.db[i]))) return st;
      prev = net.dout[i];
    }
    if (prev != (k ? 1 : 3)) return fail(PFHIP_ERR_UNSUPPORTED, pre + ": the head must have " + (k ? "one output" : "three outputs"));
  }
  {
    const float *wr = nullptr, *wi = nullptr, *cs = nullptr;
    if (!get("primary.stft_real", {161, 320}, &wr) || !get("primary.stft_imag", {161, 320}, &wi) || !get("primary.consts", {3}, &cs))
      return PFHIP_ERR_FORMAT;
    // (floor, power, denom): the graph's Pow exponent is 2.0 and the kernel squares
    if (cs[1] != 2.0f || !(cs[2] != 0.f) || !std::isfinite(cs[0]) || !std::isfinite(cs[2]))
      return fail(PFHIP_ERR_UNSUPPORTED, "the front end's constants: pow/y must be 2 and truediv/y finite and not 0");
    p->floor_v = cs[0];
    p->denom = cs[2];
    std::vector<float> tab((size_t)320 * 2 * pfhip::kDnsmosBinStride);
    pfhip::dnsmos_stft_table(wr, wi, tab.data());
    if ((st = dev_copy(tab.data(), tab.size(), &p->stft_tab))) return st;
  }
  if (p->has_p808) {
    std::vector<float> tab((size_t)pfhip::kDnsmosFft * 2 * pfhip::kDnsmosBinStride), melT((size_t)kBins * pfhip::kDnsmosMels);
    pfhip::dnsmos_mel_tables(tab.data(), melT.data());
    if ((st = dev_copy(tab.data(), tab.size(), &p->mel_tab)) || (st = dev_copy(melT.data(), melT.size(), &p->mel_T))) return st;
  }
  *out = p.release();
  return PFHIP_OK;
}

pfhip_status pfhip_mos_create_from_files(const char* primary_onnx, const char* p808_onnx_or_null, int device, pfhip_mos** out) {
  last_error().clear();
  if (!primary_onnx || !out) return fail(PFHIP_ERR_ARG, "null argument");
  pfhip_files::Container c;
  try {
    pfhip_files::load_dnsmos(primary_onnx, p808_onnx_or_null ? p808_onnx_or_null : "", c);
  } catch (const std::exception& e) {
    return fail(PFHIP_ERR_FORMAT, e.what());
  }
  return pfhip_mos_create_from_memory(c.blob.data(), c.blob.size() * sizeof(float), c.manifest.c_str(), device, out);
}

void pfhip_mos_destroy(pfhip_mos* h) { delete h; }

pfhip_status pfhip_mos_set_workspace(pfhip_mos* h, size_t bytes) {
  if (!h) return fail(PFHIP_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->workspace = bytes;
  return PFHIP_OK;
}

pfhip_status pfhip_mos_score(pfhip_mos* h, const float* const* pcm, const int64_t* n_samples, int n_clips, int personalized,
                             pfhip_mos_result* results) {
  return score(h, pcm, n_samples, n_clips, personalized, results);
}
pfhip_status pfhip_mos_score_s16(pfhip_mos* h, const int16_t* const* pcm, const int64_t* n_samples, int n_clips, int personalized,
                                 pfhip_mos_result* results) {
  return score(h, pcm, n_samples, n_clips, personalized, results);
}
pfhip_status pfhip_mos_score_windows(pfhip_mos* h, const float* const* pcm, const int64_t* n_samples, int n_clips, int32_t* num_hops,
                                     int32_t* n_scored, float* raw, size_t cap_windows, size_t* n_windows) {
  return windows_out(h, pcm, n_samples, n_clips, num_hops, n_scored, raw, cap_windows, n_windows);
}
pfhip_status pfhip_mos_score_windows_s16(pfhip_mos* h, const int16_t* const* pcm, const int64_t* n_samples, int n_clips, int32_t* num_hops,
                                         int32_t* n_scored, float* raw, size_t cap_windows, size_t* n_windows) {
  return windows_out(h, pcm, n_samples, n_clips, num_hops, n_scored, raw, cap_windows, n_windows);
}

}  // extern "C"
