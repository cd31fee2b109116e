// FSMN-VAD forward on MI355X — the C ABI's pfhip_vad_* family.
// Replaces FsmnVad::FbankKaldi + LfrCmvn + Forward (onnxruntime/src/fsmn-vad.cpp:137-152, 198-238, 72-135): PCM ->
// frame scores [T, 248] with the four [128 x 19] FSMN caches carried in HBM.  The network is causal, so a whole
// file goes through in ONE pass of ~12 launches instead of the reference's 1-s slices (600 Runs per 10 minutes,
// onnxruntime/src/audio.cpp:1183-1196); slice-wise calls give the same scores because the caches carry over.
// Linear layers run on the same fp32 MFMA GEMM kernels as the ASR model; their odd widths (140, 250, 248) are
// zero-padded once at load ([N up to 128][K up to 32]) so that pad outputs are exact zeros.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>

#include "internal.h"
#include "json_min.h"

using namespace pfhip_impl;

struct pfhip_vad {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int n_mels = 80, lfr_m = 5, lfr_n = 1, input_dim = 400, proj = 128, lorder = 20, layers = 4, n_out = 248, linear = 250;
  FrontendTables ft;
  DevMem cmvn_mean, cmvn_istd;
  PackedLin in1, in2, out1, out2;
  std::vector<PackedLin> blk_linear, blk_affine;
  std::vector<DevMem> fsmn_w;
  Buf pcm, fb, feats, a, b, p, f, probs, sil, meta, cache[2], segs, fbk, ops;
  int cache_cur = 0;
  int* h_pin = nullptr;
  // pinned staging for the online path's PCM (grown on demand); h_wave(n) returns a buffer of at least n floats
  float* h_wave_buf = nullptr; size_t h_wave_cap = 0;
  // merging of concurrent pfhip_vad_stream_infer callers (pfhip_set_vad_stream_batching)
  pfhip_impl::MergeQueue<struct VadReq> mq;
  int q_wait_us = 0, q_max = 1;
  std::atomic<int> live_streams{0};
  // the offline forward in company (pfhip_vad_forward_sil_batch, pfhip_set_vad_batching): frame energies, the zero block that stands
  // for a fresh file's caches, whether non-final calls have left state in cache[] since the last reset, the callers' queue
  Buf eng, zcache;
  std::atomic<bool> carried{false};
  pfhip_impl::MergeQueue<struct VadFileReq> fq;
  int fq_wait_us = 0, fq_max = 1;                 // guarded by fq.mu
  long long fq_passes = 0, fq_files = 0; int fq_max_seen = 0;      // guarded by mu: packed passes, their files, the fullest pass
  float* h_wave(size_t n) {
    if (n > h_wave_cap) {
      if (h_wave_buf) (void)hipHostFree(h_wave_buf);
      h_wave_buf = nullptr; h_wave_cap = 0;
      const size_t cap = std::max<size_t>(n, 70000);
      if (hipHostMalloc((void**)&h_wave_buf, cap * 4, hipHostMallocDefault) == hipSuccess) h_wave_cap = cap;
    }
    return h_wave_buf;
  }
  // the device set and idle before any member gives its memory back (a create that returns early comes through here too)
  ~pfhip_vad() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (h_pin) (void)hipHostFree(h_pin);
    if (h_wave_buf) (void)hipHostFree(h_wave_buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

void lin_gemm(hipStream_t s, const PackedLin& l, const float* A, int lda, float* C, int ldc, int M, bool relu) {
  pfhip_impl::lin_gemm(s, l, A, lda, C, ldc, nullptr, 0, nullptr, 0, M, relu);
}

}  // namespace

extern "C" {

pfhip_status pfhip_vad_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                                          pfhip_vad** out) {
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
  std::unique_ptr<pfhip_vad> v(new pfhip_vad);
  v->device = device;
  v->n_mels = (int)jc->number("n_mels", 80);
  v->lfr_m = (int)jc->number("lfr_m", 5);
  v->lfr_n = (int)jc->number("lfr_n", 1);
  v->input_dim = (int)jc->number("input_dim", 400);
  v->proj = (int)jc->number("proj", 128);
  v->lorder = (int)jc->number("lorder", 20);
  v->layers = (int)jc->number("layers", 4);
  v->n_out = (int)jc->number("n_out", 248);
  v->linear = (int)jc->number("linear", 250);
  const int affine = (int)jc->number("affine", 140), out_affine = (int)jc->number("out_affine", 140);
  if (v->n_mels != 80 || v->input_dim != v->n_mels * v->lfr_m || v->lorder != 20 || v->proj % 4 || v->layers < 1 ||
      v->layers > 16)
    return fail(PFHIP_ERR_UNSUPPORTED, "FSMN-VAD kernels need 80 mels, left order 20");
  const float* hb = static_cast<const float*>(blob);
  auto get = [&](const std::string& name, std::vector<int> shape, const float** p) -> bool {
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
    const size_t off = (size_t)of->num;
    if (off % 4 || off + n * 4 > blob_bytes) { last_error() = "tensor " + name + " out of blob"; return false; }
    *p = hb + off / 4;
    return true;
  };
  auto lin = [&](const std::string& name, int N, int K, bool bias, PackedLin* l) -> pfhip_status {
    const float *w = nullptr, *b = nullptr;
    if (!get(name + ".w", {N, K}, &w)) return PFHIP_ERR_FORMAT;
    if (bias && !get(name + ".b", {N}, &b)) return PFHIP_ERR_FORMAT;
    return pack_linear(w, b, N, K, l);
  };
  pfhip_status st;
  const float *mean = nullptr, *istd = nullptr;
  if (!get("cmvn.mean", {v->input_dim}, &mean) || !get("cmvn.istd", {v->input_dim}, &istd)) return PFHIP_ERR_FORMAT;
  HIP_TRY(v->cmvn_mean.upload(mean, (size_t)v->input_dim * 4));
  HIP_TRY(v->cmvn_istd.upload(istd, (size_t)v->input_dim * 4));
  if ((st = lin("in1", affine, v->input_dim, true, &v->in1)) || (st = lin("in2", v->linear, affine, true, &v->in2))) return st;
  v->blk_linear.resize(v->layers); v->blk_affine.resize(v->layers); v->fsmn_w.resize(v->layers);
  for (int i = 0; i < v->layers; ++i) {
    const std::string p = "blk." + std::to_string(i) + ".";
    if ((st = lin(p + "linear", v->proj, v->linear, false, &v->blk_linear[i])) ||
        (st = lin(p + "affine", v->linear, v->proj, true, &v->blk_affine[i])))
      return st;
    const float* fw = nullptr;
    if (!get(p + "fsmn.w", {v->proj, v->lorder}, &fw)) return PFHIP_ERR_FORMAT;
    HIP_TRY(v->fsmn_w[i].upload(fw, (size_t)v->proj * v->lorder * 4));
  }
  if ((st = lin("out1", out_affine, v->linear, true, &v->out1)) || (st = lin("out2", v->n_out, out_affine, true, &v->out2))) return st;
  if ((st = build_frontend_tables(v->n_mels, 16000, &v->ft))) return st;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(v->cache[i].ensure((size_t)v->layers * 19 * v->proj * 4));
    HIP_TRY(hipMemset(v->cache[i].p, 0, (size_t)v->layers * 19 * v->proj * 4));
  }
  HIP_TRY(v->meta.ensure(256));
  HIP_TRY(hipHostMalloc((void**)&v->h_pin, 256, hipHostMallocDefault));
  HIP_TRY(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
  *out = v.release();
  return PFHIP_OK;
}

void pfhip_vad_destroy(pfhip_vad* v) { delete v; }

pfhip_status pfhip_vad_reset(pfhip_vad* v) {
  last_error().clear();
  if (!v) return fail(PFHIP_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(v->mu);
  HIP_TRY(hipSetDevice(v->device));
  for (int i = 0; i < 2; ++i) HIP_TRY(hipMemsetAsync(v->cache[i].p, 0, (size_t)v->layers * 19 * v->proj * 4, v->stream));
  HIP_TRY(hipStreamSynchronize(v->stream));
  v->carried = false;
  return PFHIP_OK;
}

int pfhip_vad_num_classes(const pfhip_vad* v) { return v ? v->n_out : 0; }

// The FSMN-VAD network on the T packed rows waiting in v->feats (caller holds v->mu and has sized the workspace); scores in
// v->probs.  d_segs: one VadSeg per connection (its rows and caches), max_T = longest segment.
static void vad_network(pfhip_vad* v, hipStream_t s, int T, const pfhip::VadSeg* d_segs, int B, int max_T) {
  lin_gemm(s, v->in1, v->feats.f(), v->in1.Kp, v->a.f(), 256, T, false);
  lin_gemm(s, v->in2, v->a.f(), 256, v->b.f(), 256, T, true);
  for (int i = 0; i < v->layers; ++i) {
    lin_gemm(s, v->blk_linear[i], v->b.f(), 256, v->p.f(), 128, T, false);
    pfhip::launch_fsmn_causal20(v->p.f(), 128, v->fsmn_w[i].f(), d_segs, B, max_T, i, v->f.f(), 128, v->proj, s);
    lin_gemm(s, v->blk_affine[i], v->f.f(), 128, v->b.f(), 256, T, true);
  }
  lin_gemm(s, v->out1, v->b.f(), 256, v->a.f(), 256, T, false);
  lin_gemm(s, v->out2, v->a.f(), 256, v->b.f(), 256, T, false);
  pfhip::launch_softmax_rows(v->b.f(), 256, T, v->n_out, v->probs.f(), v->sil.f(), s);
}

static pfhip_status vad_workspace(pfhip_vad* v, int T) {
  const int Tp = round_up(T, 128);
  HIP_TRY(v->feats.ensure((size_t)Tp * v->in1.Kp * 4));
  HIP_TRY(v->a.ensure((size_t)Tp * 256 * 4));
  HIP_TRY(v->b.ensure((size_t)Tp * 256 * 4));
  HIP_TRY(v->p.ensure((size_t)Tp * 128 * 4));
  HIP_TRY(v->f.ensure((size_t)Tp * 128 * 4));
  HIP_TRY(v->probs.ensure((size_t)T * v->n_out * 4));
  HIP_TRY(v->sil.ensure((size_t)T * 4));
  if (v->in1.Np > 256 || v->in2.Np > 256 || v->out1.Np > 256 || v->out2.Np > 256 || v->proj > 128)
    return fail(PFHIP_ERR_UNSUPPORTED, "FSMN-VAD layer wider than the workspace");
  return PFHIP_OK;
}

static pfhip_status vad_forward_impl(pfhip_vad* v, PcmView pcm, int n_samples, int is_final, float* probs,
                                     size_t cap_floats, int* n_frames, bool sil_only, float* energy = nullptr, size_t cap_energy = 0,
                                     int* n_energy = nullptr);

pfhip_status pfhip_vad_forward(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* probs,
                               size_t cap_floats, int* n_frames) {
  return vad_forward_impl(v, PcmView{pcm, false}, n_samples, is_final, probs, cap_floats, n_frames, false);
}

pfhip_status pfhip_vad_forward_sil(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* sil_prob,
                                   size_t cap_floats, int* n_frames) {
  return vad_forward_impl(v, PcmView{pcm, false}, n_samples, is_final, sil_prob, cap_floats, n_frames, true);
}
// the same from 16-bit PCM (the bytes Audio::LoadPcmwav, audio.cpp:787-819, divides by 32768 on the host): copied as they are,
// converted by the fbank kernel's loads
pfhip_status pfhip_vad_forward_sil_s16(pfhip_vad* v, const int16_t* pcm, int n_samples, int is_final, float* sil_prob,
                                       size_t cap_floats, int* n_frames) {
  return vad_forward_impl(v, PcmView{pcm, true}, n_samples, is_final, sil_prob, cap_floats, n_frames, true);
}

// n_energy != nullptr: the call also returns the frame energies of its samples (one per fbank frame), computed from the PCM the
// fbank kernel has just read; the launches that produce the scores are the same with and without.
static pfhip_status vad_forward_impl(pfhip_vad* v, PcmView pcm, int n_samples, int is_final, float* probs,
                                     size_t cap_floats, int* n_frames, bool sil_only, float* energy, size_t cap_energy,
                                     int* n_energy) {
  last_error().clear();
  if (!v || n_samples < 0 || (n_samples > 0 && !pcm.p) || !n_frames) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(v->mu);
  HIP_TRY(hipSetDevice(v->device));
  hipStream_t s = v->stream;
  const int F = n_samples < 400 ? 0 : 1 + (n_samples - 400) / 160;
  const int T = (F + v->lfr_n - 1) / v->lfr_n;               // fsmn-vad.cpp:202
  *n_frames = T;
  if (n_energy) *n_energy = F;
  if (T == 0) return PFHIP_OK;                                // fsmn-vad.cpp:245-247
  if ((size_t)T * (sil_only ? 1 : v->n_out) > cap_floats && probs) return fail(PFHIP_ERR_CAPACITY, "probs buffer too small");
  if (n_energy && energy && (size_t)F > cap_energy) return fail(PFHIP_ERR_CAPACITY, "energy buffer too small (n_energy holds the count)");
  if (n_energy) HIP_TRY(v->eng.ensure((size_t)F * 4));
  const int Tp = round_up(T, 128);
  HIP_TRY(v->pcm.ensure((size_t)n_samples * pcm.sample_bytes()));      // the one workspace, in floats or in shorts
  HIP_TRY(v->fb.ensure((size_t)F * 80 * 4));
  HIP_TRY(v->feats.ensure((size_t)Tp * v->in1.Kp * 4));
  HIP_TRY(v->a.ensure((size_t)Tp * 256 * 4));
  HIP_TRY(v->b.ensure((size_t)Tp * 256 * 4));
  HIP_TRY(v->p.ensure((size_t)Tp * 128 * 4));
  HIP_TRY(v->f.ensure((size_t)Tp * 128 * 4));
  HIP_TRY(v->probs.ensure((size_t)T * v->n_out * 4));
  HIP_TRY(v->sil.ensure((size_t)T * 4));
  if (v->in1.Np > 256 || v->in2.Np > 256 || v->out1.Np > 256 || v->out2.Np > 256 || v->proj > 128)
    return fail(PFHIP_ERR_UNSUPPORTED, "FSMN-VAD layer wider than the workspace");
  HIP_TRY(hipMemcpyAsync(v->pcm.p, pcm.p, (size_t)n_samples * pcm.sample_bytes(), hipMemcpyHostToDevice, s));
  {
    int64_t* h64 = reinterpret_cast<int64_t*>(v->h_pin);
    h64[0] = 0;
    int* hm = v->h_pin + 2;
    hm[0] = 0; hm[1] = F; hm[2] = F;
    HIP_TRY(hipMemcpyAsync(v->meta.p, v->h_pin, 32, hipMemcpyHostToDevice, s));
  }
  const pfhip::FbankTables tb = v->ft.fbank(v->cmvn_mean.f(), v->cmvn_istd.f());
  if (pcm.s16)
    pfhip::launch_fbank_frames(static_cast<const int16_t*>(v->pcm.p), reinterpret_cast<int64_t*>(v->meta.p), v->meta.i() + 2,
                               v->meta.i() + 4, F, tb, v->fb.f(), s);
  else
    pfhip::launch_fbank_frames(v->pcm.f(), reinterpret_cast<int64_t*>(v->meta.p), v->meta.i() + 2, v->meta.i() + 4, F, tb,
                               v->fb.f(), s);
  pfhip::launch_lfr_cmvn(v->fb.f(), F, T, v->lfr_m, v->lfr_n, v->n_mels, v->cmvn_mean.f(), v->cmvn_istd.f(), v->feats.f(), v->in1.Kp, s);
  {
    pfhip::VadSeg* hs = reinterpret_cast<pfhip::VadSeg*>(v->h_pin + 16);
    *hs = pfhip::VadSeg{v->cache[v->cache_cur].f(), is_final ? nullptr : v->cache[v->cache_cur ^ 1].f(), 0, T};
    HIP_TRY(v->segs.ensure(sizeof(pfhip::VadSeg)));
    HIP_TRY(hipMemcpyAsync(v->segs.p, hs, sizeof(pfhip::VadSeg), hipMemcpyHostToDevice, s));
    vad_network(v, s, T, static_cast<const pfhip::VadSeg*>(v->segs.p), 1, T);
  }
  if (!is_final) { v->cache_cur ^= 1; v->carried = true; }      // fsmn-vad.cpp:129-134: caches kept only if not final
  if (n_energy) {
    const int64_t* so = reinterpret_cast<int64_t*>(v->meta.p);
    const bool ok = pcm.s16 ? pfhip::launch_frame_energy(static_cast<const int16_t*>(v->pcm.p), so, v->meta.i() + 2, v->meta.i() + 4, 1, F,
                                                         400, 160, v->eng.f(), s)
                            : pfhip::launch_frame_energy(v->pcm.f(), so, v->meta.i() + 2, v->meta.i() + 4, 1, F, 400, 160, v->eng.f(), s);
    if (!ok) return fail(PFHIP_ERR_UNSUPPORTED, "frame energy launch refused");
    if (energy) HIP_TRY(hipMemcpyAsync(energy, v->eng.p, (size_t)F * 4, hipMemcpyDeviceToHost, s));
  }
  if (probs && !sil_only) HIP_TRY(hipMemcpyAsync(probs, v->probs.p, (size_t)T * v->n_out * 4, hipMemcpyDeviceToHost, s));
  if (probs && sil_only)        // column 0 of the [T, n_out] score matrix
    HIP_TRY(hipMemcpyAsync(probs, v->sil.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return PFHIP_OK;
}


}  // extern "C"

// ---- complete files in company ----------------------------------------------------------------------------------------------
// One caller's file of a packed pass.  Every file is scored as an is_final call on a fresh object: zeroed caches in, nothing
// carried out (fsmn-vad.cpp:129-134), so the handle's own caches are neither read nor written.
struct VadFileReq : pfhip_impl::MergeReqBase {
  pfhip_impl::PcmView pcm; int n;
  float* sil; size_t cap; int* nf; float* energy; size_t cap_e; int* ne;
  pfhip_status st = PFHIP_OK; std::string err;
};

namespace {

// All files of one sample format.  Status per file (a file whose buffers are too small gets its counts and nothing else, the
// others are served); a failure of the shared pass fails every file.  Returns the first non-OK status.
pfhip_status vad_forward_files(pfhip_vad* v, const std::vector<VadFileReq*>& files) {
  last_error().clear();
  const int B = (int)files.size();
  const bool s16 = B > 0 && files[0]->pcm.s16;
  const size_t sb = s16 ? 2 : 4;
  auto fail_all = [&](pfhip_status st) {
    for (VadFileReq* r : files) { r->st = st; r->err = last_error(); }
    return st;
  };
  std::lock_guard<std::mutex> lk(v->mu);
  if (hipSetDevice(v->device) != hipSuccess) return fail_all(fail(PFHIP_ERR_HIP, "hipSetDevice failed"));
  hipStream_t s = v->stream;
  // ---- plan: the files that have frames (and room for their results) take samples, frames and rows, back to back ----------------
  struct Plan { VadFileReq* r; int F, T; size_t so; int fo, ro; };
  std::vector<Plan> plan;
  size_t n_samp = 0;
  int n_fr = 0, n_row = 0, max_T = 0;
  pfhip_status first = PFHIP_OK;
  std::string first_err;
  for (VadFileReq* r : files) {
    const int F = r->n < 400 ? 0 : 1 + (r->n - 400) / 160;
    const int T = (F + v->lfr_n - 1) / v->lfr_n;
    *r->nf = T; *r->ne = F;
    r->st = PFHIP_OK; r->err.clear();
    if (T == 0) continue;
    if ((r->sil && (size_t)T > r->cap) || (r->energy && (size_t)F > r->cap_e)) {
      r->st = fail(PFHIP_ERR_CAPACITY, "sil_prob or energy buffer too small (n_frames / n_energy hold the counts)");
      r->err = last_error();
      if (!first) { first = r->st; first_err = r->err; }
      continue;
    }
    plan.push_back(Plan{r, F, T, n_samp, n_fr, n_row});
    n_samp += (size_t)r->n; n_fr += F; n_row += T; max_T = std::max(max_T, T);
  }
  const int U = (int)plan.size();
  if (U > 0) {
    auto run = [&]() -> pfhip_status {
      const size_t cache_bytes = (size_t)v->layers * 19 * v->proj * 4;
      if (!v->zcache.p) {
        HIP_TRY(v->zcache.ensure(cache_bytes));
        HIP_TRY(hipMemsetAsync(v->zcache.p, 0, cache_bytes, s));
      }
      HIP_TRY(v->pcm.ensure(n_samp * sb + 16));
      HIP_TRY(v->fbk.ensure((size_t)n_fr * 80 * 4));
      HIP_TRY(v->eng.ensure((size_t)n_fr * 4));
      pfhip_status ws = vad_workspace(v, n_row);
      if (ws) return ws;
      // control block: sample_off [U] int64 | frame_off [U + 1] | nframes [U] | row_off [U] | VadSeg [U]; then the results
      const size_t o_fo = (size_t)U * 8, o_nf = o_fo + (size_t)(U + 1) * 4, o_ro = o_nf + (size_t)U * 4;
      const size_t o_seg = (o_ro + (size_t)U * 4 + 15) & ~(size_t)15;
      const size_t ctl = (o_seg + (size_t)U * sizeof(pfhip::VadSeg) + 63) & ~(size_t)63;
      float* hp_f = v->h_wave(ctl / 4 + (size_t)n_row + (size_t)n_fr + 16);
      if (!hp_f) return fail(PFHIP_ERR_HIP, "pinned staging allocation failed");
      char* hp = reinterpret_cast<char*>(hp_f);
      float* h_sil = reinterpret_cast<float*>(hp + ctl);
      float* h_eng = h_sil + n_row;
      HIP_TRY(v->ops.ensure(ctl));
      char* dp = static_cast<char*>(v->ops.p);
      int64_t* h_so = reinterpret_cast<int64_t*>(hp);
      int* h_fo = reinterpret_cast<int*>(hp + o_fo);
      int* h_nf = reinterpret_cast<int*>(hp + o_nf);
      int* h_ro = reinterpret_cast<int*>(hp + o_ro);
      pfhip::VadSeg* h_seg = reinterpret_cast<pfhip::VadSeg*>(hp + o_seg);
      for (int u = 0; u < U; ++u) {
        const Plan& pl = plan[u];
        h_so[u] = (int64_t)pl.so; h_fo[u] = pl.fo; h_nf[u] = pl.F; h_ro[u] = pl.ro;
        h_seg[u] = pfhip::VadSeg{v->zcache.f(), nullptr, pl.ro, pl.T};
        // the caller's samples go to the device as they are: no host copy, no conversion
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(v->pcm.p) + pl.so * sb, pl.r->pcm.p, (size_t)pl.r->n * sb, hipMemcpyHostToDevice, s));
      }
      h_fo[U] = n_fr;
      HIP_TRY(hipMemcpyAsync(dp, hp, ctl, hipMemcpyHostToDevice, s));
      const int64_t* d_so = reinterpret_cast<const int64_t*>(dp);
      const int *d_fo = reinterpret_cast<const int*>(dp + o_fo), *d_nf = reinterpret_cast<const int*>(dp + o_nf),
                *d_ro = reinterpret_cast<const int*>(dp + o_ro);
      const pfhip::FbankTables tb = v->ft.fbank(v->cmvn_mean.f(), v->cmvn_istd.f());
      bool ok;
      if (s16) {
        const int16_t* d_pcm = static_cast<const int16_t*>(v->pcm.p);
        pfhip::launch_fbank_frames_batch(d_pcm, d_so, d_fo, d_nf, U, n_fr, tb, v->fbk.f(), s);
        ok = pfhip::launch_frame_energy(d_pcm, d_so, d_fo, d_nf, U, n_fr, 400, 160, v->eng.f(), s);
      } else {
        pfhip::launch_fbank_frames_batch(v->pcm.f(), d_so, d_fo, d_nf, U, n_fr, tb, v->fbk.f(), s);
        ok = pfhip::launch_frame_energy(v->pcm.f(), d_so, d_fo, d_nf, U, n_fr, 400, 160, v->eng.f(), s);
      }
      if (!ok) return fail(PFHIP_ERR_UNSUPPORTED, "frame energy launch refused");
      pfhip::launch_lfr_cmvn_packed(v->fbk.f(), d_fo, d_nf, d_ro, U, max_T, v->lfr_m, v->lfr_n, v->n_mels, v->cmvn_mean.f(), v->cmvn_istd.f(),
                                    v->feats.f(), v->in1.Kp, s);
      vad_network(v, s, n_row, reinterpret_cast<const pfhip::VadSeg*>(dp + o_seg), U, max_T);
      HIP_TRY(hipMemcpyAsync(h_sil, v->sil.p, (size_t)n_row * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(h_eng, v->eng.p, (size_t)n_fr * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      HIP_TRY(hipGetLastError());
      for (const Plan& pl : plan) {
        if (pl.r->sil) std::memcpy(pl.r->sil, h_sil + pl.ro, (size_t)pl.T * 4);
        if (pl.r->energy) std::memcpy(pl.r->energy, h_eng + pl.fo, (size_t)pl.F * 4);
      }
      return PFHIP_OK;
    };
    const pfhip_status st = run();
    if (st) return fail_all(st);
    ++v->fq_passes; v->fq_files += U; v->fq_max_seen = std::max(v->fq_max_seen, U);
  }
  if (first) last_error() = first_err;
  return first;
}

template <typename Sample>
pfhip_status vad_forward_sil_batch_of(pfhip_vad* v, const Sample* const* pcm, const int* n_samples, int n_files, float* const* sil_prob,
                                      const size_t* cap_floats, int* n_frames, float* const* energy, const size_t* cap_energy,
                                      int* n_energy) {
  last_error().clear();
  if (!v || n_files <= 0 || !pcm || !n_samples || !sil_prob || !cap_floats || !n_frames || !energy || !cap_energy || !n_energy)
    return fail(PFHIP_ERR_ARG, "bad argument");
  std::vector<VadFileReq> reqs((size_t)n_files);
  std::vector<VadFileReq*> ptrs((size_t)n_files);
  for (int i = 0; i < n_files; ++i) {
    if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm[i])) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    VadFileReq& r = reqs[i];
    r.pcm = PcmView{pcm[i], sizeof(Sample) == 2}; r.n = n_samples[i];
    r.sil = sil_prob[i]; r.cap = cap_floats[i]; r.nf = &n_frames[i];
    r.energy = energy[i]; r.cap_e = cap_energy[i]; r.ne = &n_energy[i];
    ptrs[i] = &r;
  }
  return vad_forward_files(v, ptrs);
}

// pfhip_vad_forward_sil_energy[_s16]: a final call on a handle without carried caches IS a fresh file, so with
// pfhip_set_vad_batching on it joins the callers' queue and is scored in company; every other call runs alone as ever.
pfhip_status vad_forward_sil_energy_one(pfhip_vad* v, PcmView pcm, int n_samples, int is_final, float* sil_prob, size_t cap_floats,
                                        int* n_frames, float* energy, size_t cap_energy, int* n_energy) {
  if (!v || !n_frames || !n_energy || n_samples < 0 || (n_samples > 0 && !pcm.p)) { last_error().clear(); return fail(PFHIP_ERR_ARG, "bad argument"); }
  int wait_us, cap;
  { std::lock_guard<std::mutex> ql(v->fq.mu); wait_us = v->fq_wait_us; cap = v->fq_max; }
  if (!(is_final && wait_us > 0 && cap > 1 && !v->carried.load()))
    return vad_forward_impl(v, pcm, n_samples, is_final, sil_prob, cap_floats, n_frames, true, energy, cap_energy, n_energy);
  VadFileReq me;
  me.pcm = pcm; me.n = n_samples; me.sil = sil_prob; me.cap = cap_floats; me.nf = n_frames;
  me.energy = energy; me.cap_e = cap_energy; me.ne = n_energy;
  v->fq.submit(
      me, wait_us, [&](const std::deque<VadFileReq*>& q) { return (int)q.size() >= cap; },
      [&](std::deque<VadFileReq*>& q, std::vector<VadFileReq*>& take) {      // one sample format per pass: the leader's
        const bool s16 = q.front()->pcm.s16;
        std::deque<VadFileReq*> later;
        while (!q.empty()) {
          VadFileReq* r = q.front();
          q.pop_front();
          if ((int)take.size() < cap && r->pcm.s16 == s16) take.push_back(r); else later.push_back(r);
        }
        q.swap(later);
      },
      [&](std::vector<VadFileReq*>& take) { (void)vad_forward_files(v, take); }, /*fresh_no_wait=*/true);
  last_error() = me.err;
  return me.st;
}

}  // namespace

extern "C" {

pfhip_status pfhip_vad_forward_sil_energy(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* sil_prob,
                                          size_t cap_floats, int* n_frames, float* energy, size_t cap_energy, int* n_energy) {
  return vad_forward_sil_energy_one(v, PcmView{pcm, false}, n_samples, is_final, sil_prob, cap_floats, n_frames, energy, cap_energy, n_energy);
}
pfhip_status pfhip_vad_forward_sil_energy_s16(pfhip_vad* v, const int16_t* pcm, int n_samples, int is_final, float* sil_prob,
                                              size_t cap_floats, int* n_frames, float* energy, size_t cap_energy, int* n_energy) {
  return vad_forward_sil_energy_one(v, PcmView{pcm, true}, n_samples, is_final, sil_prob, cap_floats, n_frames, energy, cap_energy, n_energy);
}
pfhip_status pfhip_vad_forward_sil_batch(pfhip_vad* v, const float* const* pcm, const int* n_samples, int n_files, float* const* sil_prob,
                                         const size_t* cap_floats, int* n_frames, float* const* energy, const size_t* cap_energy,
                                         int* n_energy) {
  return vad_forward_sil_batch_of(v, pcm, n_samples, n_files, sil_prob, cap_floats, n_frames, energy, cap_energy, n_energy);
}
pfhip_status pfhip_vad_forward_sil_batch_s16(pfhip_vad* v, const int16_t* const* pcm, const int* n_samples, int n_files,
                                             float* const* sil_prob, const size_t* cap_floats, int* n_frames, float* const* energy,
                                             const size_t* cap_energy, int* n_energy) {
  return vad_forward_sil_batch_of(v, pcm, n_samples, n_files, sil_prob, cap_floats, n_frames, energy, cap_energy, n_energy);
}
pfhip_status pfhip_set_vad_batching(pfhip_vad* v, int wait_us, int max_files) {
  last_error().clear();
  if (!v || wait_us < 0 || max_files < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> ql(v->fq.mu);
  v->fq_wait_us = wait_us;
  v->fq_max = max_files;
  return PFHIP_OK;
}
pfhip_status pfhip_vad_batch_stats(pfhip_vad* v, long long* passes, long long* files, int* max_files) {
  last_error().clear();
  if (!v) return fail(PFHIP_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(v->mu);
  if (passes) *passes = v->fq_passes;
  if (files) *files = v->fq_files;
  if (max_files) *max_files = v->fq_max_seen;
  return PFHIP_OK;
}

// ---- FsmnVadOnline (onnxruntime/src/fsmn-vad-online.cpp): one object per connection -----------------------------------
// The online feature front end keeps three caches between calls: input_cache_ (samples after the last frame shift,
// :11-38), lfr_splice_cache_ (frames not yet consumed by a full LFR window, :48-70, here in HBM) and reserve_waveforms_
// (the samples that line up with the emitted rows, handed to the scorer for its dB computation, :45-68), plus the four
// network caches.  Host logic is transcribed statement by statement; arithmetic stays on the GPU (fbank, LFR, network).
struct pfhip_vad_stream {
  pfhip_vad* v = nullptr;
  std::vector<float> input_cache, reserve;
  int n_splice = 0;             // frames at the front of fb[fb_cur]
  Buf fb[2], cache[2];
  int fb_cur = 0, cache_cur = 0;
};

namespace {
constexpr int kVadMaxSamples = 64000;     // per call (4 s); the 2-pass server sends 9600, CutSplit one second
constexpr int kVadMaxFrames = 512;

pfhip_status vs_zero_caches(pfhip_vad_stream* vs, hipStream_t s) {
  pfhip_vad* v = vs->v;
  for (int i = 0; i < 2; ++i) HIP_TRY(hipMemsetAsync(vs->cache[i].p, 0, (size_t)v->layers * 19 * v->proj * 4, s));
  return PFHIP_OK;
}
}  // namespace

pfhip_status pfhip_vad_stream_create(pfhip_vad* v, pfhip_vad_stream** out) {
  last_error().clear();
  if (!v || !out) return fail(PFHIP_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(v->mu);
  HIP_TRY(hipSetDevice(v->device));
  std::unique_ptr<pfhip_vad_stream> vs(new pfhip_vad_stream);
  vs->v = v;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(vs->fb[i].ensure((size_t)kVadMaxFrames * 80 * 4));
    HIP_TRY(vs->cache[i].ensure((size_t)v->layers * 19 * v->proj * 4));
  }
  pfhip_status st = vs_zero_caches(vs.get(), v->stream);
  if (st) return st;
  HIP_TRY(hipStreamSynchronize(v->stream));
  ++v->live_streams;
  *out = vs.release();
  return PFHIP_OK;
}

void pfhip_vad_stream_destroy(pfhip_vad_stream* vs) {
  if (!vs) return;
  {
    std::lock_guard<std::mutex> lk(vs->v->mu);
    (void)hipSetDevice(vs->v->device);
    (void)hipStreamSynchronize(vs->v->stream);
    --vs->v->live_streams;
    delete vs;                // its buffers go back under the handle's lock, with the device set and the stream idle
  }
}

// Reset() + ResetCache() (fsmn-vad-online.cpp:160-163, fsmn-vad-online.h:59-63)
pfhip_status pfhip_vad_stream_reset(pfhip_vad_stream* vs) {
  last_error().clear();
  if (!vs) return fail(PFHIP_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(vs->v->mu);
  HIP_TRY(hipSetDevice(vs->v->device));
  vs->input_cache.clear(); vs->reserve.clear(); vs->n_splice = 0;
  pfhip_status st = vs_zero_caches(vs, vs->v->stream);
  if (st) return st;
  HIP_TRY(hipStreamSynchronize(vs->v->stream));
  return PFHIP_OK;
}

}  // extern "C"

namespace {

// One connection's share of a (batched) FsmnVadOnline::Infer: the host part of ExtractFeats runs first and leaves a plan,
// the device work of all connections is then issued as a handful of batched launches.
struct VadCall {
  pfhip_vad_stream* vs; PcmView pcm; int n_samples; bool fin;
  float* sil_prob; size_t cap_floats; int* n_frames; float* waves_out; size_t waves_cap; int* n_waves;
  // plan.  buf = this call's slice of the pinned sample staging: [reserve_waveforms_ | input_cache_ | new samples]
  float* buf = nullptr;
  size_t fb_off = 0, fb_len = 0;    // samples (relative to buf) whose frames are computed in this call
  size_t out_off = 0, out_len = 0;  // what the scorer gets
  size_t used = 0;
  int frame_number = 0, base = 0, n_rows = 0, Tin = 0, splice = 0;
  bool fresh = false, run_lfr = false;
  int row_off = 0;
};

// ExtractFeats (:40-88) on counters and sample ranges only; the one copy of the samples made here is the one into the
// staging buffer the device reads.  16-bit PCM becomes s / 32768.f (exact) during that copy: the caches, the waveform handed to the
// scorer (waves_out, whose decibel track needs floats) and the fbank launch stay f32 — bit for bit the f32 entry points.
pfhip_status vad_plan(VadCall& c) {
  pfhip_vad_stream* vs = c.vs;
  pfhip_vad* v = vs->v;
  const int fl = 400, fs = 160, m = v->lfr_m, n = v->lfr_n;
  const size_t r0 = vs->reserve.size(), ic = vs->input_cache.size();
  if (r0) std::memcpy(c.buf, vs->reserve.data(), r0 * 4);
  if (ic) std::memcpy(c.buf + r0, vs->input_cache.data(), ic * 4);
  pcm_to_f32(c.buf + r0 + ic, c.pcm, (size_t)c.n_samples);
  c.used = r0 + ic + (size_t)c.n_samples;
  const float* W = c.buf + r0;                              // `waves` = input_cache_ ++ new samples (:43-44)
  const int total = (int)(ic + (size_t)c.n_samples);
  c.frame_number = total >= fl ? (total - fl) / fs + 1 : 0;
  vs->input_cache.assign(W + (size_t)c.frame_number * fs, W + total);
  auto online_lfr = [&](int Tin) {                          // OnlineLfrCmvn (:90-133): counts only
    const int T_lrf = (int)std::ceil((Tin - (m - 1) / 2) / (float)n);
    int splice = T_lrf, n_out = 0;
    for (int i = 0; i < T_lrf; ++i) {
      if (m <= Tin - i * n) ++n_out;
      else if (c.fin) ++n_out;
      else { splice = i; break; }
    }
    c.splice = std::min(Tin - 1, splice * n);
    c.n_rows = n_out; c.Tin = Tin; c.run_lfr = true;
  };
  c.out_off = r0; c.out_len = (size_t)total;
  if (c.frame_number > 0) {
    const size_t wlen = (size_t)(c.frame_number - 1) * fs + fl;
    if (c.frame_number + vs->n_splice + (m - 1) / 2 > kVadMaxFrames) return fail(PFHIP_ERR_ARG, "too many frames in one online VAD call");
    c.fb_off = r0; c.fb_len = wlen;
    c.fresh = vs->n_splice == 0;
    c.base = c.fresh ? (m - 1) / 2 : vs->n_splice;
    const bool had_reserve = r0 > 0;
    c.out_off = 0; c.out_len = r0 + wlen;                   // reserve_waveforms_ goes in front of what the scorer sees
    const int n_splice = c.fresh ? c.base : vs->n_splice;   // (:48-52) fresh: (m-1)/2 copies of the first frame
    if (c.frame_number + n_splice >= m) {
      const int frame_from_waves = ((int)c.out_len - fl) / fs + 1;
      const int minus_frame = had_reserve ? 0 : (m - 1) / 2;
      online_lfr(n_splice + c.frame_number);
      const int reserve_frame_idx = std::abs(c.splice - minus_frame);
      vs->reserve.assign(c.buf + (size_t)reserve_frame_idx * fs, c.buf + (size_t)frame_from_waves * fs);
      c.out_len = (size_t)(frame_from_waves - 1) * fs + fl;
    } else {
      // (:65-69) the splice cache just grows; the reference runs the network on the raw 80-dim frames here (a latent bug
      // reachable only with < 4 frames in a call): no rows in this restatement
      vs->reserve.assign(c.buf + (fl - fs), c.buf + c.out_len);
    }
  } else if (c.fin) {                                       // (:71-83)
    if (r0) { c.out_off = 0; c.out_len = r0; }
    if (vs->n_splice > 0) online_lfr(vs->n_splice);
  }
  return PFHIP_OK;
}

pfhip_status vad_execute(pfhip_vad* v, std::vector<VadCall>& calls) {
  hipStream_t s = v->stream;
  const int B = (int)calls.size(), m = v->lfr_m, n = v->lfr_n;
  // ---- staging: [fbank meta | op lists | segment descriptors | samples of every connection | silence column] ---------------
  size_t cap_samples = 0, cap_rows = 0;
  for (VadCall& c : calls) {
    const size_t have = c.vs->reserve.size() + c.vs->input_cache.size() + (size_t)c.n_samples;
    cap_samples += have;
    cap_rows += have / 160 + (size_t)c.vs->n_splice + 2;
  }
  const size_t meta_bytes = ((size_t)B * 8 + (size_t)(B + 1) * 4 + (size_t)B * 4 + 63) & ~(size_t)63;
  const size_t ops_max = (size_t)(4 * B + 4) * 32;
  const size_t ctl_bytes = meta_bytes + ops_max + (((size_t)B * sizeof(pfhip::VadSeg) + 63) & ~(size_t)63);
  float* hp_f = v->h_wave(ctl_bytes / 4 + cap_samples + cap_rows + 64);
  if (!hp_f) return fail(PFHIP_ERR_HIP, "pinned staging allocation failed");
  char* hp = reinterpret_cast<char*>(hp_f);
  float* h_pcm = reinterpret_cast<float*>(hp + ctl_bytes);
  float* h_sil = h_pcm + cap_samples;
  {
    size_t so = 0;
    for (VadCall& c : calls) {
      c.buf = h_pcm + so;
      so += c.vs->reserve.size() + c.vs->input_cache.size() + (size_t)c.n_samples;
      pfhip_status st = vad_plan(c);
      if (st) return st;
    }
  }
  // ---- fbank of all new audio in one launch ---------------------------------------------------------------------------
  int total_frames = 0, U = 0, T = 0, max_T = 0;
  for (VadCall& c : calls) {
    if (c.frame_number > 0) { total_frames += c.frame_number; ++U; }
    c.row_off = T; T += c.n_rows; max_T = std::max(max_T, c.n_rows);
  }
  if ((size_t)T > cap_rows) return fail(PFHIP_ERR_UNSUPPORTED, "online VAD row bound exceeded");
  std::vector<pfhip::RowsCopyOp> to_fb, fresh, rotate;
  std::vector<pfhip::VadLfrOp> lfr;
  HIP_TRY(v->ops.ensure(ctl_bytes));
  char* dp = static_cast<char*>(v->ops.p);
  if (U > 0) {
    HIP_TRY(v->pcm.ensure((cap_samples + 1024) * 4));
    HIP_TRY(v->fbk.ensure((size_t)total_frames * 80 * 4));
    int64_t* h_soff = reinterpret_cast<int64_t*>(hp);
    int* h_foff = reinterpret_cast<int*>(hp + (size_t)U * 8);
    int* h_nf = h_foff + (U + 1);
    int fo = 0, u = 0;
    for (VadCall& c : calls) {
      if (c.frame_number <= 0) continue;
      h_soff[u] = (int64_t)((c.buf - h_pcm) + c.fb_off); h_foff[u] = fo; h_nf[u] = c.frame_number;
      float* fb = c.vs->fb[c.vs->fb_cur].f();
      to_fb.push_back(pfhip::RowsCopyOp{fb + (size_t)c.base * 80, v->fbk.f() + (size_t)fo * 80, 80, 80, c.frame_number, 80});
      if (c.fresh) fresh.push_back(pfhip::RowsCopyOp{fb, fb + (size_t)c.base * 80, 80, 0, c.base, 80});
      fo += c.frame_number; ++u;
    }
    h_foff[U] = fo;
    HIP_TRY(hipMemcpyAsync(v->pcm.p, h_pcm, cap_samples * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dp, hp, meta_bytes, hipMemcpyHostToDevice, s));
    const pfhip::FbankTables tb = v->ft.fbank(v->cmvn_mean.f(), v->cmvn_istd.f());
    pfhip::launch_fbank_frames_batch(v->pcm.f(), reinterpret_cast<const int64_t*>(dp), reinterpret_cast<const int*>(dp + (size_t)U * 8),
                                     reinterpret_cast<const int*>(dp + (size_t)U * 8 + (size_t)(U + 1) * 4), U, total_frames, tb,
                                     v->fbk.f(), s);
  }
  pfhip_status ws = vad_workspace(v, std::max(T, 1));
  if (ws) return ws;
  // ---- per-connection frame bookkeeping (splice caches) and the LFR rows, one launch per phase ---------------------------
  std::vector<pfhip::VadSeg> segs;
  for (VadCall& c : calls) {
    pfhip_vad_stream* vs = c.vs;
    if (c.frame_number > 0 && c.fresh) vs->n_splice = c.base;
    if (c.run_lfr) {
      const float* fb = vs->fb[vs->fb_cur].f();
      if (c.n_rows > 0) lfr.push_back(pfhip::VadLfrOp{fb, c.Tin, c.n_rows, c.row_off, 0});
      const int keep = c.Tin - c.splice;                    // lfr_splice_cache_ = frames[splice:]
      rotate.push_back(pfhip::RowsCopyOp{vs->fb[vs->fb_cur ^ 1].f(), fb + (size_t)c.splice * 80, 80, 80, keep, 80});
      vs->fb_cur ^= 1;
      vs->n_splice = keep;
    } else if (c.frame_number > 0) {
      vs->n_splice += c.frame_number;                       // (:65-69) the splice cache just grows
    }
    // (:84-87) a final call: Reset() + ResetCache() run inside ExtractFeats, BEFORE Forward (:143) — scored against
    // zeroed network caches, nothing carried over
    if (c.fin) {
      vs->input_cache.clear(); vs->reserve.clear(); vs->n_splice = 0;
      pfhip_status st = vs_zero_caches(vs, s);
      if (st) return st;
    }
    if (c.n_rows > 0)
      segs.push_back(pfhip::VadSeg{vs->cache[vs->cache_cur].f(), c.fin ? nullptr : vs->cache[vs->cache_cur ^ 1].f(), c.row_off, c.n_rows});
  }
  char* h_ops = hp + meta_bytes;
  char* d_ops = dp + meta_bytes;
  size_t off = 0;
  auto put = [&](const void* src, size_t nb) { const size_t at = off; if (nb) std::memcpy(h_ops + off, src, nb); off += nb; return at; };
  const size_t o_fb = put(to_fb.data(), to_fb.size() * sizeof(pfhip::RowsCopyOp));
  const size_t o_fr = put(fresh.data(), fresh.size() * sizeof(pfhip::RowsCopyOp));
  const size_t o_lfr = put(lfr.data(), lfr.size() * sizeof(pfhip::VadLfrOp));
  const size_t o_rot = put(rotate.data(), rotate.size() * sizeof(pfhip::RowsCopyOp));
  const size_t o_seg = put(segs.data(), segs.size() * sizeof(pfhip::VadSeg));
  if (off) HIP_TRY(hipMemcpyAsync(d_ops, h_ops, off, hipMemcpyHostToDevice, s));
  auto max_rows = [](const std::vector<pfhip::RowsCopyOp>& o) { int mx = 0; for (const auto& x : o) mx = std::max(mx, x.nrows); return mx; };
  pfhip::launch_rows_copy_batch(reinterpret_cast<const pfhip::RowsCopyOp*>(d_ops + o_fb), (int)to_fb.size(), max_rows(to_fb), s);
  pfhip::launch_rows_copy_batch(reinterpret_cast<const pfhip::RowsCopyOp*>(d_ops + o_fr), (int)fresh.size(), max_rows(fresh), s);
  pfhip::launch_lfr_cmvn_online_batch(reinterpret_cast<const pfhip::VadLfrOp*>(d_ops + o_lfr), (int)lfr.size(), max_T, m, n, v->n_mels,
                                      v->cmvn_mean.f(), v->cmvn_istd.f(), v->feats.f(), v->in1.Kp, s);
  pfhip::launch_rows_copy_batch(reinterpret_cast<const pfhip::RowsCopyOp*>(d_ops + o_rot), (int)rotate.size(), max_rows(rotate), s);
  if (T > 0) {
    vad_network(v, s, T, reinterpret_cast<const pfhip::VadSeg*>(d_ops + o_seg), (int)segs.size(), max_T);
    for (VadCall& c : calls)
      if (c.n_rows > 0 && !c.fin) c.vs->cache_cur ^= 1;
  }
  // ---- results: the silence column of all connections in one copy, handed out on the host --------------------------------------
  if (T > 0) HIP_TRY(hipMemcpyAsync(h_sil, v->sil.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  for (VadCall& c : calls) {
    if (c.out_len > c.waves_cap && c.waves_out) return fail(PFHIP_ERR_CAPACITY, "waves_out too small");
    if (c.waves_out && c.out_len) std::memcpy(c.waves_out, c.buf + c.out_off, c.out_len * 4);
    *c.n_waves = (int)c.out_len;
    if ((size_t)c.n_rows > c.cap_floats && c.sil_prob) return fail(PFHIP_ERR_CAPACITY, "sil_prob too small");
    *c.n_frames = c.n_rows;
  }
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (VadCall& c : calls)
    if (c.n_rows > 0 && c.sil_prob) std::memcpy(c.sil_prob, h_sil + c.row_off, (size_t)c.n_rows * 4);
  return PFHIP_OK;
}


// pfhip_vad_stream_infer_batch on per-connection PCM views (either sample format, connection by connection)
pfhip_status vad_stream_infer_batch(pfhip_vad_stream* const* streams, int n_streams, const PcmView* pcm,
                                    const int* n_samples, const int* input_finished, float* const* sil_prob,
                                    const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                    const size_t* waves_cap, int* n_waves) {
  last_error().clear();
  if (!streams || n_streams <= 0 || !pcm || !n_samples || !input_finished || !sil_prob || !cap_floats || !n_frames || !waves_out ||
      !waves_cap || !n_waves)
    return fail(PFHIP_ERR_ARG, "bad argument");
  pfhip_vad* v = streams[0] ? streams[0]->v : nullptr;
  if (!v) return fail(PFHIP_ERR_ARG, "null stream");
  std::vector<VadCall> calls(n_streams);
  for (int i = 0; i < n_streams; ++i) {
    if (!streams[i] || streams[i]->v != v) return fail(PFHIP_ERR_ARG, "streams of one batch must belong to one VAD model");
    for (int j = 0; j < i; ++j) if (streams[j] == streams[i]) return fail(PFHIP_ERR_ARG, "a stream appears twice in one batch");
    if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm[i].p)) return fail(PFHIP_ERR_ARG, "bad pcm buffer");
    if (n_samples[i] > kVadMaxSamples) return fail(PFHIP_ERR_ARG, "more than 64000 samples in one online VAD call");
    calls[i].vs = streams[i]; calls[i].pcm = pcm[i]; calls[i].n_samples = n_samples[i]; calls[i].fin = input_finished[i] != 0;
    calls[i].sil_prob = sil_prob[i]; calls[i].cap_floats = cap_floats[i]; calls[i].n_frames = &n_frames[i];
    calls[i].waves_out = waves_out[i]; calls[i].waves_cap = waves_cap[i]; calls[i].n_waves = &n_waves[i];
    n_frames[i] = 0; n_waves[i] = 0;
  }
  std::lock_guard<std::mutex> lk(v->mu);
  HIP_TRY(hipSetDevice(v->device));
  return vad_execute(v, calls);
}

template <typename Sample>
pfhip_status vad_stream_infer_batch_of(pfhip_vad_stream* const* streams, int n_streams, const Sample* const* pcm,
                                       const int* n_samples, const int* input_finished, float* const* sil_prob,
                                       const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                       const size_t* waves_cap, int* n_waves) {
  std::vector<PcmView> views;
  if (pcm && n_streams > 0)
    for (int i = 0; i < n_streams; ++i) views.push_back(PcmView{pcm[i], sizeof(Sample) == 2});
  return vad_stream_infer_batch(streams, n_streams, views.empty() ? nullptr : views.data(), n_samples, input_finished, sil_prob,
                                cap_floats, n_frames, waves_out, waves_cap, n_waves);
}

}  // namespace

extern "C" {

pfhip_status pfhip_vad_stream_infer_batch(pfhip_vad_stream* const* streams, int n_streams, const float* const* pcm,
                                          const int* n_samples, const int* input_finished, float* const* sil_prob,
                                          const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                          const size_t* waves_cap, int* n_waves) {
  return vad_stream_infer_batch_of(streams, n_streams, pcm, n_samples, input_finished, sil_prob, cap_floats, n_frames, waves_out,
                                   waves_cap, n_waves);
}
// the same on 16-bit PCM (the bytes Audio::LoadPcmwavOnline, audio.cpp:821-857, divides by 32768 on the host); waves_out stays f32
pfhip_status pfhip_vad_stream_infer_batch_s16(pfhip_vad_stream* const* streams, int n_streams, const int16_t* const* pcm,
                                              const int* n_samples, const int* input_finished, float* const* sil_prob,
                                              const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                              const size_t* waves_cap, int* n_waves) {
  return vad_stream_infer_batch_of(streams, n_streams, pcm, n_samples, input_finished, sil_prob, cap_floats, n_frames, waves_out,
                                   waves_cap, n_waves);
}

pfhip_status pfhip_set_vad_stream_batching(pfhip_vad* v, int wait_us, int max_streams) {
  last_error().clear();
  if (!v || wait_us < 0 || max_streams < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> ql(v->mq.mu);
  v->q_wait_us = wait_us;
  v->q_max = max_streams;
  return PFHIP_OK;
}

}  // extern "C"

// One FsmnVadOnline::Infer per websocket handler thread (funasrruntime.cpp:516-532): with wait_us > 0 the first caller to
// arrive leads, waits up to wait_us for the others and runs ONE pfhip_vad_stream_infer_batch for all of them.
struct VadReq : pfhip_impl::MergeReqBase {
  pfhip_vad_stream* vs; pfhip_impl::PcmView pcm;      // f32 and s16 callers merge freely
  int n; int fin; float* sil; size_t cap; int* nf; float* wo; size_t wcap; int* nw;
  pfhip_status st = PFHIP_OK; std::string err;
};

namespace {

void vad_run_requests(const std::vector<VadReq*>& reqs) {
  const int n = (int)reqs.size();
  std::vector<pfhip_vad_stream*> ss(n);
  std::vector<PcmView> pcm(n);
  std::vector<int> ns(n), fin(n), nf(n), nw(n);
  std::vector<float*> sil(n), wo(n);
  std::vector<size_t> cap(n), wcap(n);
  for (int i = 0; i < n; ++i) {
    const VadReq& r = *reqs[i];
    ss[i] = r.vs; pcm[i] = r.pcm; ns[i] = r.n; fin[i] = r.fin; sil[i] = r.sil; cap[i] = r.cap; wo[i] = r.wo; wcap[i] = r.wcap;
  }
  const pfhip_status st = vad_stream_infer_batch(ss.data(), n, pcm.data(), ns.data(), fin.data(), sil.data(), cap.data(),
                                                       nf.data(), wo.data(), wcap.data(), nw.data());
  const std::string err = pfhip_impl::last_error();
  for (int i = 0; i < n; ++i) { *reqs[i]->nf = nf[i]; *reqs[i]->nw = nw[i]; reqs[i]->st = st; reqs[i]->err = err; }
}

pfhip_status vad_infer_queued(pfhip_vad* v, VadReq& me) {
  int wait_us, cap;
  { std::lock_guard<std::mutex> l(v->mq.mu); wait_us = v->q_wait_us; cap = v->q_max; }
  v->mq.submit(
      me, wait_us,
      [&](const std::deque<VadReq*>& q) { return (int)q.size() >= std::min(cap, std::max(1, v->live_streams.load())); },
      [&](std::deque<VadReq*>& q, std::vector<VadReq*>& take) {
        std::deque<VadReq*> later;
        while (!q.empty() && (int)take.size() < cap) {
          VadReq* r = q.front();
          q.pop_front();
          bool dup = false;                       // two queued calls on ONE connection stay in order: the second waits
          for (VadReq* t : take) dup = dup || t->vs == r->vs;
          if (dup) later.push_back(r); else take.push_back(r);
        }
        for (auto it = later.rbegin(); it != later.rend(); ++it) q.push_front(*it);
      },
      [&](std::vector<VadReq*>& take) { vad_run_requests(take); });
  if (me.st != PFHIP_OK) pfhip_impl::last_error() = me.err;
  return me.st;
}

pfhip_status vad_stream_infer_one(pfhip_vad_stream* vs, PcmView pcm, int n_samples, int input_finished, float* sil_prob,
                                  size_t cap_floats, int* n_frames, float* waves_out, size_t waves_cap, int* n_waves) {
  if (!vs || !n_frames || !n_waves) { last_error().clear(); return fail(PFHIP_ERR_ARG, "bad argument"); }
  pfhip_vad* v = vs->v;
  bool queued;
  { std::lock_guard<std::mutex> ql(v->mq.mu); queued = v->q_wait_us > 0 && v->q_max > 1; }
  if (queued) {
    VadReq me;
    me.vs = vs; me.pcm = pcm; me.n = n_samples; me.fin = input_finished; me.sil = sil_prob; me.cap = cap_floats; me.nf = n_frames;
    me.wo = waves_out; me.wcap = waves_cap; me.nw = n_waves;
    return vad_infer_queued(v, me);
  }
  float* sp[1] = {sil_prob};
  float* wo[1] = {waves_out};
  return vad_stream_infer_batch(&vs, 1, &pcm, &n_samples, &input_finished, sp, &cap_floats, n_frames, wo, &waves_cap, n_waves);
}

}  // namespace

extern "C" {

pfhip_status pfhip_vad_stream_infer(pfhip_vad_stream* vs, const float* pcm, int n_samples, int input_finished, float* sil_prob,
                                    size_t cap_floats, int* n_frames, float* waves_out, size_t waves_cap, int* n_waves) {
  return vad_stream_infer_one(vs, PcmView{pcm, false}, n_samples, input_finished, sil_prob, cap_floats, n_frames, waves_out,
                              waves_cap, n_waves);
}
pfhip_status pfhip_vad_stream_infer_s16(pfhip_vad_stream* vs, const int16_t* pcm, int n_samples, int input_finished, float* sil_prob,
                                        size_t cap_floats, int* n_frames, float* waves_out, size_t waves_cap, int* n_waves) {
  return vad_stream_infer_one(vs, PcmView{pcm, true}, n_samples, input_finished, sil_prob, cap_floats, n_frames, waves_out,
                              waves_cap, n_waves);
}

}  // extern "C"
