// CT-Transformer punctuation forward on MI355X — the C ABI's pfhip_punc_* family.
// Replaces the `m_session->Run` + Argmax loop of CTTransformer::Infer (onnxruntime/src/ct-transformer.cpp:162-204):
// token ids [N] -> logits [N, 6] -> punctuation id = first maximum over the first CANDIDATE_NUM-1 classes.
// Same kernels as the ASR encoder (fp32 MFMA GEMMs, FSMN memory block, fused attention) plus an embedding gather fused with
// the x*sqrt(d) + sinusoidal PE step.  Any CT-Transformer with d_model % 4 == 0, d_model <= 1024, a head width
// d_k = d_model / n_head in [1, 64], ffn % 128 == 0, ffn <= 2048: d_k = 32 (the 256 / 8 / 1024 x 4 model of
// punc_ct-transformer_zh-cn-common-vocab272727) runs attention.hip's kernel in its aligned form, every other width in its exact-width form (the large model
// of the reference's English deployment, recalled as 516 / 12 / 2048 x 12: d_k = 43).  The embedding table (272727 x 256 = 279 MB,
// 471067 x 516 = 0.97 GB) stays in HBM; a call touches N rows of it.
//
// Leading dimensions.  The GEMMs run over the weights' padded shapes (internal.h lin_gemm: N = round_up(N, 128), K = round_up(K, 32)),
// so they write round_up(d, 128) columns and read round_up(d, 32): the activations x, y, mem, ctx have the row stride
// ld = round_up(d, 128) and qkv round_up(3 d, 128) (d and 3 d themselves at 256).  The pad columns [d, ld) of everything a GEMM reads
// are zeros (see punc_infer_packed): a pad column meets zero weights, but junk * 0 is NaN when the junk is.
#include <memory>

#include "internal.h"
#include "json_min.h"

using namespace pfhip_impl;

struct PuncReq : pfhip_impl::MergeReqBase {
  const int32_t* ids; int n; int vad_pos; int32_t* out;
  pfhip_status st = PFHIP_OK; std::string err;
};

struct pfhip_punc {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int vocab = 0, d = 256, n_head = 8, ffn = 1024, layers = 4, n_punc = 6, sanm_shift = 0;
  float* d_table = nullptr;
  float* d_inv_ts = nullptr;
  struct Layer { float *n1g, *n1b, *n2g, *n2b, *fsmn; PackedLin qkv, out, ffn1, ffn2; };
  std::vector<Layer> L;
  float *an_g = nullptr, *an_b = nullptr;
  PackedLin head;
  std::vector<DevMem> owned;      // the vectors and tables behind the raw pointers above
  int ld = 256, ldqkv = 768;      // row strides of x / y / mem / ctx and of qkv: round_up(d, 128), round_up(3 d, 128)
  Buf ids, x, y, qkv, mem, ctx, h, logits, punc, meta, lim;
  int* h_pin = nullptr;
  // pinned staging for one (batched) call: [ids | pos | lim | off | len] in, punctuation ids out
  int* h_stage = nullptr; size_t h_stage_cap = 0;
  int* stage(size_t n_ints) {
    if (n_ints > h_stage_cap) {
      if (h_stage) (void)hipHostFree(h_stage);
      h_stage = nullptr; h_stage_cap = 0;
      const size_t cap = n_ints + n_ints / 2 + 1024;
      if (hipHostMalloc((void**)&h_stage, cap * 4, hipHostMallocDefault) == hipSuccess) h_stage_cap = cap;
    }
    return h_stage;
  }
  // merging of concurrent callers (pfhip_set_punc_batching)
  pfhip_impl::MergeQueue<PuncReq> mq;
  int q_wait_us = 0, q_max = 1;
  // the device set and idle before any member gives its memory back (a create that returns early comes through here too)
  ~pfhip_punc() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (h_pin) (void)hipHostFree(h_pin);
    if (h_stage) (void)hipHostFree(h_stage);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

extern "C" {

pfhip_status pfhip_punc_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                                           pfhip_punc** out) {
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
  std::unique_ptr<pfhip_punc> p(new pfhip_punc);
  p->device = device;
  p->vocab = (int)jc->number("vocab", 0);
  p->d = (int)jc->number("d_model", 256);
  p->n_head = (int)jc->number("n_head", 8);
  p->ffn = (int)jc->number("ffn", 1024);
  p->layers = (int)jc->number("layers", 4);
  p->n_punc = (int)jc->number("n_punc", 6);
  const int kernel = (int)jc->number("kernel", 11);
  p->sanm_shift = (int)jc->number("sanm_shift", 0);
  if (p->sanm_shift != 0 && p->sanm_shift != 5) return fail(PFHIP_ERR_UNSUPPORTED, "sanm_shift must be 0 or 5");
  const int d = p->d;
  if (p->vocab <= 0 || d < 4 || d % 4 || d > 1024 || p->n_head < 1 || d % p->n_head || d / p->n_head > 64 || kernel != 11 || p->ffn < 128 ||
      p->ffn % 128 || p->ffn > 2048 || p->n_punc < 2 || p->n_punc > 128)
    return fail(PFHIP_ERR_UNSUPPORTED,
                "CT-Transformer kernels need d_model % 4 == 0, d_model <= 1024, d_model % n_head == 0, 1 <= d_model / n_head <= 64, "
                "ffn % 128 == 0, ffn <= 2048, FSMN kernel 11, 2 <= n_punc <= 128 (got d_model " + std::to_string(d) + ", n_head " +
                std::to_string(p->n_head) + ", ffn " + std::to_string(p->ffn) + ", kernel " + std::to_string(kernel) + ", n_punc " +
                std::to_string(p->n_punc) + ")");
  p->ld = round_up(d, 128);
  p->ldqkv = round_up(3 * d, 128);
  const float* hb = static_cast<const float*>(blob);
  auto get = [&](const std::string& name, std::vector<int> shape, const float** ptr) -> bool {
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
    *ptr = hb + off / 4;
    return true;
  };
  auto dev_copy = [&](const float* src, size_t n, float** dst) -> pfhip_status {
    DevMem mem;
    HIP_TRY(mem.upload(src, n * 4));
    *dst = mem.f();
    p->owned.push_back(std::move(mem));
    return PFHIP_OK;
  };
  auto vec = [&](const std::string& name, int n, float** dst) -> pfhip_status {
    const float* src = nullptr;
    if (!get(name, {n}, &src)) return PFHIP_ERR_FORMAT;
    return dev_copy(src, n, dst);
  };
  auto lin = [&](const std::string& name, int N, int K, PackedLin* l) -> pfhip_status {
    const float *w = nullptr, *b = nullptr;
    if (!get(name + ".w", {N, K}, &w) || !get(name + ".b", {N}, &b)) return PFHIP_ERR_FORMAT;
    return pack_linear(w, b, N, K, l);
  };
  pfhip_status st;
  {
    const float* tab = nullptr;
    if (!get("embed.w", {p->vocab, d}, &tab)) return PFHIP_ERR_FORMAT;
    if ((st = dev_copy(tab, (size_t)p->vocab * d, &p->d_table))) return st;
  }
  p->L.resize(p->layers);
  for (int i = 0; i < p->layers; ++i) {
    const std::string q = "enc." + std::to_string(i) + ".";
    pfhip_punc::Layer& l = p->L[i];
    const float* fw = nullptr;
    if ((st = vec(q + "norm1.g", d, &l.n1g)) || (st = vec(q + "norm1.b", d, &l.n1b)) || (st = vec(q + "norm2.g", d, &l.n2g)) ||
        (st = vec(q + "norm2.b", d, &l.n2b)) || (st = lin(q + "qkv", 3 * d, d, &l.qkv)) || (st = lin(q + "out", d, d, &l.out)) ||
        (st = lin(q + "ffn1", p->ffn, d, &l.ffn1)) || (st = lin(q + "ffn2", d, p->ffn, &l.ffn2)))
      return st;
    if (!get(q + "fsmn.w", {d, kernel}, &fw)) return PFHIP_ERR_FORMAT;
    if ((st = dev_copy(fw, (size_t)d * kernel, &l.fsmn))) return st;
  }
  if ((st = vec("enc.after_norm.g", d, &p->an_g)) || (st = vec("enc.after_norm.b", d, &p->an_b)) ||
      (st = lin("out", p->n_punc, d, &p->head)))
    return st;
  {
    const int half = d / 2;
    std::vector<float> inv(half);
    const float scale = (float)(-std::log(10000.0) / (half - 1));
    for (int i = 0; i < half; ++i) inv[i] = (float)exp((double)(i * scale));
    if ((st = dev_copy(inv.data(), half, &p->d_inv_ts))) return st;
  }
  HIP_TRY(p->meta.ensure(256));
  HIP_TRY(hipHostMalloc((void**)&p->h_pin, 256, hipHostMallocDefault));
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  *out = p.release();
  return PFHIP_OK;
}

void pfhip_punc_destroy(pfhip_punc* p) { delete p; }

int pfhip_punc_num_classes(const pfhip_punc* p) { return p ? p->n_punc : 0; }

// B sequences packed row-wise through one pass: per-sequence positions for the embedding, (offset, length) pairs for the FSMN
// memory and the attention, per-row key limits for the realtime mask.  vad_pos == nullptr: the offline model.
static pfhip_status punc_infer_packed(pfhip_punc* p, const int32_t* const* ids, const int* n, const int* vad_pos, int B,
                                      int32_t* const* punc_out, float* logits_out);

static pfhip_status punc_infer_queued(pfhip_punc* p, const int32_t* ids, int n, int vad_pos, int32_t* punc_out);

pfhip_status pfhip_punc_infer(pfhip_punc* p, const int32_t* ids, int n, int32_t* punc_out, float* logits_out) {
  last_error().clear();
  if (!p || !ids || n <= 0 || !punc_out) return fail(PFHIP_ERR_ARG, "bad argument");
  if (p->q_wait_us > 0 && p->q_max > 1 && !logits_out) return punc_infer_queued(p, ids, n, -1, punc_out);
  return punc_infer_packed(p, &ids, &n, nullptr, 1, &punc_out, logits_out);
}

pfhip_status pfhip_punc_infer_online(pfhip_punc* p, const int32_t* ids, int n, int cache_size, int32_t* punc_out,
                                     float* logits_out) {
  last_error().clear();
  if (!p || !ids || n <= 0 || !punc_out) return fail(PFHIP_ERR_ARG, "bad argument");
  const int vp = cache_size < 0 ? 0 : cache_size;
  if (p->q_wait_us > 0 && p->q_max > 1 && !logits_out) return punc_infer_queued(p, ids, n, vp, punc_out);
  return punc_infer_packed(p, &ids, &n, &vp, 1, &punc_out, logits_out);
}

pfhip_status pfhip_set_punc_batching(pfhip_punc* p, int wait_us, int max_sequences) {
  last_error().clear();
  if (!p || wait_us < 0 || max_sequences < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> l(p->mq.mu);
  p->q_wait_us = wait_us;
  p->q_max = max_sequences;
  return PFHIP_OK;
}

pfhip_status pfhip_punc_infer_batch(pfhip_punc* p, const int32_t* const* ids, const int* n, const int* cache_size, int n_seq,
                                    int32_t* const* punc_out) {
  last_error().clear();
  if (!p || !ids || !n || n_seq <= 0 || !punc_out) return fail(PFHIP_ERR_ARG, "bad argument");
  for (int b = 0; b < n_seq; ++b)
    if (!ids[b] || n[b] <= 0 || !punc_out[b]) return fail(PFHIP_ERR_ARG, "bad sequence");
  std::vector<int> vp;
  if (cache_size) { vp.assign(cache_size, cache_size + n_seq); for (int& v : vp) v = v < 0 ? 0 : v; }
  return punc_infer_packed(p, ids, n, cache_size ? vp.data() : nullptr, n_seq, punc_out, nullptr);
}

// One Infer per handler thread (every connection's AddPunc makes a few): merged into packed passes like the ASR calls.
static pfhip_status punc_infer_queued(pfhip_punc* p, const int32_t* ids, int n, int vad_pos, int32_t* punc_out) {
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= p->vocab) return fail(PFHIP_ERR_ARG, "token id outside the embedding table");
  PuncReq me;
  me.ids = ids; me.n = n; me.vad_pos = vad_pos; me.out = punc_out;
  int wait_us, cap;
  { std::lock_guard<std::mutex> l(p->mq.mu); wait_us = p->q_wait_us; cap = p->q_max; }
  p->mq.submit(
      me, wait_us, [&](const std::deque<PuncReq*>& q) { return (int)q.size() >= cap; },
      [&](std::deque<PuncReq*>& q, std::vector<PuncReq*>& take) {
        // one pass serves one kind of mask: offline (vad_pos < 0) and realtime calls are not mixed
        const bool online = q.front()->vad_pos >= 0;
        std::deque<PuncReq*> later;
        while (!q.empty() && (int)take.size() < cap) {
          PuncReq* r = q.front();
          q.pop_front();
          if ((r->vad_pos >= 0) == online) take.push_back(r); else later.push_back(r);
        }
        for (auto it = later.rbegin(); it != later.rend(); ++it) q.push_front(*it);
      },
      [&](std::vector<PuncReq*>& take) {
        const int B = (int)take.size();
        std::vector<const int32_t*> ids_v(B);
        std::vector<int> n_v(B), vp(B);
        std::vector<int32_t*> out_v(B);
        for (int b = 0; b < B; ++b) { ids_v[b] = take[b]->ids; n_v[b] = take[b]->n; vp[b] = take[b]->vad_pos; out_v[b] = take[b]->out; }
        const pfhip_status st = punc_infer_packed(p, ids_v.data(), n_v.data(), take[0]->vad_pos >= 0 ? vp.data() : nullptr, B,
                                                  out_v.data(), nullptr);
        const std::string err = last_error();
        for (PuncReq* r : take) { r->st = st; r->err = err; }
      },
      /*fresh_no_wait=*/true);          // a lone caller runs at once; company gathers behind the pass that is executing
  if (me.st != PFHIP_OK) last_error() = me.err;
  return me.st;
}

static pfhip_status punc_infer_packed(pfhip_punc* p, const int32_t* const* ids, const int* n, const int* vad_pos, int B,
                                      int32_t* const* punc_out, float* logits_out) {
  int total = 0, max_n = 0;
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < n[b]; ++i)
      if (ids[b][i] < 0 || ids[b][i] >= p->vocab) return fail(PFHIP_ERR_ARG, "token id outside the embedding table");
    total += n[b];
    max_n = std::max(max_n, n[b]);
  }
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int d = p->d, ld = p->ld, ldqkv = p->ldqkv, Np = round_up(total, 128);
  // Pad columns [d, ld) of the GEMMs' A operands and residuals, zero by construction (nothing to do at ld == d):
  //   x    the embedding gather zeroes them on every call; a GEMM epilogue then writes 0 (zero weights and bias) + mem's + x's own
  //   y    every LayerNorm launch zeroes columns [d, Dout = ld)
  //   ctx  the attention writes columns [0, d) only, and mem's producer (the FSMN block) likewise: a buffer that `ensure` has just
  //   mem  (re)allocated is cleared whole, on the stream, ahead of its first use, and nothing ever writes its pad columns
  // h needs none (ffn % 128 == 0: K is ffn itself); qkv's pad columns are written by its GEMM and read by nobody.
  auto ensure_cleared = [&](Buf& b, size_t bytes) -> pfhip_status {
    const bool grows = bytes > b.cap;
    HIP_TRY(b.ensure(bytes));
    if (grows && ld != d) HIP_TRY(hipMemsetAsync(b.p, 0, b.cap, s));
    return PFHIP_OK;
  };
  HIP_TRY(p->x.ensure((size_t)Np * ld * 4));
  HIP_TRY(p->y.ensure((size_t)Np * ld * 4));
  HIP_TRY(p->qkv.ensure((size_t)Np * ldqkv * 4));
  if (pfhip_status st = ensure_cleared(p->mem, (size_t)Np * ld * 4)) return st;
  if (pfhip_status st = ensure_cleared(p->ctx, (size_t)Np * ld * 4)) return st;
  HIP_TRY(p->h.ensure((size_t)Np * p->ffn * 4));
  HIP_TRY(p->logits.ensure((size_t)Np * 128 * 4));
  HIP_TRY(p->punc.ensure((size_t)total * 4));
  // one upload: [ids | pos | lim | off | len]
  const size_t n_in = (size_t)3 * total + (size_t)2 * B;
  int* hs = p->stage(n_in + (size_t)total);
  if (!hs) return fail(PFHIP_ERR_HIP, "pinned staging allocation failed");
  int *h_ids = hs, *h_pos = hs + total, *h_lim = hs + 2 * total, *h_off = hs + 3 * total, *h_len = h_off + B;
  int* h_out = hs + n_in;
  for (int b = 0, r = 0; b < B; ++b) {
    h_off[b] = r; h_len[b] = n[b];
    std::memcpy(h_ids + r, ids[b], (size_t)n[b] * 4);
    // CTTransformerOnline::VadMask (ct-transformer-online.cpp:225-240) as a per-query key limit: rows i < vad_pos-1 see
    // keys [0, vad_pos), all other rows see everything; the reference feeds this ONE mask to both mask inputs (:182-197)
    const int vp = vad_pos ? vad_pos[b] : 0;
    for (int i = 0; i < n[b]; ++i) {
      h_pos[r + i] = i;
      h_lim[r + i] = (vp > 0 && vp < n[b] && i < vp - 1) ? vp : n[b];
    }
    r += n[b];
  }
  HIP_TRY(p->meta.ensure(n_in * 4));
  HIP_TRY(hipMemcpyAsync(p->meta.p, hs, n_in * 4, hipMemcpyHostToDevice, s));
  const int* d_ids = p->meta.i();
  const int* d_pos = d_ids + total;
  const int* d_lim = vad_pos ? d_ids + 2 * total : nullptr;
  const int* d_off = d_ids + 3 * total;
  const int* d_len = d_off + B;
  float* x = p->x.f();
  pfhip::launch_embed_gather(d_ids, p->d_table, p->vocab, d, ld, x, ld, total, p->d_inv_ts, sqrtf((float)d), B > 1 ? d_pos : nullptr, s);
  // every layer's attention, with the VadMask prefix limits when the model is the online one: d_k = 32 on the aligned form of attention.hip's
  // kernel, any other width on its exact-width form
  const int dk = d / p->n_head;
  pfhip::AttnOp att{.Q = p->qkv.f(), .ldq = ldqkv, .K = p->qkv.f() + d, .ldk = ldqkv, .V = p->qkv.f() + 2 * d, .ldv = ldqkv,
                    .O = p->ctx.f(), .ldo = ld};
  att.q_off = att.kv_off = d_off; att.q_len = att.kv_len = d_len;
  att.B = B; att.H = p->n_head; att.max_q_len = max_n; att.scale = 1.0f / sqrtf((float)dk); att.head_dim = dk; att.q_kv_limit = d_lim;
  for (int i = 0; i < p->layers; ++i) {
    const pfhip_punc::Layer& l = p->L[i];
    pfhip::launch_layernorm(x, ld, p->y.f(), ld, l.n1g, l.n1b, total, d, ld, 1e-12f, s);
    lin_gemm(s, l.qkv, p->y.f(), ld, p->qkv.f(), ldqkv, nullptr, 0, nullptr, 0, total, false);
    pfhip::launch_fsmn_shift(p->qkv.f() + 2 * d, ldqkv, l.fsmn, nullptr, 0, p->mem.f(), ld, d_off, d_len, B, max_n, d,
                             p->sanm_shift, s);
    if (dk == 32) pfhip::launch_attention(att, s);
    else pfhip::launch_attention_dk(att, s);
    lin_gemm(s, l.out, p->ctx.f(), ld, x, ld, p->mem.f(), ld, x, ld, total, false);          // in_size == size: residual
    pfhip::launch_layernorm(x, ld, p->y.f(), ld, l.n2g, l.n2b, total, d, ld, 1e-12f, s);
    lin_gemm(s, l.ffn1, p->y.f(), ld, p->h.f(), p->ffn, nullptr, 0, nullptr, 0, total, true);
    lin_gemm(s, l.ffn2, p->h.f(), p->ffn, x, ld, x, ld, nullptr, 0, total, false);
  }
  pfhip::launch_layernorm(x, ld, p->y.f(), ld, p->an_g, p->an_b, total, d, ld, 1e-12f, s);
  lin_gemm(s, p->head, p->y.f(), ld, p->logits.f(), 128, nullptr, 0, nullptr, 0, total, false);
  // Argmax(p, p + CANDIDATE_NUM - 1): first maximum over the first n_punc-1 classes (ct-transformer.cpp:193-196)
  pfhip::launch_argmax_first(p->logits.f(), 128, total, p->n_punc - 1, static_cast<int32_t*>(p->punc.p), s);
  HIP_TRY(hipMemcpyAsync(h_out, p->punc.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  if (logits_out)
    HIP_TRY(hipMemcpy2DAsync(logits_out, (size_t)p->n_punc * 4, p->logits.p, 128 * 4, (size_t)p->n_punc * 4, total,
                             hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (int b = 0; b < B; ++b) std::memcpy(punc_out[b], h_out + h_off[b], (size_t)n[b] * 4);
  return PFHIP_OK;
}

}  // extern "C"

// ---- AddPunc's mini-sentence bookkeeping on token ids (ct-transformer.cpp:39-155) --------------------
// The text side of AddPunc (tokeniser, joining words and punctuation strings, en-bpe symbol mapping) stays above this call;
// what is restated here decides WHICH ids each Infer sees and which punctuation every token finally gets: 20-token
// mini-sentences, the un-punctuated tail of a mini-sentence carried into the next one (RemainIDs), a forced period at the
// last comma once the carried text exceeds CACHE_POP_TRIGGER_LIMIT, and the sentence-final fix-up of the last token.
pfhip_status pfhip_punc_add_punc(pfhip_punc* p, const int32_t* ids, int n, int32_t* punc_out, int cap, int* n_out) {
  last_error().clear();
  if (!p || !ids || n < 0 || !punc_out || !n_out) return fail(PFHIP_ERR_ARG, "bad argument");
  constexpr int kTokenLen = 20, kCachePopTriggerLimit = 200;           // com-define.h:126,136
  constexpr int kNotPunc = 1, kComma = 2, kPeriod = 3, kQuestion = 4, kDun = 5;   // com-define.h:131-135
  *n_out = 0;
  std::vector<int32_t> remain, out;
  const int total_batch = (n + kTokenLen - 1) / kTokenLen;
  for (int i = 0; i < n; i += kTokenLen) {
    const int take = std::min(kTokenLen, n - i);
    std::vector<int32_t> input(remain);
    input.insert(input.end(), ids + i, ids + i + take);
    std::vector<int32_t> punc(input.size());
    pfhip_status st = pfhip_punc_infer(p, input.data(), (int)input.size(), punc.data(), nullptr);
    if (st) return st;
    const int cur_batch = i / kTokenLen;
    if (cur_batch < total_batch - 1) {                                // not the last mini-sentence (:66-90)
      int sent_end = -1, last_comma = -1;
      for (int k = (int)punc.size() - 2; k > 0; --k) {
        if (punc[k] == kPeriod || punc[k] == kQuestion) { sent_end = k; break; }
        if (last_comma < 0 && punc[k] == kComma) last_comma = k;
      }
      if (sent_end < 0 && (int)input.size() > kCachePopTriggerLimit && last_comma > 0) {
        sent_end = last_comma;
        punc[sent_end] = kPeriod;
      }
      remain.assign(input.begin() + (sent_end + 1), input.end());
      punc.resize((size_t)(sent_end + 1));
    }
    out.insert(out.end(), punc.begin(), punc.end());
  }
  if (!out.empty()) {                                                 // last mini-sentence (:112-127)
    const int last = out.back();
    if (last == kComma || last == kDun) out.back() = kPeriod;
    else if (last != kPeriod && last != kQuestion) out.push_back(kPeriod);   // a period is APPENDED after the last token
  }
  (void)kNotPunc;
  if ((int)out.size() > cap) return fail(PFHIP_ERR_CAPACITY, "punc_out too small (needs up to n + 1)");
  std::copy(out.begin(), out.end(), punc_out);
  *n_out = (int)out.size();
  return PFHIP_OK;
}
