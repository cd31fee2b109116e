// Hotwords: the per-device bank of projected K/V rows, a forward's sets, the default set, the embedder.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

#include "offline.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

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

// The default set becomes (or stays) a pinned entry of the device's bank: filled on the owner's stream and waited for, the previous
// default let go.  owner->mu is held.  A set the bank cannot take stays a host copy and is projected per call.
pfhip_status pin_default_hotwords(pfhip_model* owner, const float* hw_emb, int H) {
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

std::vector<pfhip_model*> device_owners(pfhip_model* head) {
  std::lock_guard<std::mutex> l(head->bq.mu);
  std::vector<pfhip_model*> devs{head};
  for (pfhip_model* r : head->replicas) devs.push_back(r);
  return devs;
}

}  // namespace

namespace pfhip_impl {

void release_hotwords(pfhip_model* m) {
  if (m->fw_pins.empty()) return;
  HwBankDev& D = *bank_owner(m)->hwbank;
  std::lock_guard<std::mutex> l(D.mu);
  for (int id : m->fw_pins) D.bank.release(id);
  m->fw_pins.clear();
}

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

}  // namespace pfhip_impl

extern "C" {

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

int pfhip_is_contextual(const pfhip_model* m) { return m ? m->weights->cfg.contextual : 0; }

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

}  // extern "C"
