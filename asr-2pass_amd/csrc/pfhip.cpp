// C-ABI implementation (include/pfhip.h): model container + launch sequence of the offline
// Paraformer forward on one MI355X.  Layout in HBM:
//   * all utterances of a batch are PACKED row-major with no padding rows: utterance b owns LFR rows
//     [row_off[b], row_off[b]+T_b) of every [M, *] activation matrix (M = sum T_b); the reference's
//     GPU flavour zero-pads to Tmax instead (onnxruntime/src/paraformer-torch.cpp:342-347);
//   * decoder-side matrices are packed the same way over the CIF-fired tokens (ML = sum fires);
//   * weights stay in the blob's torch [out,in] layout = the K-contiguous B operand of the GEMM.
// This file: handles, getters, execution slots.  The rest of the offline path: one concern per file, see offline.h.
#include "../../include/pfhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "offline.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

// PFHIP_DEVICES="0,1,2,..." turns every model created through pfhip_create / pfhip_create_from_memory into a group with one
// replica per listed device (the `device` argument is then ignored): the unchanged server with its one shared handle and
// `decoder-thread-num` threads (funasr-wss-server.cpp:479-481) uses all of them.
bool env_devices(std::vector<int>& devs) {
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
pfhip_status apply_env_inflight(pfhip_model** out) {
  const char* e = std::getenv("PFHIP_INFLIGHT");
  if (!e || !*e) return PFHIP_OK;
  const int n = std::atoi(e);
  if (n < 1 || n > 16) return PFHIP_OK;
  const pfhip_status st = pfhip_set_inflight(*out, n);
  if (st) { const std::string why = g_err; pfhip_destroy(*out); *out = nullptr; g_err = why; }
  return st;
}

}  // namespace

namespace pfhip_impl {

std::string& last_error() {
  thread_local std::string e;
  return e;
}

// ---- execution slots -----------------------------------------------------------------------------------------------
// A handle fronts one or more execution slots: the contexts of its device (pfhip_set_inflight) and of every replica device
// (pfhip_create_group).  `slots` on the head lists them device-major per round (context 0 of every device, then context 1 of
// every device, ...), so that filling them in order spreads calls over the GPUs before it stacks them on one.
void rebuild_slots_locked(pfhip_model* head) {
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
pfhip_model* acquire_slot(pfhip_model* head) {
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
void release_slot(pfhip_model* head, pfhip_model* slot) {
  --slot->inflight;
  head->bq.slot_freed();
}

// every execution slot of the handle, for calls that configure all of them
std::vector<pfhip_model*> all_slots(pfhip_model* head) {
  std::lock_guard<std::mutex> l(head->bq.mu);
  if (head->slots.empty()) rebuild_slots_locked(head);
  return head->slots;
}

}  // namespace pfhip_impl

// =================================================================================================
extern "C" {

const char* pfhip_last_error(void) { return g_err.c_str(); }

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
int pfhip_has_timestamp_head(const pfhip_model* m) { return m ? m->weights->cfg.timestamp : 0; }

pfhip_status pfhip_set_batching(pfhip_model* m, int wait_us, int max_utterances) {
  g_err.clear();
  if (!m || wait_us < 0 || max_utterances < 1) return fail(PFHIP_ERR_ARG, "bad argument");
  if (is_svs(m)) return fail(PFHIP_ERR_UNSUPPORTED, "a SenseVoice (CTC) handle merges its callers through pfhip_svs_set_batching");
  std::lock_guard<std::mutex> ql(m->bq.mu);
  m->batch_wait_us = wait_us;
  m->batch_max_utts = max_utterances;
  return PFHIP_OK;
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

}  // extern "C"
