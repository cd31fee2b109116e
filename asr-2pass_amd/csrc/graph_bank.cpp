// The per-device bank of hotword context graphs (internal.h GraphBankDev; hotword_bank.h keeps the books): packed graph images
// that stay on the device between forwards, found again by content.  Serves pfhip_svs_forward_beam_sets and merged beam callers.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "ctx_graph.h"
#include "offline.h"

#define g_err (pfhip_impl::last_error())

namespace {
using namespace pfhip_impl;

constexpr size_t kRowBytes = kGraphRowBytes;

pfhip_model* bank_owner(pfhip_model* m) { return m->weights_of ? m->weights_of : m; }

// sizes the arena at first use; the bank mutex is held
void ensure_bank_locked(pfhip_model* owner) {
  GraphBankDev& D = *owner->gbank;
  if (D.configured) return;
  if (D.bound_bytes < 0) {
    const char* e = getenv("PFHIP_CTX_GRAPH_BANK_MB");
    const long mb = e && *e ? atol(e) : 16;
    D.bound_bytes = (int64_t)std::max(0L, mb) << 20;
  }
  graph_bank_configure(D.bank, D.bound_bytes);
  const size_t bytes = (size_t)D.bank.capacity_granules() * kRowBytes;
  if (bytes > 0 && hipMalloc((void**)&D.arena, bytes) != hipSuccess) {
    (void)hipGetLastError();          // no room for the arena: every graph goes up with its call
    D.arena = nullptr;
    graph_bank_configure(D.bank, 0);
  }
  D.configured = true;
}

}  // namespace

namespace pfhip_impl {

void svs_release_graphs(pfhip_model* m) {
  if (m->svs_graph_pins.empty()) return;
  GraphBankDev& D = *bank_owner(m)->gbank;
  std::lock_guard<std::mutex> l(D.mu);
  for (int id : m->svs_graph_pins) {
    D.bank.entry(id).settled = true;          // the forward has synchronised: whatever filled the slab is complete
    D.bank.release(id);
  }
  m->svs_graph_pins.clear();
}

// Before the first launch of a forward in its sets form: every graph of m->svs_beam_graphs is looked up in the device's bank and
// pinned; m->svs_graph_dev[g] becomes its image there, or null for a graph the bank cannot take (it then goes up with the call).
// All misses go up in ONE copy from the pinned staging to a device staging and from there, device to device, into their slabs, on
// `s`; the ready event tells other contexts' streams when.  m->mu is held.
pfhip_status svs_pin_graphs_locked(pfhip_model* m, hipStream_t s) {
  const size_t G = m->svs_beam_graphs.size();
  m->svs_graph_dev.assign(G, nullptr);
  if (G == 0) return PFHIP_OK;
  GraphBankDev& D = *bank_owner(m)->gbank;
  std::lock_guard<std::mutex> l(D.mu);
  ensure_bank_locked(bank_owner(m));
  if (D.bank.capacity_granules() == 0) return PFHIP_OK;
  std::vector<int> ids(G, -1), miss;            // per graph its entry; the graphs this forward fills
  std::vector<size_t> up_off(G, 0);
  size_t up_bytes = 0;
  std::vector<float> padded;
  for (size_t g = 0; g < G; ++g) {
    const pfhip_ctx_graph* cg = m->svs_beam_graphs[g];
    bool hit = false;
    ids[g] = graph_bank_acquire(D.bank, cg->packed.data(), cg->packed.size(), &hit, &padded);
    if (ids[g] < 0) continue;                   // refused: with the call
    m->svs_graph_pins.push_back(ids[g]);
    m->svs_graph_dev[g] = D.arena + graph_bank_offset(D.bank, ids[g]);
    if (!hit) { miss.push_back((int)g); up_off[g] = up_bytes; up_bytes += (size_t)graph_bank_rows(cg->packed.size()) * kRowBytes; }
  }
  // an upload that cannot be enqueued leaves no entry behind that claims an image it does not hold (nobody else can have found the
  // entries: the bank's mutex has been held since they were made); graphs of this call on such an entry go up with the call
  auto give_up = [&](size_t from, pfhip_status st) {
    for (size_t i = from; i < miss.size(); ++i) {
      const int id = ids[(size_t)miss[i]];
      m->svs_graph_pins.erase(std::remove(m->svs_graph_pins.begin(), m->svs_graph_pins.end(), id), m->svs_graph_pins.end());
      for (size_t g = 0; g < G; ++g)
        if (ids[g] == id) { ids[g] = -1; m->svs_graph_dev[g] = nullptr; }
      D.bank.discard(id);
    }
    return st;
  };
  if (up_bytes) {
    if (m->svs_graph_stage.ensure(up_bytes) != hipSuccess || m->svs_graph_up.ensure(up_bytes) != hipSuccess)
      return give_up(0, fail(PFHIP_ERR_HIP, "allocation of the graph staging buffers failed"));
    char* host = static_cast<char*>(m->svs_graph_stage.p);
    std::memset(host, 0, up_bytes);
    for (int g : miss) std::memcpy(host + up_off[(size_t)g], m->svs_beam_graphs[(size_t)g]->packed.data(), m->svs_beam_graphs[(size_t)g]->packed.size() * 4);
    if (hipMemcpyAsync(m->svs_graph_up.p, host, up_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
      return give_up(0, fail(PFHIP_ERR_HIP, "upload of the context graphs failed"));
    for (size_t i = 0; i < miss.size(); ++i) {
      const int g = miss[i], id = ids[(size_t)g];
      HotwordBank::Entry& e = D.bank.entry(id);
      hipError_t he = hipMemcpyAsync(D.arena + graph_bank_offset(D.bank, id), static_cast<const char*>(m->svs_graph_up.p) + up_off[(size_t)g],
                                     (size_t)e.H * kRowBytes, hipMemcpyDeviceToDevice, s);
      if (he == hipSuccess && !e.ready) {
        hipEvent_t ev;
        he = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (he == hipSuccess) e.ready = ev;
      }
      if (he == hipSuccess) he = hipEventRecord(static_cast<hipEvent_t>(e.ready), s);
      if (he != hipSuccess) return give_up(i, fail(PFHIP_ERR_HIP, "fill of the graph bank failed"));      // the earlier ones stay
      e.ready_on = s;
    }
  }
  for (size_t g = 0; g < G; ++g) {              // a hit that another context's stream is still filling: this stream waits for its event
    if (ids[g] < 0) continue;
    HotwordBank::Entry& e = D.bank.entry(ids[g]);
    if (!e.settled && e.ready && e.ready_on && e.ready_on != s) HIP_TRY(hipStreamWaitEvent(s, static_cast<hipEvent_t>(e.ready), 0));
  }
  return PFHIP_OK;
}

void destroy_graph_bank(pfhip_model* m) {
  if (!m->gbank) return;
  GraphBankDev& D = *m->gbank;
  for (size_t i = 0; i < D.bank.id_count(); ++i)
    if (D.bank.entry((int)i).ready) (void)hipEventDestroy(static_cast<hipEvent_t>(D.bank.entry((int)i).ready));
  if (D.arena) (void)hipFree(D.arena);
  D.arena = nullptr;
}

}  // namespace pfhip_impl

extern "C" {

pfhip_status pfhip_svs_set_graph_bank_bytes(pfhip_model* m, int64_t bytes) {
  g_err.clear();
  if (!m || bytes < 0) return fail(PFHIP_ERR_ARG, "bad argument");
  if (!is_svs(m)) return fail(PFHIP_ERR_UNSUPPORTED, "not a SenseVoice (CTC) model: there is no search to keep graphs for");
  if (m->group_head || m->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  std::lock_guard<std::mutex> lk(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  GraphBankDev& D = *m->gbank;
  std::lock_guard<std::mutex> l(D.mu);
  if (D.bank.pinned_entries() > 0) return fail(PFHIP_ERR_ARG, "graph bank in use: set its bound while no forward is in flight");
  HIP_TRY(hipDeviceSynchronize());
  if (D.arena) HIP_TRY(hipFree(D.arena));
  D.arena = nullptr;
  D.bound_bytes = bytes;
  D.configured = false;
  ensure_bank_locked(m);
  return PFHIP_OK;
}

pfhip_status pfhip_svs_graph_bank_stats(pfhip_model* m, pfhip_svs_graph_bank_stats_t* out) {
  g_err.clear();
  if (!m || !out) return fail(PFHIP_ERR_ARG, "bad argument");
  *out = pfhip_svs_graph_bank_stats_t{};
  pfhip_model* owner = m->weights_of ? m->weights_of : m;
  GraphBankDev& D = *owner->gbank;
  std::lock_guard<std::mutex> l(D.mu);
  out->hits = D.bank.hits; out->misses = D.bank.misses; out->evictions = D.bank.evictions; out->refused = D.bank.refused;
  out->bytes_in_use = (int64_t)D.bank.used_granules() * (int64_t)kRowBytes;
  out->bytes_capacity = (int64_t)D.bank.capacity_granules() * (int64_t)kRowBytes;
  out->graphs_resident = D.bank.live_entries();
  return PFHIP_OK;
}

}  // extern "C"
