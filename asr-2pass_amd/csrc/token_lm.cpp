// pfhip_set_token_lm: a token n-gram language model (lm_graph.h) for the searches of a handle's forwards.  The packed image goes to
// the handle's device once, into memory a TokenLm owns (weights.h DevMem); the forwards that search — pfhip_svs_forward_beam[_sets],
// merged beam callers, pfhip_offline_forward_bias — take a reference for their length and run the kernels' model-walking
// instantiations (heads.cpp).  Without a model nothing here is reached and every call launches what it always launched.
#include "../../include/pfhip.h"

#include "beam_front.h"
#include "internal.h"
#include "lm_graph.h"
#include "offline.h"

using namespace pfhip_impl;
#define g_err (pfhip_impl::last_error())

namespace pfhip_impl {

std::shared_ptr<const TokenLm> token_lm_of(pfhip_model* m) {
  pfhip_model* head = m->group_head ? m->group_head : m;
  std::lock_guard<std::mutex> l(head->lm_mu);
  return head->token_lm;
}

}  // namespace pfhip_impl

extern "C" {

pfhip_status pfhip_set_token_lm(pfhip_model* m, const pfhip_lm_graph* lm) {
  g_err.clear();
  if (!m) return fail(PFHIP_ERR_ARG, "null model");
  if (m->group_head || m->weights_of) return fail(PFHIP_ERR_ARG, "not the handle pfhip_create returned");
  if (!m->replicas.empty()) return fail(PFHIP_ERR_UNSUPPORTED, "token lm: not on a multi-device group");
  if (lm && lm->vocab != m->weights->cfg.vocab)
    return fail(PFHIP_ERR_ARG, "token lm: built for a vocabulary of " + std::to_string(lm->vocab) + ", the model has " +
                                   std::to_string(m->weights->cfg.vocab));
  for (pfhip_model* slot : all_slots(m))
    if (slot->inflight.load() > 0) return fail(PFHIP_ERR_ARG, "token lm: set it while no forward is in flight");
  std::shared_ptr<TokenLm> made;
  if (lm) {
    HIP_TRY(hipSetDevice(m->device));
    made = std::make_shared<TokenLm>();
    HIP_TRY(made->image.upload(lm->packed));                         // synchronous: the host graph may go afterwards
    made->dev = pfhip::lm_graph_dev(lm, made->image.p);
  }
  std::lock_guard<std::mutex> l(m->lm_mu);
  m->token_lm = made;
  return PFHIP_OK;
}

}  // extern "C"
