// SenseVoiceSmallHip: see sensevoice_hip.h.
#include "sensevoice_hip.h"
#ifndef PFHIP_WITH_FUNASR
#include "ctc_prefix_decoder_hip.h"
#endif

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace funasr {
namespace {
thread_local std::vector<std::vector<int>> tl_svs_ids, tl_svs_frames, tl_svs_search;
thread_local std::vector<std::vector<float>> tl_svs_conf;
thread_local std::vector<std::vector<int>> tl_svs_spans;
thread_local std::vector<std::vector<float>> tl_svs_stamps;

int Knob(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : dflt;
}
}  // namespace

SenseVoiceSmallHip::~SenseVoiceSmallHip() {
  if (handle_) pfhip_destroy(handle_);
  if (online_handle_) pfhip_destroy(online_handle_);
  delete vocab;
  delete online_vocab_;
}

// 2pass: online first, then the offline model with the offline directory's config and tokens (the order of paraformer.cpp:134-154)
void SenseVoiceSmallHip::InitAsr(const std::string& am_model, const std::string& en_model, const std::string& de_model,
                                 const std::string& am_cmvn, const std::string& am_config, const std::string& token_file,
                                 const std::string& online_token_file, int thread_num, const std::string& online_config_file) {
  if (online_handle_) { pfhip_destroy(online_handle_); online_handle_ = nullptr; }
  online_handle_ = LoadOnlineModelHip(en_model, de_model, am_cmvn, online_config_file, device_);
  delete online_vocab_;
  online_vocab_ = LoadVocabHip(online_token_file);
  InitAsr(am_model, am_cmvn, am_config, token_file, thread_num);
}
void SenseVoiceSmallHip::InitAsr(const std::string& am_model, const std::string& en_model, const std::string& de_model,
                                 const std::string& am_cmvn, const std::string& am_config, const std::string& token_file,
                                 const std::string& online_token_file, int thread_num) {
  InitAsr(am_model, en_model, de_model, am_cmvn, am_config, token_file, online_token_file, thread_num, am_config);
}
void SenseVoiceSmallHip::InitLm(const std::string& lm_file, const std::string& lm_config, const std::string& lex_file) {
  InitLm(lm_file, lm_config, lex_file, "");
}
void SenseVoiceSmallHip::InitLm(const std::string& lm_file, const std::string&, const std::string&, const std::string&) {
  std::fprintf(stderr, "SenseVoiceSmallHip::InitLm: %s is not loaded (no WFST / LM search for this model: the greedy text is served)\n",
               lm_file.c_str());
}

bool SenseVoiceSmallHip::InitTokenLm(const std::string& arpa_path, float scale, float token_bonus) {
  return LoadTokenLmHip(handle_, vocab, arpa_path, scale, token_bonus);
}

void SenseVoiceSmallHip::InitAsr(const std::string& am_model, const std::string& am_cmvn, const std::string& am_config,
                                 const std::string& token_file, int thread_num) {
  (void)thread_num;
  if (handle_) { pfhip_destroy(handle_); handle_ = nullptr; }
  pfhip_container* c = nullptr;
  pfhip_status st = pfhip_read_model_files("sensevoice", am_model.c_str(), nullptr, nullptr, am_cmvn.c_str(), am_config.c_str(), &c);
  if (st == PFHIP_OK) {
    size_t bytes = 0;
    const float* blob = pfhip_container_blob(c, &bytes);
    st = pfhip_create_from_memory(blob, bytes, pfhip_container_manifest(c), device_, &handle_);
    pfhip_container_free(c);
  }
  if (st == PFHIP_OK && !pfhip_is_ctc(handle_)) {
    std::fprintf(stderr, "Error when load am hip model: %s is not a SenseVoice model\n", am_model.c_str());
    std::exit(-1);
  }
  if (st != PFHIP_OK) {                                          // sensevoice-small.cpp:48-51
    std::fprintf(stderr, "Error when load am hip model: %s\n", pfhip_last_error());
    std::exit(-1);
  }
  asr_sample_rate_ = pfhip_sample_rate(handle_);
  // the decoder threads' concurrent Forward calls go to PFHIP_INFLIGHT execution contexts over the one weight set (merging them
  // into packed launches is not built for this model)
  const int inflight = Knob("PFHIP_INFLIGHT", 3);
  if (inflight > 1 && pfhip_set_inflight(handle_, inflight) != PFHIP_OK)
    std::fprintf(stderr, "SenseVoiceSmallHip::InitAsr: %s (one forward at a time)\n", pfhip_last_error());
  delete vocab;
  vocab = nullptr;
  if (!token_file.empty()) {                                     // sensevoice-small.cpp:53
#ifdef PFHIP_WITH_FUNASR
    vocab = new Vocab(token_file.c_str());
#else
    vocab = new HipVocab();
    if (!vocab->Load(token_file.c_str())) { delete vocab; vocab = nullptr; }
#endif
  }
  const int warm_s = Knob("PFHIP_WARMUP_SECONDS", 30);
  if (warm_s > 0 && pfhip_warm_up(handle_, batch_size_ > 0 ? batch_size_ : 1, warm_s * asr_sample_rate_) != PFHIP_OK)
    std::fprintf(stderr, "SenseVoiceSmallHip::InitAsr: warm-up failed: %s\n", pfhip_last_error());
}

// sensevoice-small.cpp:344-375.  The reference reads tokens[3] after checking only size() >= 3; four kept ids are required here.
std::string SenseVoiceSmallHip::TokensToString(const std::vector<int>& ids) const {
  std::string text;
  if (!vocab) {
    for (size_t i = 4; i < ids.size(); ++i) text += (i > 4 ? " " : "") + std::to_string(ids[i]);
    return text;
  }
  const std::string mark = "\xE2\x96\x81";                       // "▁"
  std::string lang, itn;
  if (ids.size() >= 4) { lang = vocab->Id2String(ids[0]); itn = vocab->Id2String(ids[3]); }
  for (size_t i = 4; i < ids.size(); ++i) {
    const std::string word = vocab->Id2String(ids[i]);
    if (word.find(mark) != std::string::npos) text += " " + (word.size() >= 3 ? word.substr(3) : std::string());
    else text += word;
  }
  if (itn == "<|withitn|>") {
    if (lang == "<|en|>") text += " ";                           // for english, a space at the end
  } else {
    text += " ";                                                 // without itn, no punctuation: a space at the end
  }
  return text;
}

std::vector<std::string> SenseVoiceSmallHip::Forward(float** din, int* len, bool input_finished, std::string svs_lang, bool svs_itn,
                                                     void* decoder_handle, int batch_in) {
  return ForwardAny(reinterpret_cast<const void* const*>(din), false, len, input_finished, svs_lang, svs_itn, decoder_handle, batch_in);
}
std::vector<std::string> SenseVoiceSmallHip::ForwardPcm16(const int16_t* const* din, const int* len, bool input_finished, std::string svs_lang,
                                                          bool svs_itn, void* decoder_handle, int batch_in) {
  return ForwardAny(reinterpret_cast<const void* const*>(din), true, len, input_finished, svs_lang, svs_itn, decoder_handle, batch_in);
}

std::vector<std::string> SenseVoiceSmallHip::ForwardAny(const void* const* din, bool s16, const int* len, bool input_finished,
                                                        const std::string& svs_lang, bool svs_itn, void* decoder_handle, int batch_in) {
  std::vector<std::string> results(batch_in > 0 ? batch_in : 0);
  tl_svs_ids.assign(results.size(), {});
  tl_svs_frames.assign(results.size(), {});
  tl_svs_conf.assign(results.size(), {});
  tl_svs_search.assign(results.size(), {});
  tl_svs_spans.clear();
  tl_svs_stamps.clear();
  if (batch_in <= 0 || !handle_) return results;
  const int B = batch_in, V = pfhip_vocab_size(handle_);
  Decoder* decoder = static_cast<Decoder*>(decoder_handle);
#ifndef PFHIP_WITH_FUNASR
  CtcPrefixDecoderHip* search = dynamic_cast<CtcPrefixDecoderHip*>(decoder);      // the device search instead of the hand-off
  if (search) decoder = nullptr;
#else
  void* search = nullptr;
#endif
  // rows per utterance are known before the call: ceil(frames / 6) + 4 (sensevoice-small.cpp:520-560 is Paraformer's LfrCmvn)
  std::vector<int> rows(B);
  int max_rows = 1;
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    const int frames = len[b] < 400 ? 0 : 1 + (len[b] - 400) / 160;
    const int T = (frames + 5) / 6;
    rows[b] = T > 0 ? T + 4 : 0;
    max_rows = std::max(max_rows, rows[b]);
    total += (size_t)rows[b];
  }
  const std::vector<int32_t> lid(B, pfhip_svs_lid(svs_lang.c_str())), textnorm(B, svs_itn ? 14 : 15);      // :597-605
  std::vector<int32_t> ids((size_t)B * max_rows), frames((size_t)B * max_rows), num(B, 0), frame_len(B, 0);
  std::vector<float> tok_logp((size_t)B * max_rows), logp(decoder ? total * (size_t)V : 0);
  pfhip_svs_out out{};
  out.ids = ids.data(); out.token_num = num.data(); out.max_tokens = max_rows;
  out.tok_frame = frames.data(); out.tok_logp = tok_logp.data(); out.frame_len = frame_len.data();
  if (decoder) { out.logp = logp.data(); out.logp_cap_floats = logp.size(); }
  std::vector<int32_t> frame_ids, b_nhyp, b_ids, b_ntok;
  pfhip_status st;
#ifndef PFHIP_WITH_FUNASR
  if (search) {
    frame_ids.assign(std::max<size_t>(total, 1), 0);
    b_nhyp.assign(B, 0); b_ntok.assign(B, 0); b_ids.assign((size_t)B * max_rows, 0);
    out.frame_ids = frame_ids.data();
    const pfhip_svs_beam_opts opts{search->FirstBeam(), search->SecondBeam(), 1, search->Graph()};
    pfhip_svs_beam_out bo{};
    bo.n_hyp = b_nhyp.data(); bo.ids = b_ids.data(); bo.n_tokens = b_ntok.data(); bo.max_tokens = max_rows;
    st = s16 ? pfhip_svs_forward_beam_s16(handle_, reinterpret_cast<const int16_t* const*>(din), len, B, lid.data(), textnorm.data(), &out, &opts, &bo)
             : pfhip_svs_forward_beam(handle_, reinterpret_cast<const float* const*>(din), len, B, lid.data(), textnorm.data(), &out, &opts, &bo);
  } else
#endif
  st = s16 ? pfhip_svs_forward_s16(handle_, reinterpret_cast<const int16_t* const*>(din), len, B, lid.data(), textnorm.data(), &out)
                              : pfhip_svs_forward(handle_, reinterpret_cast<const float* const*>(din), len, B, lid.data(), textnorm.data(), &out);
  if (st != PFHIP_OK) {                                          // the reference logs and returns "" (:664-667)
    std::fprintf(stderr, "SenseVoiceSmallHip::Forward: %s\n", pfhip_last_error());
    return results;
  }
  size_t row0 = 0;
  for (int b = 0; b < B; ++b) {
    const size_t at = (size_t)b * max_rows;
    tl_svs_ids[b].assign(ids.begin() + at, ids.begin() + at + num[b]);
    tl_svs_frames[b].assign(frames.begin() + at, frames.begin() + at + num[b]);
    for (int t = 0; t < num[b]; ++t) tl_svs_conf[b].push_back(std::exp(tok_logp[at + t]));
    if (frame_len[b] == 0) { results[b] = ""; continue; }        // :584-587
#ifndef PFHIP_WITH_FUNASR
    if (search) {                                                // CTCPrefixBeamSearch's text (:392-440) from the device's best ids
      if (b_nhyp[b] > 0) tl_svs_search[b].assign(b_ids.begin() + at, b_ids.begin() + at + b_ntok[b]);
      std::string text = search->IdsToText(tl_svs_search[b]);
      const std::string lang = vocab ? vocab->Id2String(frame_ids[row0]) : "", itn = vocab ? vocab->Id2String(frame_ids[row0 + 3]) : "";
      if (itn == "<|withitn|>") {
        if (lang == "<|en|>") text += " ";
      } else {
        text += " ";
      }
      results[b] = text;
    } else
#endif
    if (decoder) {                                               // the caller's search gets the rows; between items it is restarted
      if (b > 0) { decoder->EndUtterance(); decoder->StartUtterance(); }
      results[b] = decoder->Search(logp.data() + row0 * (size_t)V, frame_len[b], V);
      if (input_finished) results[b] = decoder->FinalizeDecode();
    } else {
      results[b] = TokensToString(tl_svs_ids[b]);
    }
    row0 += (size_t)frame_len[b];
  }
  if (ctc_stamps_ && search) AlignSearchTokens();
  else if (ctc_stamps_ && !decoder) AlignGreedyTokens();
  return results;
}

bool SenseVoiceSmallHip::AlignSearchTokens() { return AlignTokens(std::vector<std::vector<int>>(tl_svs_search)); }

bool SenseVoiceSmallHip::AlignGreedyTokens() {                     // the greedy text's tokens: the kept ids behind the four tags
  std::vector<std::vector<int>> toks(tl_svs_ids.size());
  for (size_t b = 0; b < toks.size(); ++b)
    if (tl_svs_ids[b].size() > 4) toks[b].assign(tl_svs_ids[b].begin() + 4, tl_svs_ids[b].end());
  return AlignTokens(toks);
}

bool SenseVoiceSmallHip::AlignTokens(const std::vector<std::vector<int>>& ids) {
  tl_svs_spans.clear();
  tl_svs_stamps.clear();
  const int B = (int)ids.size();
  if (!handle_ || B == 0) return false;
  int cap = 1;
  std::vector<const int32_t*> ptr(B);
  std::vector<int> n(B);
  for (int b = 0; b < B; ++b) {
    ptr[b] = ids[b].data(); n[b] = (int)ids[b].size();
    cap = std::max(cap, n[b]);
  }
  std::vector<int32_t> begin((size_t)B * cap), end((size_t)B * cap);
  std::vector<float> score(B);
  pfhip_svs_align_out out{};
  out.tok_begin = begin.data(); out.tok_end = end.data(); out.score = score.data(); out.max_tokens = cap;
  if (pfhip_svs_align(handle_, ptr.data(), n.data(), B, &out) != PFHIP_OK) {
    std::fprintf(stderr, "SenseVoiceSmallHip::AlignTokens: %s\n", pfhip_last_error());
    return false;
  }
  const float F = (float)pfhip_lfr_frame_ms(handle_);
  tl_svs_spans.assign(B, {});
  tl_svs_stamps.assign(B, {});
  for (int b = 0; b < B; ++b) {
    if (!(score[b] > -INFINITY)) continue;                         // fewer rows than the tokens need: no spans for this utterance
    for (int j = 0; j < n[b]; ++j) {
      const int tb = begin[(size_t)b * cap + j], te = end[(size_t)b * cap + j];
      tl_svs_spans[b].push_back(tb); tl_svs_spans[b].push_back(te);
      tl_svs_stamps[b].push_back((float)(tb - 4) * F); tl_svs_stamps[b].push_back((float)(te - 4) * F);
    }
  }
  return true;
}

const std::vector<std::vector<int>>& SenseVoiceSmallHip::LastTokenIds() const { return tl_svs_ids; }
const std::vector<std::vector<int>>& SenseVoiceSmallHip::LastTokenFrames() const { return tl_svs_frames; }
const std::vector<std::vector<int>>& SenseVoiceSmallHip::LastSearchIds() const { return tl_svs_search; }
const std::vector<std::vector<float>>& SenseVoiceSmallHip::LastTokenConfidence() const { return tl_svs_conf; }
const std::vector<std::vector<int>>& SenseVoiceSmallHip::LastTokenSpans() const { return tl_svs_spans; }
const std::vector<std::vector<float>>& SenseVoiceSmallHip::LastTokenStampsMs() const { return tl_svs_stamps; }

}  // namespace funasr
