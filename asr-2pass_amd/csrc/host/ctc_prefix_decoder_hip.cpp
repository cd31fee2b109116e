// CtcPrefixDecoderHip: see ctc_prefix_decoder_hip.h.
#include "ctc_prefix_decoder_hip.h"

#include <algorithm>
#include <cctype>
#include <cstdio>

namespace funasr {
namespace {
const char kWordStart[] = "\xE2\x96\x81";      // "▁"

// SplitUTF8StringToChars (utf8-string.cpp): one string per code point, by the lead byte
std::vector<std::string> Utf8Chars(const std::string& s) {
  std::vector<std::string> out;
  for (size_t i = 0; i < s.size();) {
    const unsigned char c = (unsigned char)s[i];
    size_t n = 1;
    if ((c & 0xE0) == 0xC0) n = 2;
    else if ((c & 0xF0) == 0xE0) n = 3;
    else if ((c & 0xF8) == 0xF0) n = 4;
    n = std::min(n, s.size() - i);
    out.push_back(s.substr(i, n));
    i += n;
  }
  return out;
}
int Utf8Length(const std::string& s) { return (int)Utf8Chars(s).size(); }      // UTF8StringLength (utf8-string.cpp:120-136)
bool IsAlpha(const std::string& s) {                                             // utf8-string.cpp:138-145
  for (char ch : s)
    if (!std::isalpha((unsigned char)ch)) return false;
  return true;
}
std::string Trim(const std::string& s) {
  const char* ws = " \t\n\r\f\v";
  const size_t a = s.find_first_not_of(ws);
  return a == std::string::npos ? std::string() : s.substr(a, s.find_last_not_of(ws) - a + 1);
}
}  // namespace

CtcPrefixDecoderHip::CtcPrefixDecoderHip(HipVocab* vocab, float glob_beam, float lat_beam)
    : vocab_(vocab), first_beam_(static_cast<int>(glob_beam)), second_beam_(static_cast<int>(lat_beam)) {
  for (int i = 0; vocab_ && i < vocab_->Size(); ++i) token_id_.emplace(vocab_->Id2String(i), i);      // the first id of a string, as Find
}

CtcPrefixDecoderHip::~CtcPrefixDecoderHip() { UnloadHwsRes(); }

void CtcPrefixDecoderHip::UnloadHwsRes() {
  if (graph_) pfhip_ctx_graph_destroy(graph_);
  graph_ = nullptr;
}

bool CtcPrefixDecoderHip::TextToIds(const std::string& text, std::vector<int>* ids, std::vector<std::string>* words) const {
  const std::vector<std::string> chars = Utf8Chars(Trim(text));
  bool no_oov = true;
  for (size_t start = 0; start < chars.size();) {
    bool moved = false;
    for (size_t end = chars.size(); end > start && !moved; --end) {
      std::string word;
      for (size_t i = start; i < end; ++i) word += chars[i];
      if (word == " ") { start = end; moved = true; break; }
      if (IsAlpha(word)) word = kWordStart + word;
      const auto it = token_id_.find(word);
      if (it != token_id_.end()) {
        ids->push_back(it->second);
        if (words) words->push_back(word);
        start = end; moved = true; break;
      }
      if (end == start + 1) { ++start; no_oov = false; moved = true; break; }
    }
  }
  return no_oov;
}

int CtcPrefixDecoderHip::LoadHwsRes(int inc_bias, std::unordered_map<std::string, int>& hws_map) {
  (void)inc_bias;
  if (hws_map.empty() || !vocab_) return 0;
  std::vector<int32_t> ids;
  std::vector<int> n_ids;
  std::vector<float> weight;
  int taken = 0;
  for (const auto& hw : hws_map) {
    if (hw.first.size() > 100) continue;                             // max_context_length
    if (taken >= 5000) break;                                        // max_contexts
    std::vector<int> tok;
    std::vector<std::string> words;
    if (!TextToIds(hw.first, &tok, &words) || tok.empty()) continue; // an unknown piece: the hotword is skipped (:66-69)
    if (std::find(tok.begin(), tok.end(), 0) != tok.end()) continue; // id 0 is the graph's escape label (and this model's blank)
    for (size_t i = 0; i < tok.size(); ++i) {
      ids.push_back(tok[i]);
      weight.push_back((float)hw.second * (float)Utf8Length(words[i]));
    }
    n_ids.push_back((int)tok.size());
    ++taken;
  }
  if (taken == 0) return 0;
  pfhip_ctx_graph* g = nullptr;
  if (pfhip_ctx_graph_create(ids.data(), n_ids.data(), weight.data(), taken, vocab_->Size(), &g) != PFHIP_OK) {
    std::fprintf(stderr, "CtcPrefixDecoderHip::LoadHwsRes: the hotwords were refused (a non-finite score?): none loaded\n");
    return 0;
  }
  UnloadHwsRes();
  graph_ = g;
  return taken;
}

std::string CtcPrefixDecoderHip::IdsToText(const std::vector<int>& ids) const {
  std::string text;
  if (!vocab_) {
    for (size_t i = 0; i < ids.size(); ++i) text += (i ? " " : "") + std::to_string(ids[i]);
    return text;
  }
  for (int id : ids) text += vocab_->Id2String(id);
  const std::string from = kWordStart;
  for (size_t pos = 0; (pos = text.find(from, pos)) != std::string::npos; pos += 1) text.replace(pos, from.size(), " ");
  return text;
}

}  // namespace funasr
