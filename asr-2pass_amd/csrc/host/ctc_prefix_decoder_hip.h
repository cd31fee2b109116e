// `CtcPrefixDecoderHip`, the sibling of `funasr::CtcPrefixDecoder` (onnxruntime/src/ctc-prefix-decoder.{h,cpp}): the per-connection
// decoder object a server creates when no LM is loaded (funasrruntime.cpp:836-894).  It holds what the search needs — the two beam
// sizes and the connection's hotwords as a context graph — and no search of its own: SenseVoiceSmallHip::Forward recognises the class
// behind its decoder handle and runs the search on the device (pfhip_svs_forward_beam), so no log-prob row crosses to the host.
// Any other Decoder keeps being handed the full rows.  Stand-alone build only: inside the reference tree the servers keep creating
// the reference's own CtcPrefixDecoder (INTEGRATION.md says what one line would change).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "paraformer_hip.h"

namespace funasr {

class CtcPrefixDecoderHip : public Decoder {
 public:
  // the reference's casts (ctc-prefix-decoder.cpp:27-34): first beam = (int)glob_beam, second beam = (int)lat_beam.  vocab may be
  // null: hotwords then cannot be loaded and the text is the ids.
  CtcPrefixDecoderHip(HipVocab* vocab, float glob_beam, float lat_beam);
  ~CtcPrefixDecoderHip() override;
  CtcPrefixDecoderHip(const CtcPrefixDecoderHip&) = delete;
  CtcPrefixDecoderHip& operator=(const CtcPrefixDecoderHip&) = delete;
  // CtcPrefixDecoder::LoadHwsRes (:74-98): hotword text -> score.  A text becomes token ids by the greedy longest match of
  // ContextGraph::SplitUTF8StringToWords (context_graph.cpp:120-159; alphabetic words get the "▁" prefix, spaces are skipped), a
  // token weighs score x the UTF-8 length of its string (:76-77; the incremental score is 0), a hotword with an unknown piece or
  // longer than 100 bytes is skipped, at most 5000 are taken.  inc_bias is stored in the reference's config and read nowhere; so
  // here.  An empty map changes nothing, as there.  Returns the hotwords that entered the graph.
  int LoadHwsRes(int inc_bias, std::unordered_map<std::string, int>& hws_map);
  void UnloadHwsRes();
  int FirstBeam() const { return first_beam_; }
  int SecondBeam() const { return second_beam_; }
  const pfhip_ctx_graph* Graph() const { return graph_; }
  // the text step on the host (true: every piece is in the vocabulary): the pieces of SplitUTF8StringToWords as ids
  bool TextToIds(const std::string& text, std::vector<int>* ids, std::vector<std::string>* words = nullptr) const;
  // UpdateResult + CtcFinalizeDecode (:265-278, :301-313): the pieces concatenated, "▁" replaced by " "
  std::string IdsToText(const std::vector<int>& ids) const;

 private:
  HipVocab* vocab_;
  int first_beam_, second_beam_;
  pfhip_ctx_graph* graph_ = nullptr;
  std::unordered_map<std::string, int> token_id_;
};

}  // namespace funasr
