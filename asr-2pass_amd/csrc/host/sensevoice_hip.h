// `SenseVoiceSmallHip`, the sibling of `funasr::SenseVoiceSmall` (onnxruntime/src/sensevoice-small.{h,cpp}) behind the plug-in seam
// `class funasr::Model` (model.h:12-46), offline: the model the reference builds when the model directory's name contains
// MODEL_SVS (offline-stream.cpp:50-56).  Same two builds as paraformer_hip.h: inside the reference tree (-DPFHIP_WITH_FUNASR) it
// derives from the real funasr::Model + funasr::WfstDecodable; stand-alone from the small interfaces of paraformer_hip.h.
// Model widths and wiring underneath are recalled from upstream FunASR (no SenseVoice file was available).
#pragma once
#include <string>
#include <vector>

#include "paraformer_hip.h"

namespace funasr {

class SenseVoiceSmallHip : public ParaformerHipBase, public OnlineModelOwner
#ifdef PFHIP_WITH_FUNASR
    , public WfstDecodable
#endif
{
 public:
  SenseVoiceSmallHip() {}
  ~SenseVoiceSmallHip() override;

  // SenseVoiceSmall::InitAsr (sensevoice-small.cpp:22-56), the five-argument form offline-stream.cpp:89 calls.  am_model:
  // <dir>/model.onnx (or model_quant.onnx) with am.mvn and config.yaml, read by pfhip_read_model_files("sensevoice", ...) and cached
  // beside the source, or a container x.pfhip.bin of kind "sensevoice".  Exits on failure like the reference's (:48-51).
  void InitAsr(const std::string& am_model, const std::string& am_cmvn, const std::string& am_config, const std::string& token_file,
               int thread_num) override;
  // The 2-pass forms TpassStream calls on this model (tpass-stream.cpp:44-50, :76-77; sensevoice-small.cpp's nine-argument
  // InitAsr): the online encoder and decoder (a small online Paraformer) into a handle of their own with stream batching on, as
  // ParaformerHip's 2-pass InitAsr loads them, then the offline SenseVoice model with the offline directory's config and tokens.
  // am_cmvn is the ONLINE directory's am.mvn and serves both, as tpass-stream.cpp:72 passes it.
  void InitAsr(const std::string& am_model, const std::string& en_model, const std::string& de_model, const std::string& am_cmvn,
               const std::string& am_config, const std::string& token_file, const std::string& online_token_file, int thread_num,
               const std::string& online_config_file) override;
  void InitAsr(const std::string& am_model, const std::string& en_model, const std::string& de_model, const std::string& am_cmvn,
               const std::string& am_config, const std::string& token_file, const std::string& online_token_file, int thread_num) override;
  using ParaformerHipBase::InitAsr;        // the six-argument online-only form stays visible (empty in the base)
  // TpassStream calls InitLm when LM_DIR is set (tpass-stream.cpp:92-98): no search is built for this model, so the call returns
  // having loaded nothing and says so once
  void InitLm(const std::string& lm_file, const std::string& lm_config, const std::string& lex_file) override;
  void InitLm(const std::string& lm_file, const std::string& lm_config, const std::string& lex_file, const std::string& lm_units_path) override;
  // NOT InitLm and no TLG.fst: an ARPA n-gram over THIS MODEL'S TOKENS (tokens.json gives the strings) for the device search a
  // CtcPrefixDecoderHip decoder handle stands for (pfhip_set_token_lm; ParaformerHip::InitTokenLm says the rest).  Calls without such a
  // handle keep serving the greedy text.  false: nothing was loaded.
  bool InitTokenLm(const std::string& arpa_path, float scale = 1.0f, float token_bonus = 0.0f);
  // the online model ParaformerOnlineHip(this, chunk_size, MODEL_SVS) streams from
  pfhip_model* OnlineHandle() const override { return online_handle_; }
  std::string OnlineTokensToString(const std::vector<int>& ids) override { return OnlineIdsToString(online_vocab_, ids); }
  int OnlineSampleRate() const override { return online_handle_ ? pfhip_sample_rate(online_handle_) : asr_sample_rate_; }
  // The overload of model.h:33-34 (sensevoice-small.cpp:575-690).  Returns batch_in strings; the reference refuses batch_in != 1
  // (:577-580), here the utterances are packed, all with the call's svs_lang / svs_itn.  decoder_handle == nullptr: the text of
  // CTCSearch (:323-377), made on the host from the ids the device collapsed.  With a decoder handle the full log-prob rows of every
  // utterance are handed to `((Decoder*)decoder_handle)->Search(rows, n_rows, vocab)` — the search itself (CTCPrefixBeamSearch /
  // BeamSearch, :651-662) is not part of this path — and, when input_finished, FinalizeDecode() gives the text.
  // A decoder handle that is a CtcPrefixDecoderHip (ctc_prefix_decoder_hip.h; stand-alone build) is what the reference serves with
  // CTCPrefixBeamSearch (:392-440, :651-657): the search then runs on the device with the decoder's beams and hotword graph
  // (pfhip_svs_forward_beam), no log-prob row crosses to the host, and the text is made from the best ids — the pieces
  // concatenated, "▁" to " " (CtcFinalizeDecode), then the trailing-space rule of :428-436 on the language and ITN tags, which
  // are the arg-max of rows 0 and 3 (:413-420).  LastSearchIds() holds the best ids; with SetCtcTimestamps on they are aligned.
  // "" for an utterance without one full fbank window (:584-587) and for every item when the device call fails.
  std::vector<std::string> Forward(float** din, int* len, bool input_finished, std::string svs_lang = "auto", bool svs_itn = false,
                                   void* decoder_handle = nullptr, int batch_in = 1)
#ifdef PFHIP_WITH_FUNASR
      override
#endif
      ;
  using ParaformerHipBase::Forward;        // the Paraformer overloads stay visible (and keep their empty defaults)
  // the same on 16-bit PCM as the server receives it (pfhip_svs_forward_s16); not a virtual
  std::vector<std::string> ForwardPcm16(const int16_t* const* din, const int* len, bool input_finished, std::string svs_lang = "auto",
                                        bool svs_itn = false, void* decoder_handle = nullptr, int batch_in = 1);
  void StartUtterance() override {}
  void EndUtterance() override {}
  void Reset() override {}
  std::string Rescoring() override { return ""; }             // "Not Imp" in the reference too (:686-690)
  std::string GetLang() override { return language; }
  int GetAsrSampleRate() override { return asr_sample_rate_; }
  void SetBatchSize(int batch_size) override { batch_size_ = batch_size; }
  int GetBatchSize() override { return batch_size_; }
#ifdef PFHIP_WITH_FUNASR
  std::shared_ptr<fst::Fst<fst::StdArc>> GetLm() const override { return nullptr; }       // InitLm is out of scope for this model
  Vocab* GetVocab() const override { return vocab; }
  PhoneSet* GetPhoneSet() const override { return nullptr; }
  Vocab* GetLmVocab() const override { return nullptr; }
  Vocab* GetVocab() override { return vocab; }
  PhoneSet* GetPhoneSet() override { return nullptr; }
  Vocab* GetLmVocab() override { return nullptr; }
#endif
  // of the last Forward of the calling thread, per utterance: the kept ids (the four leading tags included), the row of the T + 4
  // sequence each kept run starts at, and exp(log-prob of that frame's arg-max)
  const std::vector<std::vector<int>>& LastTokenIds() const;
  const std::vector<std::vector<int>>& LastTokenFrames() const;
  const std::vector<std::vector<float>>& LastTokenConfidence() const;
  // per utterance the best token sequence of the device search of the calling thread's last Forward (text tokens only, no tags);
  // empty lists when that Forward ran no device search
  const std::vector<std::vector<int>>& LastSearchIds() const;
  // AlignTokens on LastSearchIds(): what Forward does for a CtcPrefixDecoderHip call when the switch is on
  bool AlignSearchTokens();
  HipVocab* GetHipVocab() const { return vocab; }
  // Token time spans by CTC forced alignment (pfhip_svs_align; an extension: the reference's SenseVoiceSmall returns no stamps).
  // Off (the default), Forward calls exactly what it always called.  On, a Forward WITHOUT a decoder handle (the text is the greedy
  // text) aligns the kept ids minus the four leading tags — the tokens of the text — right after the forward; with a
  // CtcPrefixDecoderHip the best ids of the device search are aligned; with any other decoder handle nothing is aligned, as that
  // search returns a string and no ids.  ms rule (the project's own): speech row t = row - 4 covers
  // [t F, (t + 1) F) with F = pfhip_lfr_frame_ms (60 ms), a token's span is [begin_t F, end_t F]; a caller that cut the audio into VAD
  // segments adds the segment's offset, as for the CIF stamps.  Not virtual, like every method added here.
  void SetCtcTimestamps(bool on) { ctc_stamps_ = on; }
  bool GetCtcTimestamps() const { return ctc_stamps_; }
  // Aligns ids of the caller's own (one list per utterance of the calling thread's last Forward, WITHOUT the four tags: a search
  // result it has tokenised, a transcript) against that Forward's rows and replaces LastTokenSpans / LastTokenStampsMs; false (and
  // both emptied) when the device call refuses them — bad ids, or another thread's Forward has taken the execution context since
  // (possible with more calling threads than PFHIP_INFLIGHT contexts: the result then simply has no spans).
  bool AlignTokens(const std::vector<std::vector<int>>& ids);
  // AlignTokens on the text tokens of the calling thread's last Forward (its kept ids behind the four tags): what Forward itself
  // does when the switch is on, for a caller that decides call by call (FunOfflineInferBuffer)
  bool AlignGreedyTokens();
  // of the last Forward (or AlignTokens) of the calling thread, per utterance: begin / end row pairs (rows of the T + 4 sequence like
  // LastTokenFrames, end exclusive) and [begin_ms, end_ms] pairs, two entries per aligned token; empty while the switch is off, with
  // a decoder handle, and for an utterance too short for its tokens
  const std::vector<std::vector<int>>& LastTokenSpans() const;
  const std::vector<std::vector<float>>& LastTokenStampsMs() const;
  void SetDevice(int device) { device_ = device; }
  pfhip_model* Handle() const { return handle_; }
  // CTCSearch's text step (:348-375) on kept ids; without a vocabulary the ids from the fifth on, space-separated
  std::string TokensToString(const std::vector<int>& ids) const;

  std::string language = "auto";

 private:
  std::vector<std::string> ForwardAny(const void* const* din, bool s16, const int* len, bool input_finished, const std::string& svs_lang,
                                      bool svs_itn, void* decoder_handle, int batch_in);
  pfhip_model* handle_ = nullptr;
  pfhip_model* online_handle_ = nullptr;
  HipVocab* online_vocab_ = nullptr;
  HipVocab* vocab = nullptr;
  int asr_sample_rate_ = 16000, device_ = 0, batch_size_ = 1;
  bool ctc_stamps_ = false;
};

}  // namespace funasr
