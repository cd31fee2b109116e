#include "funasrruntime_hip.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <mutex>
#include <numeric>
#include <sstream>

#include "ct_transformer_hip.h"
#include "fsmn_vad_hip.h"
#include "paraformer_hip.h"
#include "ctc_prefix_decoder_hip.h"
#include "sensevoice_hip.h"
#include "tpass_audio.h"

#include <atomic>

namespace {

struct OfflineStreamHip {
  funasr::ParaformerHip asr;
  std::unique_ptr<funasr::SenseVoiceSmallHip> svs;      // model type MODEL_SVS (offline-stream.cpp:50-56): `asr` stays unloaded
  std::unique_ptr<funasr::FsmnVadHip> vad;      // complete files only (InferFile): no per-file state, no lock
  std::unique_ptr<funasr::PuncModelHipBase> punc;      // OfflineStream::punc_handle (offline-stream.cpp:105-129)
  std::atomic<bool> svs_ctc_stamps{false};      // FunOfflineSetCtcStamps: decided per call (a call with a decoder attached aligns nothing)
};

struct RecogResult {               // funasr::FUNASR_RECOG_RESULT (com-define.h)
  std::string msg, stamp, tpass_msg;
  float snippet_time = 0.f;
  std::vector<std::vector<int>> seg_ids;
  std::vector<std::pair<int, int>> segs;
  std::vector<int> online_ids;       // ids the streaming chunks of this call emitted (inspection)
  std::vector<float> confidence;     // FunASRGetTokenConfidence (FunOfflineSetNbest / FunTpassSetNbest: the second-pass text)
  std::vector<float> online_conf;    // FunASRGetOnlineConfidence, FunASRGetOnlineFireMs: parallel to online_ids (FunTpassSetNbest)
  std::vector<int> online_fire_ms;
};

bool ReadAll(const std::string& path, std::vector<char>& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  f.seekg(0, std::ios::end);
  out.resize((size_t)f.tellg());
  f.seekg(0);
  f.read(out.data(), (std::streamsize)out.size());
  return (bool)f;
}

constexpr int kSegSample = 16;      // samples per ms at 16 kHz (audio.cpp: seg_sample = MODEL_SAMPLE_RATE / 1000)

// Audio::CutSplit (audio.cpp:1172-1240): the FSMN-VAD scores the whole buffer in one pass (it is causal: the reference's
// 1-s slices carry the same cache state), the end-point detector runs on the host, segments come back in ms.
// The n samples come as floats (pcm) or as 16-bit PCM (pcm16), never both: the detector's decibel track is computed on the device
// from whichever was sent there, so 16-bit input is not converted on the host.  Nothing is shared between calls — the configuration
// travels with the call, the detector is the call's own, every file is scored against fresh caches — so the decoder threads run
// this at once and the VAD handle scores their files in company.
bool CutSplit(OfflineStreamHip* os, const float* pcm, const int16_t* pcm16, int n, int vad_tail_sil, int vad_max_len,
              std::vector<std::pair<int, int>>& frames, std::vector<int>& index_vector) {
  frames.clear();
  index_vector.clear();
  const std::vector<std::vector<int>> segs = os->vad->InferFile(pcm16 ? nullptr : pcm, pcm16, n, vad_tail_sil, vad_max_len);
  for (const std::vector<int>& sg : segs) frames.emplace_back(sg[0] * kSegSample, std::min(sg[1] * kSegSample, n));
  index_vector.resize(frames.size());
  std::iota(index_vector.begin(), index_vector.end(), 0);
  // audio.cpp:1226-1239: queue by increasing length (ties keep time order)
  std::stable_sort(index_vector.begin(), index_vector.end(), [&](int a, int b) {
    return frames[a].second - frames[a].first < frames[b].second - frames[b].first;
  });
  return true;
}

// Audio::FetchDynamic (audio.cpp:1052-1108): pops one batch off the front of `queue` (positions into `order`)
int FetchDynamic(const std::vector<std::pair<int, int>>& frames, const std::vector<int>& order, size_t& head, int batch_size,
                 std::vector<int>& batch) {
  const long max_acc = 300L * 1000 * kSegSample, max_sent = 60L * 1000 * kSegSample;
  batch.clear();
  long bs_acc = 0, max_len = 0;
  const int max_batch = (int)std::min<size_t>((size_t)batch_size, order.size() - head);
  for (int i = 0; i < max_batch; ++i) {
    const auto& fr = frames[order[head]];
    const long length = fr.second - fr.first;
    if (length >= max_sent) {
      if (bs_acc == 0) { ++bs_acc; batch.push_back(order[head++]); }
      break;
    }
    max_len = std::max(max_len, length);
    if (max_len * (bs_acc + 1) > max_acc) break;
    ++bs_acc;
    batch.push_back(order[head++]);
  }
  return (int)batch.size();
}

}  // namespace

namespace {
bool FileExists(const std::string& path) { return (bool)std::ifstream(path); }
std::string PathAppend(const std::string& dir, const std::string& name) { return dir.empty() || dir.back() == '/' ? dir + name : dir + "/" + name; }
bool IsTrue(std::map<std::string, std::string>& model_path, const char* key) { return model_path.count(key) && model_path[key] == "true"; }
// a directory converted ahead of time holds no model.onnx; the loader finds its container from the ONNX name
bool HasContainer(const std::string& dir, const char* legacy) {
  return FileExists(PathAppend(dir, "model.pfhip.bin")) || FileExists(PathAppend(dir, std::string(legacy) + ".pfhip.bin"));
}
// the VAD block both stream classes open with (offline-stream.cpp:6-29, tpass-stream.cpp:6-29)
std::unique_ptr<funasr::FsmnVadHip> MakeVad(std::map<std::string, std::string>& model_path, int thread_num) {
  if (!model_path.count(VAD_DIR) || model_path[VAD_DIR].empty()) return nullptr;
  const std::string dir = model_path[VAD_DIR];
  const std::string vad_model_path = PathAppend(dir, IsTrue(model_path, VAD_QUANT) ? QUANT_MODEL_NAME : MODEL_NAME);
  const std::string vad_cmvn_path = PathAppend(dir, VAD_CMVN_NAME), vad_config_path = PathAppend(dir, VAD_CONFIG_NAME);
  if (!HasContainer(dir, "vad") && (!FileExists(vad_model_path) || !FileExists(vad_cmvn_path) || !FileExists(vad_config_path))) {
    std::fprintf(stderr, "VAD model file is not exist, skip load vad model.\n");
    return nullptr;
  }
  std::unique_ptr<funasr::FsmnVadHip> vad(new funasr::FsmnVadHip());
  vad->InitVad(vad_model_path, vad_cmvn_path, vad_config_path, thread_num);      // exits on failure
  return vad;
}
}  // namespace

// OfflineStream::OfflineStream (offline-stream.cpp:4-129) on the HIP plug-ins, call for call
FUNASR_HANDLE FunOfflineInit(std::map<std::string, std::string>& model_path, int thread_num, bool use_gpu, int batch_size) {
  auto os = std::make_unique<OfflineStreamHip>();
  os->vad = MakeVad(model_path, thread_num);
  if (model_path.count(MODEL_DIR)) {
    const std::string dir = model_path[MODEL_DIR];
    if (dir.find(MODEL_SVS) != std::string::npos) {                              // :50-56: the directory's name picks the model
      os->svs.reset(new funasr::SenseVoiceSmallHip());
      os->svs->SetBatchSize(batch_size);
      std::string token_path = model_path.count(TOKEN_PATH_KEY) ? model_path[TOKEN_PATH_KEY] : PathAppend(dir, TOKEN_PATH);
      if (!FileExists(token_path)) token_path.clear();
      os->svs->InitAsr(PathAppend(dir, IsTrue(model_path, QUANTIZE) ? QUANT_MODEL_NAME : MODEL_NAME), PathAppend(dir, AM_CMVN_NAME),
                       PathAppend(dir, AM_CONFIG_NAME), token_path, thread_num);   // :89, exits on failure
    } else {
    os->asr.SetBatchSize(batch_size);                                            // :41 (before InitAsr)
    const std::string hw_cpu_model_path = PathAppend(dir, MODEL_EB_NAME), hw_gpu_model_path = PathAppend(dir, TORCH_MODEL_EB_NAME);
    const std::string seg_dict_path = PathAppend(dir, MODEL_SEG_DICT);
    if (FileExists(hw_cpu_model_path)) {                                         // :63-67 if model_eb.onnx exist, hotword enabled
      os->asr.InitHwCompiler(hw_cpu_model_path, thread_num);
      os->asr.InitSegDict(seg_dict_path);
    }
    if (use_gpu && FileExists(hw_gpu_model_path)) {                              // :68-72
      os->asr.InitHwCompiler(hw_gpu_model_path, thread_num);
      os->asr.InitSegDict(seg_dict_path);
    }
    std::string am_model_path = PathAppend(dir, IsTrue(model_path, QUANTIZE) ? QUANT_MODEL_NAME : MODEL_NAME);      // :74-77
    if (use_gpu) am_model_path = PathAppend(dir, TORCH_MODEL_NAME);              // :79-84 (the ONNX file beside it is read)
    std::string token_path = model_path.count(TOKEN_PATH_KEY) ? model_path[TOKEN_PATH_KEY] : PathAppend(dir, TOKEN_PATH);
    if (!FileExists(token_path)) token_path.clear();                             // harness runs on synthetic models: ids as text
    os->asr.InitAsr(am_model_path, PathAppend(dir, AM_CMVN_NAME), PathAppend(dir, AM_CONFIG_NAME), token_path, thread_num);   // :89, exits on failure
    }
  }
  if (model_path.count(PUNC_DIR) && !model_path[PUNC_DIR].empty())               // :105-129, always CTTransformer here
    os->punc.reset(funasr::CreatePuncModelHip(model_path[PUNC_DIR], thread_num, false, IsTrue(model_path, PUNC_QUANT)));
  return os.release();
}

// Audio::LoadPcmwav / LoadPcmwavOnline (audio.cpp:787-857): s16 LE -> f32 / 32768, then Audio::WavResample (:259-284) when the
// caller's rate is not the model's — on the GPU (pfhip_resample), a fresh resampler with flush per buffer as the reference builds
// one per call.  False for a rate the resampler refuses.
// The 16-bit samples of a little-endian s16 buffer, host-endian and 2-byte aligned: the caller's own bytes where they already are
// that (every supported host is little-endian), else a copy in `store`.
static const int16_t* Pcm16View(const char* buf, int n, std::vector<int16_t>& store) {
  const uint16_t probe = 1;
  const bool little = *reinterpret_cast<const uint8_t*>(&probe) == 1;
  if (little && (reinterpret_cast<uintptr_t>(buf) & 1) == 0) return reinterpret_cast<const int16_t*>(buf);
  store.resize((size_t)n);
  const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
  for (int i = 0; i < n; ++i) store[i] = (int16_t)((b[2 * i + 1] << 8) | b[2 * i]);
  return store.data();
}

static bool LoadPcm(pfhip_model* m, const char* buf, int n_len, int sampling_rate, std::vector<float>& out) {
  const int n = n_len / 2;
  std::vector<float> pcm((size_t)n);
  const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
  for (int i = 0; i < n; ++i) pcm[i] = (float)(int16_t)((b[2 * i + 1] << 8) | b[2 * i]) / 32768.f;
  const int fs_out = pfhip_sample_rate(m);
  if (sampling_rate == fs_out) { out.swap(pcm); return true; }
  const int64_t n_out = pfhip_resample_len(sampling_rate, fs_out, n);
  if (n_out < 0 || n_out > INT32_MAX) return false;
  out.assign((size_t)std::max<int64_t>(n_out, 1), 0.f);
  const float* in[1] = {pcm.data()};
  float* dst[1] = {out.data()};
  const int cap = (int)out.size();
  int got = 0;
  if (pfhip_resample(m, in, &n, 1, sampling_rate, dst, &cap, &got) != PFHIP_OK) return false;
  out.resize((size_t)got);
  return true;
}

FUNASR_RESULT FunOfflineInferBuffer(FUNASR_HANDLE handle, const char* sz_buf, int n_len, FUNASR_MODE mode, QM_CALLBACK fn_callback,
                                    const std::vector<std::vector<float>>& hw_emb, int sampling_rate, std::string wav_format,
                                    bool itn, int vad_tail_sil, int vad_max_len, FUNASR_DEC_HANDLE dec_handle, std::string svs_lang,
                                    bool svs_itn) {
  (void)mode; (void)itn;
  OfflineStreamHip* os = static_cast<OfflineStreamHip*>(handle);
  if (!os || !sz_buf) return nullptr;
  funasr::SenseVoiceSmallHip* svs = os->svs.get();      // funasrruntime.cpp:265-266: the model type routes the Forward call
  // FunOfflineSetCtcStamps: the spans of the greedy text's tokens.  With a decoder attached the text is a search's, which returns a
  // string and no ids to align: the stamps stay empty
  // A CtcPrefixDecoderHip (FunASRCtcDecoderInit) selects the device search: its handle goes through to the adapter, and its best
  // ids ARE there to align.  Any other decoder handle keeps what it had for this model: it is not passed on.
  funasr::CtcPrefixDecoderHip* search = svs ? dynamic_cast<funasr::CtcPrefixDecoderHip*>(static_cast<funasr::Decoder*>(dec_handle)) : nullptr;
  const bool svs_stamps = svs && os->svs_ctc_stamps.load() && (!dec_handle || search);
  // a Paraformer is handed such a handle too (hotwords for any Paraformer); any other decoder handle is not passed on, as before
  funasr::Decoder* const bias_dec = svs ? nullptr : dynamic_cast<funasr::CtcPrefixDecoderHip*>(static_cast<funasr::Decoder*>(dec_handle));
  if (wav_format != "pcm" && wav_format != "PCM") return nullptr;      // the reference decodes other containers with ffmpeg
  // Audio::LoadPcmwav (audio.cpp:787-819); from here on samples, segments and stamps are at the model's rate (GetTimeLen
  // divides by dest_sample_rate, audio.cpp:254-257).
  // The acoustic model (and the VAD network) take the caller's 16-bit samples as they are:
  //   * at the model's rate, every segment is a range of the caller's buffer (ParaformerHip::ForwardPcm16) and no float copy of the
  //     file is made, with or without a VAD: the end-point detector's decibel track comes back from the device as frame energies;
  //   * at another rate WITHOUT a VAD the one segment is the whole buffer: it goes to the device as s16 and is resampled there
  //     (pfhip_offline_forward_rate_s16), no float copy at all;
  //   * at another rate WITH a VAD the segments are ranges of the RESAMPLED waveform, which is on the host as floats (LoadPcm):
  //     that path stays on floats, and its VAD takes the energy form as well.
  // FunOfflineSetNbest and FunOfflineSetCifStamps change none of this: their calls take 16-bit samples and a sample rate too
  // (pfhip_offline_forward_nbest_s16, pfhip_offline_forward_detail_s16).
  const int model_rate = svs ? svs->GetAsrSampleRate() : os->asr.GetAsrSampleRate();
  const int n_in = n_len / 2;
  const bool same_rate = sampling_rate == model_rate;
  const bool use16 = same_rate || (!os->vad && !svs);      // SenseVoice has no call at another rate: resampled through LoadPcm
  std::vector<int16_t> store16;
  const int16_t* pcm16 = use16 ? Pcm16View(sz_buf, n_in, store16) : nullptr;
  std::vector<float> pcm;
  int n;
  if (use16 && !same_rate) {                         // whole buffer, resampled on the device
    const int64_t n_rs = pfhip_resample_len(sampling_rate, model_rate, n_in);
    if (n_rs < 0 || n_rs > INT32_MAX) {
      std::fprintf(stderr, "FunOfflineInferBuffer: unsupported sample rate %d\n", sampling_rate);
      return nullptr;
    }
    n = (int)n_rs;
  } else if (use16) {
    n = n_in;
  } else {
    if (!LoadPcm(svs ? svs->Handle() : os->asr.Handle(), sz_buf, n_len, sampling_rate, pcm)) {
      std::fprintf(stderr, "FunOfflineInferBuffer: %s\n", pfhip_last_error());
      return nullptr;
    }
    n = (int)pcm.size();
  }
  auto res = std::make_unique<RecogResult>();
  res->snippet_time = (float)n / (float)model_rate;
  if (n == 0) return res.release();
  std::vector<int> index_vector = {0};
  res->segs.assign(1, {0, n});
  if (os->vad) {
    if (!CutSplit(os, pcm.data(), pcm16, n, vad_tail_sil, vad_max_len, res->segs, index_vector)) {
      std::fprintf(stderr, "FunOfflineInferBuffer: %s\n", pfhip_last_error());
      return res.release();
    }
  }
  std::vector<std::string> msgs(index_vector.size());
  std::vector<std::vector<float>> spans(index_vector.size()), conf(index_vector.size()), svs_ms(index_vector.size());
  res->seg_ids.assign(index_vector.size(), {});
  size_t head = 0, msg_idx = 0;
  std::vector<int> batch;
  const int batch_size = svs ? svs->GetBatchSize() : os->asr.GetBatchSize();
  int step = 0;
  while (FetchDynamic(res->segs, index_vector, head, batch_size, batch) > 0) {
    std::vector<float*> buff(batch.size());
    std::vector<const int16_t*> buff16(batch.size());
    std::vector<int> len(batch.size());
    for (size_t k = 0; k < batch.size(); ++k) {
      if (pcm16) buff16[k] = pcm16 + (same_rate ? res->segs[batch[k]].first : 0);
      else buff[k] = pcm.data() + res->segs[batch[k]].first;
      len[k] = same_rate || !pcm16 ? res->segs[batch[k]].second - res->segs[batch[k]].first : n_in;
    }
    const std::vector<std::string> msg_batch =
        svs ? (pcm16 ? svs->ForwardPcm16(buff16.data(), len.data(), true, svs_lang, svs_itn, search, (int)batch.size())
                     : svs->Forward(buff.data(), len.data(), true, svs_lang, svs_itn, search, (int)batch.size())) :
        pcm16 ? os->asr.ForwardPcm16(buff16.data(), len.data(), true, hw_emb, bias_dec, (int)batch.size(), same_rate ? 0 : sampling_rate)
              : os->asr.Forward(buff.data(), len.data(), true, hw_emb, bias_dec, (int)batch.size());
    for (size_t k = 0; k < batch.size(); ++k, ++msg_idx) {        // funasrruntime.cpp:270-279
      const int seg = index_vector[msg_idx];
      msgs[seg] = msg_batch[k];
      res->seg_ids[seg] = svs ? svs->LastTokenIds()[k] : os->asr.LastTokenIds()[k];
      if (svs) {                                                  // confidences stay with the adapter
        if (svs_stamps && k == 0) search ? svs->AlignSearchTokens() : svs->AlignGreedyTokens();      // once per batch, right behind its forward; refused: no stamps
        if (svs_stamps && k < svs->LastTokenStampsMs().size()) svs_ms[seg] = svs->LastTokenStampsMs()[k];
        continue;
      }
      if (k < os->asr.LastTimestamps().size()) spans[seg] = os->asr.LastTimestamps()[k];
      if (k < os->asr.LastTokenConfidence().size()) conf[seg] = os->asr.LastTokenConfidence()[k];
    }
    if (fn_callback) fn_callback(++step, (int)index_vector.size());
  }
  std::string cur_stamp = "[";
  for (size_t idx = 0; idx < msgs.size(); ++idx) {                                     // funasrruntime.cpp:291-312
    if (msgs[idx].empty()) continue;
    res->confidence.insert(res->confidence.end(), conf[idx].begin(), conf[idx].end());       // in the order the text is assembled
    const float t0 = (float)res->segs[idx].first / (float)model_rate;                  // msg_stimes
    const size_t bar = msgs[idx].find(" | ");
    res->msg += msgs[idx].substr(0, bar);
    if (svs) {                                      // [begin_ms, end_ms] per text token from the forced alignment, the segment's offset added
      const int t0_ms = (int)(1000 * t0);
      for (size_t i = 0; i + 1 < svs_ms[idx].size(); i += 2)
        cur_stamp += "[" + std::to_string((int)svs_ms[idx][i] + t0_ms) + "," + std::to_string((int)svs_ms[idx][i + 1] + t0_ms) + "],";
    } else if (bar != std::string::npos) {                 // "<text> | b0, e0,b1, e1": seconds relative to the segment
      std::vector<float> v;
      std::stringstream ss(msgs[idx].substr(bar + 3));
      std::string item;
      while (std::getline(ss, item, ',')) { try { v.push_back(std::stof(item)); } catch (...) { break; } }
      for (size_t i = 0; i + 1 < v.size(); i += 2)
        cur_stamp += "[" + std::to_string((int)(1000 * (v[i] + t0))) + "," + std::to_string((int)(1000 * (v[i + 1] + t0))) + "],";
    } else {                                        // no vocabulary loaded: ids as text, stamps straight from the adapter
      for (size_t i = 0; i + 2 < spans[idx].size() + 1 && i + 2 <= spans[idx].size(); i += 3) {
        if (spans[idx][i + 2] != 0.f) continue;
        cur_stamp += "[" + std::to_string((int)(1000 * (spans[idx][i] + t0))) + "," + std::to_string((int)(1000 * (spans[idx][i + 1] + t0))) + "],";
      }
    }
  }
  if (cur_stamp != "[") {
    cur_stamp.erase(cur_stamp.size() - 1);
    res->stamp = cur_stamp + "]";
  }
  if (os->punc) res->msg = os->punc->AddPunc(res->msg.c_str(), "zh-cn");               // funasrruntime.cpp:317-320 (re-entrant)
  return res.release();
}

const std::vector<std::vector<float>> CompileHotwordEmbedding(FUNASR_HANDLE handle, std::string& hotwords, ASR_TYPE mode) {
  (void)mode;
  OfflineStreamHip* os = static_cast<OfflineStreamHip*>(handle);
  if (!os) return {};
  return os->asr.CompileHotwordEmbedding(hotwords);
}

const char* FunASRGetResult(FUNASR_RESULT result, int n_index) {
  (void)n_index;
  return result ? static_cast<RecogResult*>(result)->msg.c_str() : nullptr;
}
const char* FunASRGetStamp(FUNASR_RESULT result) { return result ? static_cast<RecogResult*>(result)->stamp.c_str() : nullptr; }
float FunASRGetRetSnippetTime(FUNASR_RESULT result) { return result ? static_cast<RecogResult*>(result)->snippet_time : 0.f; }
void FunASRFreeResult(FUNASR_RESULT result) { delete static_cast<RecogResult*>(result); }
void FunOfflineUninit(FUNASR_HANDLE handle) { delete static_cast<OfflineStreamHip*>(handle); }
const std::vector<std::vector<int>>& FunASRGetSegmentIds(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->seg_ids; }
const std::vector<std::pair<int, int>>& FunASRGetSegments(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->segs; }
const std::vector<int>& FunASRGetOnlineIds(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->online_ids; }
void FunOfflineSetNbest(FUNASR_HANDLE handle, int k) { if (handle) static_cast<OfflineStreamHip*>(handle)->asr.SetNbest(k); }
void FunOfflineSetCtcStamps(FUNASR_HANDLE handle, int on) {
  OfflineStreamHip* os = static_cast<OfflineStreamHip*>(handle);
  if (os && os->svs) os->svs_ctc_stamps.store(on != 0);
}
int FunOfflineLoadTokenLm(FUNASR_HANDLE handle, const char* arpa_path, float scale, float token_bonus) {
  OfflineStreamHip* os = static_cast<OfflineStreamHip*>(handle);
  if (!os || !arpa_path) return 0;
  return (os->svs ? os->svs->InitTokenLm(arpa_path, scale, token_bonus) : os->asr.InitTokenLm(arpa_path, scale, token_bonus)) ? 1 : 0;
}
void FunOfflineSetCifStamps(FUNASR_HANDLE handle, int mode) { if (handle) static_cast<OfflineStreamHip*>(handle)->asr.SetCifTimestamps(mode); }
const std::vector<float>& FunASRGetTokenConfidence(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->confidence; }
const std::vector<float>& FunASRGetOnlineConfidence(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->online_conf; }
const std::vector<int>& FunASRGetOnlineFireMs(FUNASR_RESULT result) { return static_cast<RecogResult*>(result)->online_fire_ms; }
pfhip_model* FunOfflineGetAsrHandle(FUNASR_HANDLE handle) { return handle ? static_cast<OfflineStreamHip*>(handle)->asr.Handle() : nullptr; }


// ---- 2-pass --------------------------------------------------------------------------------------------------------------
namespace {

struct TpassStreamHip {               // funasr::TpassStream (tpass-stream.cpp): the shared models
  funasr::ParaformerHip asr;          // ONE object holds the offline session and the online encoder / decoder (paraformer.cpp:134-154)
  std::unique_ptr<funasr::SenseVoiceSmallHip> svs;      // MODEL_DIR names MODEL_SVS (tpass-stream.cpp:44-50): this one holds both, `asr` stays unloaded
  std::atomic<bool> svs_ctc_stamps{false};              // FunTpassSetCtcStamps
  int detail_k = 0;                   // FunTpassSetNbest: for the streams of later FunTpassOnlineInit calls
  std::unique_ptr<funasr::FsmnVadHip> vad;
  std::unique_ptr<funasr::PuncModelHipBase> punc_online;      // TpassStream::punc_online_handle (tpass-stream.cpp:100-135)
};

struct TpassOnlineStreamHip {         // funasr::TpassOnlineStream (tpass-online-stream.cpp:14-15): per connection
  TpassStreamHip* shared = nullptr;
  std::unique_ptr<funasr::ParaformerOnlineHip> asr_online;      // asr_online_handle (tpass-online-stream.cpp:14-15)
  std::unique_ptr<funasr::FsmnVadOnlineHip> vad_online;
  pfhip_host::TpassAudio audio;
};

}  // namespace

// TpassStream::TpassStream (tpass-stream.cpp:4-135) on the HIP plug-ins, call for call
FUNASR_HANDLE FunTpassInit(std::map<std::string, std::string>& model_path, int thread_num) {
  auto ts = std::make_unique<TpassStreamHip>();
  ts->vad = MakeVad(model_path, thread_num);
  if (!model_path.count(OFFLINE_MODEL_DIR) || !model_path.count(ONLINE_MODEL_DIR)) {                 // :79-82
    std::fprintf(stderr, "Can not find offline-model-dir or online-model-dir\n");
    std::exit(-1);
  }
  const std::string mdir = model_path[MODEL_DIR], odir = model_path[ONLINE_MODEL_DIR];
  const std::string hw_compile_model_path = PathAppend(mdir, MODEL_EB_NAME), seg_dict_path = PathAppend(mdir, MODEL_SEG_DICT);
  if (FileExists(hw_compile_model_path) && FileExists(seg_dict_path)) {                             // :54-60
    ts->asr.InitHwCompiler(hw_compile_model_path, thread_num);
    ts->asr.InitSegDict(seg_dict_path);
  }
  const bool q = IsTrue(model_path, QUANTIZE);                                                       // :62-72
  const std::string am_model_path = PathAppend(model_path[OFFLINE_MODEL_DIR], q ? QUANT_MODEL_NAME : MODEL_NAME);
  const std::string en_model_path = PathAppend(odir, q ? QUANT_ENCODER_NAME : ENCODER_NAME);
  const std::string de_model_path = PathAppend(odir, q ? QUANT_DECODER_NAME : DECODER_NAME);
  auto tokens_or_none = [](const std::string& p) { return FileExists(p) ? p : std::string(); };
  if (mdir.find(MODEL_SVS) != std::string::npos) {                                                   // :44-50: the directory's name picks the class
    ts->svs.reset(new funasr::SenseVoiceSmallHip());
    ts->svs->InitAsr(am_model_path, en_model_path, de_model_path, PathAppend(odir, AM_CMVN_NAME), PathAppend(mdir, AM_CONFIG_NAME),
                     tokens_or_none(PathAppend(mdir, TOKEN_PATH)), tokens_or_none(PathAppend(odir, TOKEN_PATH)), thread_num,
                     PathAppend(odir, AM_CONFIG_NAME));                                              // :76-77, exits on failure
    if (model_path.count(LM_DIR) && !model_path[LM_DIR].empty())                                     // :84-98: a call that returns
      ts->svs->InitLm(PathAppend(model_path[LM_DIR], LM_FST_RES), PathAppend(model_path[LM_DIR], LM_CONFIG_NAME),
                      PathAppend(model_path[LM_DIR], LEX_PATH), "");
  } else
  ts->asr.InitAsr(am_model_path, en_model_path, de_model_path, PathAppend(odir, AM_CMVN_NAME), PathAppend(mdir, AM_CONFIG_NAME),
                  tokens_or_none(PathAppend(mdir, TOKEN_PATH)), tokens_or_none(PathAppend(odir, TOKEN_PATH)), thread_num,
                  PathAppend(odir, AM_CONFIG_NAME));                                                 // :76-77, exits on failure
  if (!ts->vad) {                                                                                    // tpass-online-stream.cpp:8-11
    std::fprintf(stderr, "vad_handle is null\n");
    std::exit(-1);
  }
  if (model_path.count(PUNC_DIR) && !model_path[PUNC_DIR].empty())                                   // :100-135, realtime or offline class
    ts->punc_online.reset(funasr::CreatePuncModelHip(model_path[PUNC_DIR], thread_num, true, IsTrue(model_path, PUNC_QUANT)));
  // One handler thread per connection in the server: the VAD's concurrent device calls are merged into batched passes (the
  // online acoustic model's queue is set up by ParaformerHip::InitAsr).  Not keyed on `thread_num`: that is --model-thread-num
  // (onnxruntime intra-op threads, default 1: funasr-wss-server-2pass.cpp:110,569), not the number of handler threads.
  {
    auto knob = [](const char* name, int dflt) { const char* e = std::getenv(name); return e && *e ? std::atoi(e) : dflt; };
    pfhip_set_vad_stream_batching(ts->vad->Handle(), knob("PFHIP_VAD_WAIT_US", 1000), knob("PFHIP_VAD_MAX", 256));
  }
  return ts.release();
}

// TpassOnlineStream::TpassOnlineStream (tpass-online-stream.cpp:4-19)
FUNASR_HANDLE FunTpassOnlineInit(FUNASR_HANDLE tpass_handle, std::vector<int> chunk_size) {
  TpassStreamHip* ts = static_cast<TpassStreamHip*>(tpass_handle);
  if (!ts || chunk_size.size() != 3) return nullptr;
  auto os = std::make_unique<TpassOnlineStreamHip>();
  os->shared = ts;
  os->vad_online.reset(new funasr::FsmnVadOnlineHip(ts->vad.get()));
  if (ts->svs) os->asr_online.reset(new funasr::ParaformerOnlineHip(ts->svs.get(), chunk_size, MODEL_SVS));      // tpass-online-stream.cpp:14-15
  else os->asr_online.reset(new funasr::ParaformerOnlineHip(&ts->asr, chunk_size));
  if (!os->asr_online->ok() || !os->vad_online->ok()) {
    std::fprintf(stderr, "FunTpassOnlineInit: %s\n", pfhip_last_error());
    return nullptr;
  }
  if (ts->detail_k > 0) os->asr_online->SetDetail(ts->detail_k, true);      // FunTpassSetNbest
  return os.release();
}

int FunTpassLoadTokenLm(FUNASR_HANDLE tpass_handle, const char* arpa_path, float scale, float token_bonus) {
  TpassStreamHip* ts = static_cast<TpassStreamHip*>(tpass_handle);
  if (!ts || !arpa_path) return 0;
  return (ts->svs ? ts->svs->InitTokenLm(arpa_path, scale, token_bonus) : ts->asr.InitTokenLm(arpa_path, scale, token_bonus)) ? 1 : 0;
}

void FunTpassSetNbest(FUNASR_HANDLE tpass_handle, int k) {
  TpassStreamHip* ts = static_cast<TpassStreamHip*>(tpass_handle);
  if (!ts) return;
  ts->asr.SetNbest(k);
  ts->detail_k = ts->asr.GetNbest();
}

void FunTpassSetCifStamps(FUNASR_HANDLE tpass_handle, int mode) {
  if (tpass_handle) static_cast<TpassStreamHip*>(tpass_handle)->asr.SetCifTimestamps(mode);
}

void FunTpassSetCtcStamps(FUNASR_HANDLE tpass_handle, int on) {
  TpassStreamHip* ts = static_cast<TpassStreamHip*>(tpass_handle);
  if (ts && ts->svs) ts->svs_ctc_stamps.store(on != 0);
}

// FunASRWfstDecoderInit's no-LM branch (funasrruntime.cpp:836-894): a CtcPrefixDecoder on the model's vocabulary
FUNASR_DEC_HANDLE FunASRCtcDecoderInit(FUNASR_HANDLE handle, float glob_beam, float lat_beam, ASR_TYPE asr_type) {
  if (!handle) return nullptr;
  funasr::SenseVoiceSmallHip* svs = asr_type == ASR_OFFLINE ? static_cast<OfflineStreamHip*>(handle)->svs.get()
                                                            : static_cast<TpassStreamHip*>(handle)->svs.get();
  // A Paraformer stream gets one on its own vocabulary: it has no CTC rows, but with hotwords loaded ParaformerHip runs the biased
  // search over its head's candidates (an extension; the reference creates the decoder and then never looks at it, paraformer.cpp:563-579)
  funasr::HipVocab* vocab = svs ? svs->GetHipVocab()
                                : (asr_type == ASR_OFFLINE ? static_cast<OfflineStreamHip*>(handle)->asr : static_cast<TpassStreamHip*>(handle)->asr).GetHipVocab();
  return static_cast<funasr::Decoder*>(new funasr::CtcPrefixDecoderHip(vocab, glob_beam, lat_beam));
}
static funasr::CtcPrefixDecoderHip* SearchOf(FUNASR_DEC_HANDLE dec) {
  return dynamic_cast<funasr::CtcPrefixDecoderHip*>(static_cast<funasr::Decoder*>(dec));
}
int FunCtcDecoderLoadHwsRes(FUNASR_DEC_HANDLE dec, int inc_bias, std::unordered_map<std::string, int>& hws_map) {
  funasr::CtcPrefixDecoderHip* d = dec ? SearchOf(dec) : nullptr;
  return d ? d->LoadHwsRes(inc_bias, hws_map) : 0;
}
void FunCtcDecoderUnloadHwsRes(FUNASR_DEC_HANDLE dec) {
  if (funasr::CtcPrefixDecoderHip* d = dec ? SearchOf(dec) : nullptr) d->UnloadHwsRes();
}
void FunCtcDecoderUninit(FUNASR_DEC_HANDLE dec) { delete static_cast<funasr::Decoder*>(dec); }

FUNASR_RESULT FunTpassInferBuffer(FUNASR_HANDLE handle, FUNASR_HANDLE online_handle, const char* sz_buf, int n_len,
                                  std::vector<std::vector<std::string>>& punc_cache, bool input_finished, int sampling_rate,
                                  std::string wav_format, ASR_TYPE mode, const std::vector<std::vector<float>>& hw_emb, bool itn,
                                  int vad_tail_sil, int vad_max_len, FUNASR_DEC_HANDLE dec_handle, std::string svs_lang, bool svs_itn) {
  (void)itn;
  TpassStreamHip* ts = static_cast<TpassStreamHip*>(handle);
  TpassOnlineStreamHip* os = static_cast<TpassOnlineStreamHip*>(online_handle);
  if (!ts || !os || !sz_buf) return nullptr;
  if (wav_format != "pcm" && wav_format != "PCM") return nullptr;                  // funasrruntime.cpp:523-531
  if (ts->punc_online && punc_cache.size() < 2) return nullptr;                    // [0]: online text, [1]: 2nd-pass text
  if (sampling_rate == 16000) {
    if (!os->audio.LoadPcmwavOnline(sz_buf, n_len)) return nullptr;
  } else {                  // LoadPcmwavOnline with WavResample of THIS buffer alone (audio.cpp:821-857): no state across calls
    std::vector<float> pcm;
    if (!LoadPcm(ts->svs ? ts->svs->Handle() : ts->asr.Handle(), sz_buf, n_len, sampling_rate, pcm)) {
      std::fprintf(stderr, "FunTpassInferBuffer: %s\n", pfhip_last_error());
      return nullptr;
    }
    os->audio.LoadSamplesOnline(pcm.data(), (int)pcm.size());
  }
  auto res = std::make_unique<RecogResult>();
  res->snippet_time = os->audio.GetTimeLen();
  // FsmnVadOnline::Infer (fsmn-vad-online.cpp:135-151) as the VAD of Audio::Split
  os->vad_online->SetConfig(vad_tail_sil, vad_max_len);
  // at 16 kHz the message's own 16-bit samples go to the VAD network (Split hands the callable exactly this message's samples as
  // floats; the detector gets its float waveform back from the device call), to the streaming model and to the offline model
  std::vector<int16_t> store16;
  const int16_t* msg16 = sampling_rate == 16000 ? Pcm16View(sz_buf, n_len / 2, store16) : nullptr;
  auto vad_infer = [&](std::vector<float>& waves, bool fin) {
    if (msg16 && (int)waves.size() == n_len / 2) return os->vad_online->InferPcm16(msg16, n_len / 2, fin);
    return os->vad_online->Infer(waves, fin);
  };
  os->audio.Split(vad_infer, os->asr_online->chunk_len, input_finished, (pfhip_host::AsrType)mode);
  pfhip_host::TpassFrame frame;
  while (os->audio.FetchChunck(frame)) {                                            // funasrruntime.cpp:538-566
    const std::string msg = frame.pcm16.size() == frame.data.size() && !frame.data.empty()
                                ? os->asr_online->ForwardPcm16(frame.pcm16.data(), (int)frame.pcm16.size(), frame.is_final)
                                : os->asr_online->Forward(frame.data.data(), (int)frame.data.size(), frame.is_final);      // :540
    res->online_ids.insert(res->online_ids.end(), os->asr_online->LastTokenIds().begin(), os->asr_online->LastTokenIds().end());
    res->online_conf.insert(res->online_conf.end(), os->asr_online->LastTokenConfidence().begin(), os->asr_online->LastTokenConfidence().end());
    for (int f : os->asr_online->LastFireFrames()) res->online_fire_ms.push_back(funasr::ParaformerOnlineHip::FireFrameMs(f));
    if (mode == ASR_ONLINE) {
      os->asr_online->online_res += msg;
      if (frame.is_final) {                                                         // funasrruntime.cpp:543-556
        res->tpass_msg = os->asr_online->online_res;
        if (ts->punc_online) res->tpass_msg = ts->punc_online->AddPunc(os->asr_online->online_res.c_str(), punc_cache[0]);
        os->asr_online->online_res.clear();
      }
      res->msg += msg;
    } else if (mode == ASR_TWO_PASS) {
      res->msg += msg;
    }
  }
  std::string cur_stamp = "[";
  while (os->audio.FetchTpass(frame)) {                                             // funasrruntime.cpp:570-639
    float* buff[1] = {frame.data.data()};
    int len[1] = {(int)frame.data.size()};
    const int16_t* buff16[1] = {frame.pcm16.data()};
    if (ts->svs) {                               // funasrruntime.cpp:583-587, :609-631: the model type routes the second pass
      funasr::SenseVoiceSmallHip* svs = ts->svs.get();
      // a CtcPrefixDecoderHip selects the device search for the second pass; any other decoder handle is not passed on, as before
      funasr::CtcPrefixDecoderHip* search = dynamic_cast<funasr::CtcPrefixDecoderHip*>(static_cast<funasr::Decoder*>(dec_handle));
      const std::vector<std::string> texts = frame.pcm16.size() == frame.data.size() && !frame.data.empty()
                                                 ? svs->ForwardPcm16(buff16, len, true, svs_lang, svs_itn, search, 1)
                                                 : svs->Forward(buff, len, true, svs_lang, svs_itn, search, 1);
      const std::string text = texts.empty() ? "" : texts[0];
      if (text.empty()) continue;
      res->seg_ids.push_back(svs->LastTokenIds()[0]);
      res->segs.emplace_back(frame.global_start, frame.global_end);      // ms on the connection's time axis
      // FunTpassSetCtcStamps: the greedy tokens' spans (60-ms rows) plus the segment's start; a refused alignment leaves no pairs
      if (ts->svs_ctc_stamps.load() && (search ? svs->AlignSearchTokens() : svs->AlignGreedyTokens()) && !svs->LastTokenStampsMs().empty()) {
        const std::vector<float>& ms = svs->LastTokenStampsMs()[0];
        for (size_t i = 0; i + 1 < ms.size(); i += 2)
          cur_stamp += "[" + std::to_string((int)ms[i] + frame.global_start) + "," + std::to_string((int)ms[i + 1] + frame.global_start) + "],";
        if (cur_stamp != "[") {
          cur_stamp.erase(cur_stamp.size() - 1);
          res->stamp += cur_stamp + "]";
          cur_stamp = "[";
        }
      }
      res->tpass_msg = text;                     // no punctuation and no ITN for this model (:609-631)
      continue;
    }
    // a CtcPrefixDecoderHip goes through to the second pass (hotwords for any Paraformer); any other decoder handle does not, as before
    funasr::Decoder* const bias_dec = dynamic_cast<funasr::CtcPrefixDecoderHip*>(static_cast<funasr::Decoder*>(dec_handle));
    const std::vector<std::string> msgs = frame.pcm16.size() == frame.data.size() && !frame.data.empty()
                                              ? ts->asr.ForwardPcm16(buff16, len, true, hw_emb, bias_dec, 1)
                                              : ts->asr.Forward(buff, len, true, hw_emb, bias_dec, 1);
    std::string msg = msgs.empty() ? "" : msgs[0];
    if (msg.empty()) continue;
    if (bias_dec) res->seg_ids.push_back(ts->asr.LastTokenIds()[0]);            // what FunASRGetSegmentIds returns for such a call
    if (!ts->asr.LastTokenConfidence().empty())                                     // FunTpassSetNbest: as FunOfflineInferBuffer
      res->confidence.insert(res->confidence.end(), ts->asr.LastTokenConfidence()[0].begin(), ts->asr.LastTokenConfidence()[0].end());
    const size_t bar = msg.find(" | ");
    if (bar != std::string::npos) {
      std::vector<float> v;
      std::stringstream ss(msg.substr(bar + 3));
      std::string item;
      while (std::getline(ss, item, ',')) { try { v.push_back(std::stof(item)); } catch (...) { break; } }
      for (size_t i = 0; i + 1 < v.size(); i += 2) {
        const float b = v[i] + (float)frame.global_start / 1000.0f, e = v[i + 1] + (float)frame.global_start / 1000.0f;
        cur_stamp += "[" + std::to_string((int)(1000 * b)) + "," + std::to_string((int)(1000 * e)) + "],";
      }
      msg = msg.substr(0, bar);
    }
    if (cur_stamp != "[") {
      cur_stamp.erase(cur_stamp.size() - 1);
      res->stamp += cur_stamp + "]";
    }
    res->tpass_msg = msg;
    if (ts->punc_online) {                                                          // funasrruntime.cpp:609-614 (re-entrant)
      res->tpass_msg = ts->punc_online->AddPunc(msg.c_str(), punc_cache[1]);
      if (input_finished && ts->punc_online->is_online) res->tpass_msg += "\xE3\x80\x82";      // "。"
    }
  }
  if (input_finished) os->audio.ResetIndex();
  return res.release();
}

const char* FunASRGetTpassResult(FUNASR_RESULT result, int n_index) {
  (void)n_index;
  return result ? static_cast<RecogResult*>(result)->tpass_msg.c_str() : nullptr;
}
void FunTpassOnlineUninit(FUNASR_HANDLE online_handle) { delete static_cast<TpassOnlineStreamHip*>(online_handle); }
void FunTpassUninit(FUNASR_HANDLE handle) { delete static_cast<TpassStreamHip*>(handle); }
