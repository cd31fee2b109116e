// Harness over SenseVoiceSmallHip (sensevoice_hip.h), the shape of a decoder thread's call:
//   svs_infer <am_model> <tokens.json|-> <svs_lang> <svs_itn 0|1> <pcm_s16_file>...
//   svs_infer --decoder <am_model> <pcm_s16_file>...      the same packed call with a stub Decoder as decoder_handle (the shape of
//                          decoder_handoff.cpp for Paraformer): prints what every Search call received — "search <i> rows <n> vocab <V> :
//                          <arg-max of each row>" — the Start / End / Finalize calls it saw, and the strings Forward returned
//   svs_infer --handle-api <model_dir> <svs_lang> <svs_itn 0|1> <pcm_s16_file>      FunOfflineInit -> FunOfflineInferBuffer on the
//                          directory (its name decides the model type); prints "seg <start> <end> : <ids>" and "text [<text>]"
//   svs_infer --ctc-stamps ...       any of the three with token time spans by CTC forced alignment switched on (SetCtcTimestamps /
//                          FunOfflineSetCtcStamps): the default form adds "utt <i> spans : <begin end>..." (rows) and "utt <i> stamps :
//                          <begin_ms end_ms>..." per utterance, --decoder adds "utt <i> stamps <count>" (0: a search returns no ids),
//                          --handle-api adds "handle stamp [<FunASRGetStamp>]"; --ctc-stamps --with-decoder --handle-api ... also
//                          passes a decoder handle to FunOfflineInferBuffer (the stamp stays empty).  Without the flag nothing differs.
//   svs_infer --beam <am_model> <tokens.json|-> <svs_lang> <svs_itn 0|1> <glob_beam> <lat_beam> [--hotword <text> <score>]... <pcm_s16_file>...
//                          the packed call with a CtcPrefixDecoderHip as decoder_handle (the device search): "hotwords loaded <n>",
//                          per utterance "utt <i> search ids : ..." and "utt <i> text [<text>]" (with --ctc-stamps also "utt <i>
//                          stamps : ..."), then the same after UnloadHwsRes as "unloaded utt <i> search ids : ..."
//   svs_infer --beam-handle-api <model_dir> <svs_lang> <svs_itn 0|1> <glob_beam> <lat_beam> [--hotword <text> <score>]... <pcm_s16_file>
//                          FunOfflineInit -> FunASRCtcDecoderInit -> FunCtcDecoderLoadHwsRes -> FunOfflineInferBuffer with that handle
//                          -> FunCtcDecoderUninit; prints "hotwords loaded <n>", "handle text [<text>]", with --ctc-stamps "handle stamp [..]"
// One packed ForwardPcm16 over all files, then Forward on the floats of the first file alone.  Prints per utterance
// "utt <i> ids : ..." / "utt <i> frames : ..." / "utt <i> text [<text>]", then "alone ids : ..." for the float call.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "ctc_prefix_decoder_hip.h"
#include "funasrruntime_hip.h"
#include "sensevoice_hip.h"

namespace {
bool g_ctc_stamps = false, g_with_decoder = false;
std::string dir_file(const std::string& model, const char* name) {      // <dir of am_model>/<name>, as the factory builds its paths
  const size_t slash = model.rfind('/');
  return (slash == std::string::npos ? std::string() : model.substr(0, slash + 1)) + name;
}
std::vector<std::vector<int16_t>> read_pcm(int argc, char** argv, int first) {
  std::vector<std::vector<int16_t>> pcm;
  for (int i = first; i < argc; ++i) {
    std::ifstream f(argv[i], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    pcm.emplace_back(reinterpret_cast<const int16_t*>(raw.data()), reinterpret_cast<const int16_t*>(raw.data()) + raw.size() / 2);
  }
  return pcm;
}
// what a caller's search would be handed: records every call
struct StubDecoder : funasr::Decoder {
  int starts = 0, ends = 0, finals = 0, searches = 0;
  void StartUtterance() override { ++starts; }
  void EndUtterance() override { ++ends; }
  std::string Search(float* in, int len, int64_t token_nums) override {
    std::printf("search %d rows %d vocab %lld :", searches, len, (long long)token_nums);
    for (int t = 0; t < len; ++t) {
      const float* row = in + (size_t)t * token_nums;
      int best = 0;
      for (int64_t v = 1; v < token_nums; ++v) if (row[v] > row[best]) best = (int)v;
      std::printf(" %d", best);
    }
    std::printf("\n");
    return "partial" + std::to_string(searches++);
  }
  std::string FinalizeDecode(bool, std::vector<float>, std::vector<float>) override { return "final" + std::to_string(finals++); }
};
}  // namespace

static int decoder_mode(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::vector<std::vector<int16_t>> pcm = read_pcm(argc, argv, 3);
  funasr::SenseVoiceSmallHip model;
  model.InitAsr(argv[2], dir_file(argv[2], "am.mvn"), dir_file(argv[2], "config.yaml"), "", 1);
  std::vector<const int16_t*> ptr;
  std::vector<int> len;
  for (const auto& p : pcm) { ptr.push_back(p.data()); len.push_back((int)p.size()); }
  StubDecoder dec;
  model.SetCtcTimestamps(g_ctc_stamps);
  for (int finished = 0; finished < 2; ++finished) {
    const std::vector<std::string> text = model.ForwardPcm16(ptr.data(), len.data(), finished != 0, "auto", false, &dec, (int)pcm.size());
    for (size_t i = 0; i < text.size(); ++i) std::printf("finished %d utt %zu text [%s]\n", finished, i, text[i].c_str());
    if (g_ctc_stamps)
      for (size_t i = 0; i < text.size(); ++i)
        std::printf("utt %zu stamps %zu\n", i, i < model.LastTokenStampsMs().size() ? model.LastTokenStampsMs()[i].size() : (size_t)0);
  }
  std::printf("calls starts %d ends %d finals %d searches %d\n", dec.starts, dec.ends, dec.finals, dec.searches);
  return 0;
}

// the --hotword <text> <score> pairs from argv[at] on; returns the index behind them
static int read_hotwords(int argc, char** argv, int at, std::unordered_map<std::string, int>& hws) {
  while (at + 2 < argc && std::string(argv[at]) == "--hotword") { hws[argv[at + 1]] = std::atoi(argv[at + 2]); at += 3; }
  return at;
}

static int beam_mode(int argc, char** argv) {
  if (argc < 9) return 2;
  const std::string tokens = std::string(argv[3]) == "-" ? "" : argv[3], lang = argv[4];
  const bool itn = std::atoi(argv[5]) != 0;
  std::unordered_map<std::string, int> hws;
  const int first = read_hotwords(argc, argv, 8, hws);
  const std::vector<std::vector<int16_t>> pcm = read_pcm(argc, argv, first);
  funasr::SenseVoiceSmallHip model;
  model.InitAsr(argv[2], dir_file(argv[2], "am.mvn"), dir_file(argv[2], "config.yaml"), tokens, 1);
  model.SetCtcTimestamps(g_ctc_stamps);
  funasr::CtcPrefixDecoderHip dec(model.GetHipVocab(), (float)std::atof(argv[6]), (float)std::atof(argv[7]));
  std::printf("hotwords loaded %d\n", dec.LoadHwsRes(3, hws));
  std::vector<const int16_t*> ptr;
  std::vector<int> len;
  for (const auto& p : pcm) { ptr.push_back(p.data()); len.push_back((int)p.size()); }
  for (int pass = 0; pass < 2; ++pass) {
    const char* tag = pass ? "unloaded " : "";
    const std::vector<std::string> text = model.ForwardPcm16(ptr.data(), len.data(), true, lang, itn, &dec, (int)pcm.size());
    for (size_t i = 0; i < text.size(); ++i) {
      std::printf("%sutt %zu search ids :", tag, i);
      for (int id : model.LastSearchIds()[i]) std::printf(" %d", id);
      std::printf("\n%sutt %zu greedy ids :", tag, i);
      for (int id : model.LastTokenIds()[i]) std::printf(" %d", id);
      std::printf("\n%sutt %zu text [%s]\n", tag, i, text[i].c_str());
      if (g_ctc_stamps) {
        std::printf("%sutt %zu stamps :", tag, i);
        if (i < model.LastTokenStampsMs().size()) for (float ms : model.LastTokenStampsMs()[i]) std::printf(" %d", (int)ms);
        std::printf("\n");
      }
    }
    dec.UnloadHwsRes();
  }
  return 0;
}

static int beam_handle_api(int argc, char** argv) {
  if (argc < 8) return 2;
  std::map<std::string, std::string> paths;
  paths[MODEL_DIR] = argv[2];
  std::unordered_map<std::string, int> hws;
  const int first = read_hotwords(argc, argv, 7, hws);
  if (first >= argc) return 2;
  std::ifstream f(argv[first], std::ios::binary);
  const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  FUNASR_HANDLE h = FunOfflineInit(paths, 1, false, 1);
  if (g_ctc_stamps) FunOfflineSetCtcStamps(h, 1);
  FUNASR_DEC_HANDLE dec = FunASRCtcDecoderInit(h, (float)std::atof(argv[5]), (float)std::atof(argv[6]));
  if (!dec) { std::fprintf(stderr, "no decoder for this handle\n"); return 1; }
  std::printf("hotwords loaded %d\n", FunCtcDecoderLoadHwsRes(dec, 3, hws));
  const std::vector<std::vector<float>> no_hw;
  FUNASR_RESULT r = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, 16000, "pcm", true, 800, 60000, dec, argv[3],
                                          std::atoi(argv[4]) != 0);
  if (!r) { std::fprintf(stderr, "inference failed\n"); return 1; }
  std::printf("handle text [%s]\n", FunASRGetResult(r, 0));
  if (g_ctc_stamps) std::printf("handle stamp [%s]\n", FunASRGetStamp(r));
  FunASRFreeResult(r);
  FunCtcDecoderUnloadHwsRes(dec);
  FunCtcDecoderUninit(dec);
  FunOfflineUninit(h);
  return 0;
}

static int handle_api(int argc, char** argv) {
  if (argc < 6) return 2;
  std::map<std::string, std::string> paths;
  paths[MODEL_DIR] = argv[2];
  std::ifstream f(argv[5], std::ios::binary);
  const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  FUNASR_HANDLE h = FunOfflineInit(paths, 1, false, 1);
  if (g_ctc_stamps) FunOfflineSetCtcStamps(h, 1);
  const std::vector<std::vector<float>> no_hw;
  StubDecoder dec;
  FUNASR_RESULT r = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, 16000, "pcm", true, 800, 60000,
                                          g_with_decoder ? static_cast<FUNASR_DEC_HANDLE>(&dec) : nullptr, argv[3], std::atoi(argv[4]) != 0);
  if (!r) { std::fprintf(stderr, "inference failed\n"); return 1; }
  const auto& segs = FunASRGetSegments(r);
  const auto& ids = FunASRGetSegmentIds(r);
  for (size_t i = 0; i < segs.size(); ++i) {
    std::printf("seg %d %d :", segs[i].first, segs[i].second);
    for (int id : ids[i]) std::printf(" %d", id);
    std::printf("\n");
  }
  std::printf("handle text [%s]\n", FunASRGetResult(r, 0));
  if (g_ctc_stamps) std::printf("handle stamp [%s]\n", FunASRGetStamp(r));
  FunASRFreeResult(r);
  FunOfflineUninit(h);
  return 0;
}

int main(int argc, char** argv) {
  while (argc > 1 && (std::string(argv[1]) == "--ctc-stamps" || std::string(argv[1]) == "--with-decoder")) {      // leading switches
    (std::string(argv[1]) == "--ctc-stamps" ? g_ctc_stamps : g_with_decoder) = true;
    for (int i = 1; i + 1 < argc; ++i) argv[i] = argv[i + 1];
    --argc;
  }
  if (argc > 1 && std::string(argv[1]) == "--beam") return beam_mode(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "--beam-handle-api") return beam_handle_api(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "--handle-api") return handle_api(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "--decoder") return decoder_mode(argc, argv);
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s am_model tokens.json|- svs_lang svs_itn pcm_s16_file...\n", argv[0]);
    return 2;
  }
  const std::string tokens = std::string(argv[2]) == "-" ? "" : argv[2], lang = argv[3];
  const bool itn = std::atoi(argv[4]) != 0;
  const std::vector<std::vector<int16_t>> pcm = read_pcm(argc, argv, 5);
  funasr::SenseVoiceSmallHip model;
  model.SetBatchSize((int)pcm.size());
  model.InitAsr(argv[1], dir_file(argv[1], "am.mvn"), dir_file(argv[1], "config.yaml"), tokens, 1);
  model.SetCtcTimestamps(g_ctc_stamps);
  std::vector<const int16_t*> ptr;
  std::vector<int> len;
  for (const auto& p : pcm) { ptr.push_back(p.data()); len.push_back((int)p.size()); }
  const std::vector<std::string> text = model.ForwardPcm16(ptr.data(), len.data(), true, lang, itn, nullptr, (int)pcm.size());
  for (size_t i = 0; i < text.size(); ++i) {
    std::printf("utt %zu ids :", i);
    for (int id : model.LastTokenIds()[i]) std::printf(" %d", id);
    std::printf("\nutt %zu frames :", i);
    for (int fr : model.LastTokenFrames()[i]) std::printf(" %d", fr);
    std::printf("\nutt %zu confidence_ok %d\nutt %zu text [%s]\n", i, (int)(model.LastTokenConfidence()[i].size() == model.LastTokenIds()[i].size()), i,
                text[i].c_str());
    if (g_ctc_stamps) {
      std::printf("utt %zu spans :", i);
      if (i < model.LastTokenSpans().size()) for (int r : model.LastTokenSpans()[i]) std::printf(" %d", r);
      std::printf("\nutt %zu stamps :", i);
      if (i < model.LastTokenStampsMs().size()) for (float ms : model.LastTokenStampsMs()[i]) std::printf(" %d", (int)ms);
      std::printf("\n");
    }
  }
  std::vector<float> f32(pcm[0].size());
  for (size_t i = 0; i < f32.size(); ++i) f32[i] = (float)pcm[0][i] / 32768.f;
  float* one = f32.data();
  int n = (int)f32.size();
  const std::vector<std::string> alone = model.Forward(&one, &n, true, lang, itn, nullptr, 1);
  std::printf("alone ids :");
  for (int id : model.LastTokenIds()[0]) std::printf(" %d", id);
  std::printf("\nalone text [%s]\n", alone[0].c_str());
  return 0;
}
