// Harness over the 2-pass handle API (funasrruntime_hip.h), one connection fed like the websocket server feeds it
// (websocket/bin/websocket-server-2pass.cpp:135-148: 9600-sample pieces, the last one with input_finished):
//   tpass_infer <offline_model_dir> <online_model_dir> <vad_dir> <pcm_s16_file> [step_samples=9600] [mode=2] [punc_dir|-] [audio_fs=16000] [nbest=0] [cif_stamps=0]
//   (step_samples counts samples at audio_fs, as the reference server forwards each message with its audio_fs)
// One line per call: "call <j> | online <text> | tpass <text> | stamp <stamp>".
// nbest = 1..8 (FunTpassSetNbest, an extension) appends two fields to every line: " | online_detail <confidence>@<fire ms> ..." with one
// entry per streamed token id of the call, and " | tpass_conf <confidence> ..." for the tokens of the second-pass text.
// cif_stamps = 1 | 2 (FunTpassSetCifStamps, an extension): the stamp field of the second pass comes from the CIF scan's fire frames.
// An offline_model_dir whose name contains "SenseVoiceSmall" makes the second pass a SenseVoiceSmallHip (tpass-stream.cpp:44-50); three
// more arguments then apply: [svs_lang=auto] [svs_itn=1] [ctc_stamps=0] (FunTpassInferBuffer's trailing arguments, FunTpassSetCtcStamps),
// and every line gets a field " | tpass_ids <second-pass ids of the segments closed in the call>".
// Three or more further arguments, [glob_beam lat_beam [hotword score]...] behind those (use "auto 1 0" for the three before them): the
// connection gets a decoder handle (FunASRCtcDecoderInit, FunCtcDecoderLoadHwsRes) that every FunTpassInferBuffer call passes on, and
// every line gets the " | tpass_ids" field.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "funasrruntime_hip.h"

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s offline_dir online_dir vad_dir pcm_s16_file [step] [mode] [punc_dir|-] [audio_fs] [nbest] [cif_stamps]\n", argv[0]);
    return 2;
  }
  std::map<std::string, std::string> paths;
  paths[MODEL_DIR] = argv[1]; paths[ONLINE_MODEL_DIR] = argv[2]; paths[VAD_DIR] = argv[3];
  if (argc > 7 && std::string(argv[7]) != "-") paths[PUNC_DIR] = argv[7];
  const int audio_fs = argc > 8 ? std::atoi(argv[8]) : 16000;
  const int step = argc > 5 ? std::atoi(argv[5]) : 9600;
  const ASR_TYPE mode = argc > 6 ? (ASR_TYPE)std::atoi(argv[6]) : ASR_TWO_PASS;
  std::ifstream f(argv[4], std::ios::binary);
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  FUNASR_HANDLE h = FunTpassInit(paths, 1);
  const int nbest = argc > 9 ? std::atoi(argv[9]) : 0;
  if (h && nbest > 0) FunTpassSetNbest(h, nbest);                  // before the connection's stream is made
  if (h && argc > 10) FunTpassSetCifStamps(h, std::atoi(argv[10]));      // the offline pass stamps from the CIF scan (an extension)
  const bool svs = std::string(argv[1]).find(MODEL_SVS) != std::string::npos;
  const std::string svs_lang = argc > 11 ? argv[11] : "auto";
  const bool svs_itn = argc > 12 ? std::atoi(argv[12]) != 0 : true;
  if (h && svs && argc > 13) FunTpassSetCtcStamps(h, std::atoi(argv[13]));
  FUNASR_HANDLE oh = FunTpassOnlineInit(h, {5, 10, 5});
  if (!h || !oh) return 1;
  FUNASR_DEC_HANDLE dec = nullptr;
  if (argc > 15) {
    dec = FunASRCtcDecoderInit(h, (float)std::atof(argv[14]), (float)std::atof(argv[15]), ASR_TWO_PASS);
    std::unordered_map<std::string, int> hws;
    for (int a = 16; a + 1 < argc; a += 2) hws[argv[a]] = std::atoi(argv[a + 1]);
    std::printf("dec_handle %d hw_loaded %d\n", dec ? 1 : 0, FunCtcDecoderLoadHwsRes(dec, 0, hws));
  }
  std::vector<std::vector<std::string>> punc_cache(2);
  const int n_bytes = (int)buf.size(), step_bytes = step * 2;
  int j = 0;
  for (int off = 0; off < n_bytes; off += step_bytes, ++j) {
    const int nb = std::min(step_bytes, n_bytes - off);
    const bool last = off + step_bytes >= n_bytes;
    FUNASR_RESULT r = FunTpassInferBuffer(h, oh, buf.data() + off, nb, punc_cache, last, audio_fs, "pcm", mode, {{0.0f}}, true, 800, 60000,
                                          dec, svs_lang, svs_itn);
    if (!r) { std::fprintf(stderr, "inference failed\n"); return 1; }
    std::printf("call %d | online %s | tpass %s | stamp %s", j, FunASRGetResult(r, 0), FunASRGetTpassResult(r, 0), FunASRGetStamp(r));
    if (nbest > 0) {
      const std::vector<float>& conf = FunASRGetOnlineConfidence(r);
      const std::vector<int>& ms = FunASRGetOnlineFireMs(r);
      std::printf(" | online_detail");
      for (size_t t = 0; t < conf.size() && t < ms.size(); ++t) std::printf(" %.9g@%d", conf[t], ms[t]);
      std::printf(" | tpass_conf");
      for (float c : FunASRGetTokenConfidence(r)) std::printf(" %.9g", c);
    }
    if (svs || dec) {
      std::printf(" | tpass_ids");
      for (const std::vector<int>& seg : FunASRGetSegmentIds(r)) for (int id : seg) std::printf(" %d", id);
    }
    std::printf("\n");
    FunASRFreeResult(r);
  }
  if (dec) FunCtcDecoderUninit(dec);
  FunTpassOnlineUninit(oh);
  FunTpassUninit(h);
  return 0;
}
