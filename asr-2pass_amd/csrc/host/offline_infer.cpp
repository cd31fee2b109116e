// Harness over the handle-API mirror (funasrruntime_hip.h) with the shape of the reference's offline client
// (onnxruntime/bin/funasr-onnx-offline.cpp: FunOfflineInit -> FunOfflineInferBuffer per file -> FunASRGetResult):
//   offline_infer <model_dir> <vad_dir|-> <pcm_s16_file> [batch=32] [threads=1] [repeat=1] [punc_dir|-] [audio_fs] [nbest=0] [cif_stamps=0]
//                 [glob_beam lat_beam [hotword score]...]
// With the two beams: one more pass through a decoder handle (FunASRCtcDecoderInit -> FunOfflineInferBuffer(dec_handle)) before any
// hotword is loaded ("dec_seg ...", "dec_text", "dec_stamp"), then with the hotwords (FunCtcDecoderLoadHwsRes: "hw_loaded <n>",
// "hw_seg ...", "hw_text", "hw_stamp", "hw_confidence ..."); nbest and cif_stamps, where given, stay on for both.
// PFHIP_TOKEN_LM=<arpa file> (with PFHIP_TOKEN_LM_SCALE / PFHIP_TOKEN_LM_BONUS, defaults 1 / 0) in the environment: the file is
// loaded with FunOfflineLoadTokenLm behind the passes without a decoder handle ("lm_loaded <0|1>"), so the "dec" pass — a decoder
// handle, no hotwords — is the search with the model and the "hw" pass the search with both.
// Prints one line per VAD segment, time order: "seg <start_sample> <end_sample> : <ids...>", then timing; with threads > 1
// every thread transcribes the same buffer through the shared handle (the server's decoder threads).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <thread>
#include <unordered_map>
#include <vector>

#include "funasrruntime_hip.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s model_dir vad_dir|- pcm_s16_file [batch] [threads] [repeat] [punc_dir|-] [audio_fs] [nbest] [cif_stamps]\n", argv[0]);
    return 2;
  }
  std::map<std::string, std::string> paths;
  paths[MODEL_DIR] = argv[1];
  if (std::string(argv[2]) != "-") paths[VAD_DIR] = argv[2];
  if (argc > 7 && std::string(argv[7]) != "-") paths[PUNC_DIR] = argv[7];
  const int audio_fs = argc > 8 ? std::atoi(argv[8]) : 16000;      // the client's --audio-fs (funasr-wss-client.cpp:194,240,366)
  const int nbest = argc > 9 ? std::atoi(argv[9]) : 0;             // FunOfflineSetNbest for one extra pass (an extension)
  const int cif_stamps = argc > 10 ? std::atoi(argv[10]) : 0;      // FunOfflineSetCifStamps mode for one extra pass (an extension)
  const int batch = argc > 4 ? std::atoi(argv[4]) : 32, threads = argc > 5 ? std::atoi(argv[5]) : 1, repeat = argc > 6 ? std::atoi(argv[6]) : 1;
  std::ifstream f(argv[3], std::ios::binary);
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  FUNASR_HANDLE h = FunOfflineInit(paths, threads, true, batch);
  const std::vector<std::vector<float>> no_hw;
  {
    FUNASR_RESULT r = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, audio_fs, "pcm");
    if (!r) { std::fprintf(stderr, "inference failed\n"); return 1; }
    const auto& segs = FunASRGetSegments(r);
    const auto& ids = FunASRGetSegmentIds(r);
    for (size_t i = 0; i < segs.size(); ++i) {
      std::printf("seg %d %d :", segs[i].first, segs[i].second);
      for (int id : ids[i]) std::printf(" %d", id);
      std::printf("\n");
    }
    std::printf("text %s\nstamp %s\n", FunASRGetResult(r, 0), FunASRGetStamp(r));
    if (nbest > 0) {       // the same buffer once more with candidates on: its text, and the confidence of every token of the text
      std::printf("confidence_off %zu\n", FunASRGetTokenConfidence(r).size());
      FunOfflineSetNbest(h, nbest);
      FUNASR_RESULT q = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, audio_fs, "pcm");
      if (!q) { std::fprintf(stderr, "inference failed\n"); return 1; }
      std::printf("nbest_text %s\nconfidence", FunASRGetResult(q, 0));
      for (float c : FunASRGetTokenConfidence(q)) std::printf(" %.9g", c);
      std::printf("\n");
      FunASRFreeResult(q);
      FunOfflineSetNbest(h, 0);
    }
    if (cif_stamps > 0) {  // the same buffer once more with stamps from the CIF scan: "cif_text <text>", "cif_stamp <stamps>"
      FunOfflineSetCifStamps(h, cif_stamps);
      FUNASR_RESULT q = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, audio_fs, "pcm");
      if (!q) { std::fprintf(stderr, "inference failed\n"); return 1; }
      std::printf("cif_text %s\ncif_stamp %s\n", FunASRGetResult(q, 0), FunASRGetStamp(q));
      FunASRFreeResult(q);
      FunOfflineSetCifStamps(h, 0);
    }
    if (const char* lm = std::getenv("PFHIP_TOKEN_LM")) {
      const char *sc = std::getenv("PFHIP_TOKEN_LM_SCALE"), *bo = std::getenv("PFHIP_TOKEN_LM_BONUS");
      std::printf("lm_loaded %d\n", FunOfflineLoadTokenLm(h, lm, sc ? (float)std::atof(sc) : 1.0f, bo ? (float)std::atof(bo) : 0.0f));
    }
    if (argc > 12) {
      if (nbest > 0) FunOfflineSetNbest(h, nbest);
      if (cif_stamps > 0) FunOfflineSetCifStamps(h, cif_stamps);
      FUNASR_DEC_HANDLE dec = FunASRCtcDecoderInit(h, (float)std::atof(argv[11]), (float)std::atof(argv[12]), ASR_OFFLINE);
      std::printf("dec_handle %d\n", dec ? 1 : 0);
      std::unordered_map<std::string, int> hws;
      for (int a = 13; a + 1 < argc; a += 2) hws[argv[a]] = std::atoi(argv[a + 1]);
      for (const char* tag : {"dec", "hw"}) {
        if (std::string(tag) == "hw") std::printf("hw_loaded %d\n", FunCtcDecoderLoadHwsRes(dec, 0, hws));
        FUNASR_RESULT q = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, audio_fs, "pcm", true, 800, 60000, dec);
        if (!q) { std::fprintf(stderr, "inference failed\n"); return 1; }
        const auto& qsegs = FunASRGetSegments(q);
        const auto& qids = FunASRGetSegmentIds(q);
        for (size_t i = 0; i < qsegs.size(); ++i) {
          std::printf("%s_seg %d %d :", tag, qsegs[i].first, qsegs[i].second);
          for (int id : qids[i]) std::printf(" %d", id);
          std::printf("\n");
        }
        std::printf("%s_text %s\n%s_stamp %s\n%s_confidence", tag, FunASRGetResult(q, 0), tag, FunASRGetStamp(q), tag);
        for (float c : FunASRGetTokenConfidence(q)) std::printf(" %.9g", c);
        std::printf("\n");
        FunASRFreeResult(q);
      }
      FunCtcDecoderUninit(dec);
      FunOfflineSetNbest(h, 0);
      FunOfflineSetCifStamps(h, 0);
    }
    const std::string want_text = FunASRGetResult(r, 0), want_stamp = FunASRGetStamp(r);
    std::atomic<int> mismatches{0};
    const float secs = FunASRGetRetSnippetTime(r);
    FunASRFreeResult(r);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
      pool.emplace_back([&] {
        for (int k = 0; k < repeat; ++k) {
          FUNASR_RESULT q = FunOfflineInferBuffer(h, buf.data(), (int)buf.size(), RASR_NONE, nullptr, no_hw, audio_fs, "pcm");
          if (!q || want_text != FunASRGetResult(q, 0) || want_stamp != FunASRGetStamp(q)) {      // re-entrancy check
            if (mismatches++ == 0) std::fprintf(stderr, "differing text %s\nstamp %s\n", q ? FunASRGetResult(q, 0) : "(null)", q ? FunASRGetStamp(q) : "");
          }
          FunASRFreeResult(q);
        }
      });
    for (auto& th : pool) th.join();
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("audio %.1f s x %d files in %.3f s -> %.0f xRT\n", secs, threads * repeat, dt, secs * threads * repeat / dt);
    if (mismatches.load()) { std::fprintf(stderr, "%d concurrent results differ from the single-threaded one\n", mismatches.load()); return 3; }
  }
  FunOfflineUninit(h);
  return 0;
}
