// Robustness harness for the DNSMOS file reader (asr-2pass_amd/csrc/mos_files.cpp over model_files.cpp), built by
// tests/test_dnsmos_files.py with g++ -fsanitize=address,undefined (CPU only, no device, no library).
//   dnsmos_files_check primary <file.onnx> [iterations [seed]]
//   dnsmos_files_check p808 <file.onnx> <valid primary.onnx> [iterations [seed]]
// Loads the file as it is and prints "loaded <tensors bytes>" or "refused: <message>"; then, `iterations` times, loads a damaged copy
// of its bytes — a truncation, a run of flipped bytes, a length byte made huge.  Any outcome but "loaded" or "refused with a message"
// (a crash, an out-of-bounds read, undefined behaviour) ends the process with a sanitizer report and a non-zero code.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../../asr-2pass_amd/csrc/model_files.h"

namespace {
// a minimal valid partner so that either net can be the one under test
bool load(const std::vector<char>& bytes, bool primary, const std::vector<char>& partner, std::string* msg) {
  pfhip_files::Container c;
  try {
    if (primary) pfhip_files::load_dnsmos_bytes(bytes.data(), bytes.size(), nullptr, 0, c);
    else pfhip_files::load_dnsmos_bytes(partner.data(), partner.size(), bytes.data(), bytes.size(), c);
  } catch (const std::exception& e) {
    *msg = e.what();
    return false;
  }
  *msg = std::to_string(c.blob.size() * 4);
  return true;
}
std::vector<char> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: dnsmos_files_check <primary|p808> <file.onnx> [partner.onnx] [iterations [seed]]\n"); return 2; }
  const bool primary = std::strcmp(argv[1], "primary") == 0;
  const std::vector<char> good = slurp(argv[2]);
  int arg = 3;
  std::vector<char> partner;
  if (!primary) {
    if (argc < 4) { std::fprintf(stderr, "p808 needs the primary file as its partner\n"); return 2; }
    partner = slurp(argv[arg++]);
  }
  const int iters = argc > arg ? std::atoi(argv[arg]) : 0;
  std::mt19937 rng(argc > arg + 1 ? (unsigned)std::atoi(argv[arg + 1]) : 1u);
  std::string msg;
  const bool ok = load(good, primary, partner, &msg);
  std::printf("%s%s\n", ok ? "loaded " : "refused: ", msg.c_str());
  if (!ok && msg.empty()) { std::printf("refused without a message\n"); return 1; }
  int loaded = 0, refused = 0;
  for (int i = 0; i < iters && !good.empty(); ++i) {
    std::vector<char> b = good;
    switch (rng() % 3) {
      case 0: b.resize(rng() % b.size()); break;
      case 1: { const size_t at = rng() % b.size(), n = 1 + rng() % 8; for (size_t k = at; k < at + n && k < b.size(); ++k) b[k] = (char)(rng() & 0xFF); break; }
      default: { const size_t at = rng() % std::min<size_t>(b.size(), 4096); b[at] = (char)0xFF; if (at + 1 < b.size()) b[at + 1] = (char)0xFF; break; }
    }
    const bool r = load(b, primary, partner, &msg);
    if (!r && msg.empty()) { std::printf("iteration %d refused without a message\n", i); return 1; }
    (r ? loaded : refused)++;
  }
  if (iters) std::printf("damaged: %d loaded, %d refused\n", loaded, refused);
  return 0;
}
