// The ARPA reader of the token n-gram language model (asr-2pass_amd/csrc/lm_graph.cpp) over a fixed list of damaged texts, as a
// stand-alone program for the address and undefined-behaviour sanitizers: host code only, no device, no library, no Python.
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       asr-2pass_amd/csrc/lm_graph.cpp tools/fuzz/lm_arpa_fuzz.cpp -o lm_arpa_fuzz && ./lm_arpa_fuzz <scratch directory>
// Every text must be either read (then the graph is dumped and walked, so that every index it holds is used) or refused with
// PFHIP_ERR_ARG and a message; the sanitizers say the rest.  Exit status 0: all texts behaved; the count is printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pfhip.h"

namespace pfhip_impl {
std::string& last_error() {                      // what lm_graph.cpp expects of the library around it
  static thread_local std::string e;
  return e;
}
}  // namespace pfhip_impl

namespace {

int g_failed = 0;
#define CHECK(c) \
  do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_case); ++g_failed; } } while (0)
const char* g_case = "";

constexpr int kVocab = 5;
const char* const kTokens[kVocab] = {"a", "b", "c", "b", "\xe7\x9a\x84"};

const std::string kGood =
    "\n\\data\\\nngram 1=5\nngram 2=3\nngram 3=1\n\n\\1-grams:\n-1.0\ta\t-0.5\n-0.7\tb\t-0.2\n-1.2\t\xe7\x9a\x84\t-0.1\n-99\t<s>\t-0.3\n-1.1\t</s>\n\n"
    "\\2-grams:\n-0.3\t<s> a\t-0.2\n-0.4\ta b\t-0.1\n-0.2\tb </s>\n\n\\3-grams:\n-0.1\t<s> a b\n\n\\end\\\n";

// a graph that was built: every index inside its arrays, every weight finite, every state reachable by a bounded walk
void walk(const pfhip_lm_graph* g) {
  int S = 0, A = 0, start = 0, eos = 0;
  CHECK(pfhip_lm_graph_dump(g, &S, &A, &start, &eos, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) == PFHIP_OK);
  const int U = pfhip_lm_graph_vocab(g) + 1;
  CHECK(U == kVocab + 1 && S >= 1 && A >= 0 && start >= 0 && start < S);
  std::vector<float> uni_w(U), back_w(S), arc_w(A + 1);
  std::vector<int32_t> uni_next(U), begin(S + 1), back_s(S), label(A + 1), next(A + 1);
  CHECK(pfhip_lm_graph_dump(g, &S, &A, &start, &eos, uni_w.data(), uni_next.data(), U, begin.data(), back_w.data(), back_s.data(), S, label.data(),
                            next.data(), arc_w.data(), A) == PFHIP_OK);
  CHECK(pfhip_lm_graph_dump(g, &S, &A, &start, &eos, uni_w.data(), uni_next.data(), U - 1, begin.data(), back_w.data(), back_s.data(), S,
                            label.data(), next.data(), arc_w.data(), A) == PFHIP_ERR_CAPACITY);
  CHECK(begin[0] == 0 && begin[S] == A);
  for (int u = 0; u < U; ++u) CHECK(std::isfinite(uni_w[u]) && uni_next[u] >= 0 && uni_next[u] < S);
  for (int s = 0; s < S; ++s) {
    CHECK(begin[s] <= begin[s + 1] && std::isfinite(back_w[s]) && back_s[s] >= 0 && (s == 0 || back_s[s] < s));
    for (int a = begin[s]; a < begin[s + 1]; ++a) {
      CHECK(label[a] >= 0 && label[a] < U && next[a] >= 0 && next[a] < S && std::isfinite(arc_w[a]));
      if (a > begin[s]) CHECK(label[a - 1] < label[a]);
    }
  }
}

void run(const char* name, const std::string& text, const std::string& dir, bool must_refuse) {
  g_case = name;
  const std::string path = dir + "/lm_arpa_fuzz.arpa";
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
  if (!text.empty()) CHECK(std::fwrite(text.data(), 1, text.size(), f) == text.size());
  std::fclose(f);
  pfhip_lm_graph* g = reinterpret_cast<pfhip_lm_graph*>(1);
  long long skipped = -1;
  pfhip_impl::last_error().clear();
  const pfhip_status st = pfhip_lm_graph_create_from_arpa(path.c_str(), kTokens, kVocab, 0.5f, 0.25f, -8.f, &g, &skipped);
  if (st == PFHIP_OK) {
    CHECK(!must_refuse);
    CHECK(g != nullptr && skipped >= 0);
    if (g) walk(g);
    pfhip_lm_graph_destroy(g);
  } else {
    CHECK(st == PFHIP_ERR_ARG && g == nullptr && !pfhip_impl::last_error().empty());
  }
  std::remove(path.c_str());
}

std::string replaced(std::string s, const std::string& what, const std::string& with) {
  const size_t at = s.find(what);
  if (at == std::string::npos) { std::fprintf(stderr, "no '%s' in the good text\n", what.c_str()); std::exit(2); }
  return s.replace(at, what.size(), with);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  int n = 0;
  auto go = [&](const char* name, const std::string& text, bool must_refuse) { run(name, text, dir, must_refuse); ++n; };
  go("good", kGood, false);
  go("good, CRLF", [&] { std::string s; for (char c : kGood) { if (c == '\n') s += '\r'; s += c; } return s; }(), false);
  go("empty", "", true);
  // truncated at every byte: each prefix is read to its end, none of them past it
  for (size_t cut = 1; cut < kGood.size(); ++cut) go("truncated", kGood.substr(0, cut), cut + 1 < kGood.size());
  go("huge count", replaced(kGood, "ngram 2=3", "ngram 2=1073741823"), true);
  go("count beyond int32", replaced(kGood, "ngram 2=3", "ngram 2=4294967299"), true);
  go("count beyond int64", replaced(kGood, "ngram 2=3", "ngram 2=99999999999999999999999999"), true);
  go("counts whose product is beyond int32", replaced(kGood, "ngram 3=1", "ngram 3=900000000"), true);
  go("negative count", replaced(kGood, "ngram 2=3", "ngram 2=-3"), true);
  go("negative order", replaced(kGood, "ngram 2=3", "ngram -2=3"), true);
  go("order above the cap", replaced(kGood, "ngram 3=1\n", "ngram 3=1\nngram 4=0\nngram 5=0\nngram 6=0\nngram 7=0\n"), true);
  go("no count", replaced(kGood, "ngram 2=3", "ngram 2="), true);
  go("a line of 10^6 characters in a section", replaced(kGood, "-0.4\ta b", "-0.4\t" + std::string(1000000, 'a') + " b"), false);
  go("a line of 10^6 fields", replaced(kGood, "-0.4\ta b", "-0.4\t" + [] { std::string s; for (int i = 0; i < 500000; ++i) s += "a "; return s; }()), true);
  go("a number of 10^6 characters", replaced(kGood, "-0.4\ta b", std::string(1000000, '1') + "\ta b"), true);
  go("a line of 10^6 characters before the data", std::string(1000000, 'x') + kGood, false);
  go("a count line of 10^6 characters", replaced(kGood, "ngram 2=3", "ngram 2=" + std::string(1000000, '3')), true);
  go("NUL in a word", replaced(kGood, "-0.4\ta b", std::string("-0.4\ta\0 b", 9)), false);
  go("NUL in a number", replaced(kGood, "-0.4\ta b", std::string("-0.\0" "4\ta b", 9)), true);
  go("NUL in a count", replaced(kGood, "ngram 2=3", std::string("ngram 2=\0" "3", 10)), true);
  go("NULs alone", std::string(4096, '\0'), true);
  go("NUL behind the data line", replaced(kGood, "\\data\\\n", std::string("\\data\\\0\n", 8)), true);
  go("nan", replaced(kGood, "-0.4\ta b", "nan\ta b"), true);
  go("inf", replaced(kGood, "-0.2\tb </s>", "-inf\tb </s>"), true);
  go("hex float", replaced(kGood, "-0.4\ta b", "-0x1p-1\ta b"), false);
  go("overflowing exponent", replaced(kGood, "-0.4\ta b", "-1e99999\ta b"), true);
  go("a weight beyond float", replaced(kGood, "-0.4\ta b", "-9e38\ta b"), true);
  go("too few fields", replaced(kGood, "-0.2\tb </s>", "-0.2\tb"), true);
  go("too many fields", replaced(kGood, "-0.1\t<s> a b", "-0.1\t<s> a b\t-0.1\t-0.1"), true);
  go("a section twice", replaced(kGood, "\\3-grams:", "\\2-grams:"), true);
  go("sections out of turn", replaced(replaced(kGood, "\\2-grams:", "\\9-grams:"), "\\3-grams:", "\\2-grams:"), true);
  go("an n-gram twice", replaced(kGood, "-0.2\tb </s>", "-0.2\ta b"), true);
  go("an unknown word and <unk> above order 1", replaced(replaced(kGood, "-0.4\ta b", "-0.4\ta zzz"), "-0.2\tb </s>", "-0.2\t<unk> </s>"), false);
  go("a history that is not listed", replaced(kGood, "-0.3\t<s> a", "-0.3\tb a"), false);
  go("no end line", replaced(kGood, "\\end\\", "\\end"), true);
  go("text behind the end line", kGood + "trailing\n\\1-grams:\n" + std::string(1000, '\xff'), false);
  go("bytes above 127 everywhere", [] { std::string s(8192, ' '); for (size_t i = 0; i < s.size(); ++i) s[i] = (char)(128 + i % 128); return s; }(), true);
  if (g_failed) { std::fprintf(stderr, "lm_arpa_fuzz: %d checks failed\n", g_failed); return 1; }
  std::printf("lm_arpa_fuzz: %d texts behaved\n", n);
  return 0;
}
