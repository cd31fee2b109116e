// The token n-gram language model of the device searches (pfhip_lm_graph_*, include/pfhip.h): host only, no HIP include, so that it
// builds stand-alone (tools/fuzz/lm_arpa_fuzz.cpp links this file alone and brings its own pfhip_impl::last_error).
//
// An ARPA back-off model scores a token w after a history h as p(h, w) where the n-gram (h, w) is listed, else as backoff(h) +
// score(w after h without its oldest label).  As an automaton: one state per listed history, one arc per listed n-gram, and the
// back-off as a weight and a state to fall to.  The n-grams of one length are sorted lexicographically (oldest label first), which
// numbers the states, groups the arcs of a state together and sorts them by label in one go.  Every weight is formed once, here, in
// double and rounded to float once (bake below): the device only adds.  tests/lm_ref.py restates all of it.
#include "lm_graph.h"

#include "../../include/pfhip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>

namespace pfhip_impl {
std::string& last_error();                       // thread-local, pfhip.cpp (a stand-alone program brings its own)
}

namespace {

constexpr long long kIndexMax = 0x3fffffffLL;    // labels, states and arcs are int32 indices
constexpr double kLn10 = 2.302585092994046;

pfhip_status refuse(const std::string& msg) {
  pfhip_impl::last_error() = msg;
  return PFHIP_ERR_ARG;
}

// fl32((log10 * ln10) * scale + bonus): three double operations in three statements through a volatile, so that no compiler fuses
// two of them, and one rounding to float
float bake(double log10v, double scale, double bonus) {
  volatile double t = log10v * kLn10;
  t = t * scale;
  t = t + bonus;
  return (float)t;
}

struct Gram {
  const int32_t* lab;
  double p, b;
};

int compare(const int32_t* a, const int32_t* b, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}

// the position of the n-gram lab[0 .. n) in the sorted list of its length, or -1
int find(const std::vector<Gram>& sorted, const int32_t* lab, int n) {
  size_t lo = 0, hi = sorted.size();
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (compare(sorted[mid].lab, lab, n) < 0) lo = mid + 1; else hi = mid;
  }
  return lo < sorted.size() && compare(sorted[lo].lab, lab, n) == 0 ? (int)lo : -1;
}

}  // namespace

extern "C" {

pfhip_status pfhip_lm_graph_create(int order, const int* n_grams, const int32_t* labels, const double* log10_prob, const double* log10_backoff,
                                   int vocab, float scale, float token_bonus, float oov_log10, pfhip_lm_graph** g) {
  if (!g) return refuse("pfhip_lm_graph_create: no output handle");
  *g = nullptr;
  if (order < 1 || order > PFHIP_LM_ORDER_MAX) return refuse("pfhip_lm_graph_create: the order must be 1 .. " + std::to_string(PFHIP_LM_ORDER_MAX));
  if (!n_grams) return refuse("pfhip_lm_graph_create: no n-gram counts");
  if (vocab < 1 || vocab > kIndexMax - 3) return refuse("pfhip_lm_graph_create: vocab outside 1 .. 2^30 - 4");
  if (!std::isfinite(scale) || !std::isfinite(token_bonus) || !std::isfinite(oov_log10))
    return refuse("pfhip_lm_graph_create: scale, token_bonus and oov_log10 must be finite");
  long long n_all = 0, n_labels = 0;
  for (int n = 1; n <= order; ++n) {
    const long long c = n_grams[n - 1];
    if (c < 0) return refuse("pfhip_lm_graph_create: a negative n-gram count");
    if (c > kIndexMax) return refuse("pfhip_lm_graph_create: too many n-grams for int32 indices");
    n_all += c;                                                      // <= 6 * 2^30
    n_labels += c * n;                                               // <= 21 * 2^30
    if (n_all + vocab > kIndexMax || n_labels > kIndexMax) return refuse("pfhip_lm_graph_create: too many n-grams for int32 indices");
  }
  if (n_all > 0 && (!labels || !log10_prob || !log10_backoff)) return refuse("pfhip_lm_graph_create: a missing array");
  const int V = vocab, kEos = vocab, kBos = vocab + 1, kUnk = vocab + 2;
  const double sc = scale, bonus = token_bonus;

  // ---- the n-grams of every length, validated, sorted, those without a listed history dropped
  std::vector<std::vector<Gram>> kept((size_t)order + 1);
  bool have_unk = false;
  double unk_p = 0.0;
  {
    size_t at = 0, idx = 0;
    for (int n = 1; n <= order; ++n) {
      std::vector<Gram>& list = kept[n];
      for (int i = 0; i < n_grams[n - 1]; ++i, at += n, ++idx) {
        const int32_t* lab = labels + at;
        const double p = log10_prob[idx], b = log10_backoff[idx];
        if (!std::isfinite(p) || !std::isfinite(b)) return refuse("pfhip_lm_graph_create: a non-finite probability or back-off weight");
        for (int j = 0; j < n; ++j) {
          if (lab[j] < 0 || lab[j] > kUnk) return refuse("pfhip_lm_graph_create: a label outside 0 .. vocab + 2");
          if (lab[j] == kUnk && n > 1) return refuse("pfhip_lm_graph_create: <unk> (vocab + 2) above order 1");
        }
        if (lab[n - 1] == kUnk) {
          if (have_unk) return refuse("pfhip_lm_graph_create: an n-gram listed twice");
          have_unk = true; unk_p = p;
          continue;
        }
        if (n > 1 && lab[n - 1] == kBos) continue;                   // predicts <s>
        list.push_back({lab, p, b});
      }
      std::sort(list.begin(), list.end(), [n](const Gram& x, const Gram& y) { return compare(x.lab, y.lab, n) < 0; });
      for (size_t i = 1; i < list.size(); ++i)
        if (compare(list[i - 1].lab, list[i].lab, n) == 0) return refuse("pfhip_lm_graph_create: an n-gram listed twice");
      if (n > 1) {
        size_t w = 0;
        for (size_t i = 0; i < list.size(); ++i)
          if (find(kept[n - 1], list[i].lab, n - 1) >= 0) list[w++] = list[i];
        list.resize(w);
      }
    }
  }

  // ---- states: 0, then the kept n-grams of length 1 .. order - 1 in their sorted order
  std::vector<long long> base((size_t)order + 1, 0);
  long long S = 1;
  for (int m = 1; m < order; ++m) { base[m] = S; S += (long long)kept[m].size(); }
  long long A = 0;
  for (int n = 2; n <= order; ++n) A += (long long)kept[n].size();
  if (S > kIndexMax || A > kIndexMax) return refuse("pfhip_lm_graph_create: too many n-grams for int32 indices");
  // the longest suffix of lab[0 .. len) that is a state
  auto state_of = [&](const int32_t* lab, int len) -> int {
    for (int m = std::min(len, order - 1); m >= 1; --m) {
      const int i = find(kept[m], lab + len - m, m);
      if (i >= 0) return (int)(base[m] + i);
    }
    return 0;
  };

  pfhip_lm_graph* out = new (std::nothrow) pfhip_lm_graph;
  if (!out) return refuse("pfhip_lm_graph_create: out of memory");
  struct Guard { pfhip_lm_graph* p; ~Guard() { delete p; } } guard{out};
  out->vocab = V; out->order = order;
  bool finite = true;
  auto checked = [&](float w) { finite = finite && std::isfinite(w); return w; };

  const float miss = checked(bake(have_unk ? unk_p : (double)oov_log10, sc, bonus));
  out->uni_w.assign((size_t)V + 1, miss);
  out->uni_w[V] = 0.f;                                               // never read unless has_eos
  out->uni_next.assign((size_t)V + 1, 0);
  for (size_t i = 0; i < kept[1].size(); ++i) {
    const Gram& u = kept[1][i];
    const int w = u.lab[0];
    if (w == kBos) { if (order > 1) out->start = (int)(base[1] + (long long)i); continue; }
    out->uni_w[w] = checked(bake(u.p, sc, w == kEos ? 0.0 : bonus));
    out->uni_next[w] = order > 1 ? (int32_t)(base[1] + (long long)i) : 0;
    if (w == kEos) out->has_eos = 1;
  }

  out->backoff_w.assign((size_t)S, 0.f);
  out->backoff_state.assign((size_t)S, 0);
  out->arc_begin.assign((size_t)S + 1, 0);
  out->arc_label.reserve((size_t)A); out->arc_next.reserve((size_t)A); out->arc_weight.reserve((size_t)A);
  for (int m = 1; m < order; ++m) {
    for (size_t i = 0; i < kept[m].size(); ++i) {
      const size_t s = (size_t)base[m] + i;
      out->backoff_w[s] = checked(bake(kept[m][i].b, sc, 0.0));
      const int back = state_of(kept[m][i].lab + 1, m - 1);
      if (back >= base[m]) return refuse("pfhip_lm_graph_create: a back-off state that is not a shorter history");    // cannot happen
      out->backoff_state[s] = back;
    }
    // the (m + 1)-grams are sorted by history first: the arcs of one state lie together, states in order, labels ascending
    for (const Gram& a : kept[m + 1]) {
      const size_t s = (size_t)base[m] + (size_t)find(kept[m], a.lab, m);
      const int w = a.lab[m];
      out->arc_begin[s + 1] += 1;
      out->arc_label.push_back(w);
      out->arc_next.push_back(state_of(a.lab, m + 1));
      out->arc_weight.push_back(checked(bake(a.p, sc, w == kEos ? 0.0 : bonus)));
    }
  }
  for (size_t s = 0; s < (size_t)S; ++s) out->arc_begin[s + 1] += out->arc_begin[s];
  if (!finite) return refuse("pfhip_lm_graph_create: a weight that is not finite in fp32 after scaling");

  auto words = [&](const void* src, size_t n) {
    const size_t at = out->packed.size();
    out->packed.resize(at + n);
    if (n) std::memcpy(out->packed.data() + at, src, 4 * n);
  };
  words(out->uni_w.data(), out->uni_w.size());
  words(out->uni_next.data(), out->uni_next.size());
  words(out->arc_begin.data(), out->arc_begin.size());
  words(out->backoff_w.data(), out->backoff_w.size());
  words(out->backoff_state.data(), out->backoff_state.size());
  words(out->arc_label.data(), out->arc_label.size());
  words(out->arc_next.data(), out->arc_next.size());
  words(out->arc_weight.data(), out->arc_weight.size());
  guard.p = nullptr;
  *g = out;
  return PFHIP_OK;
}

void pfhip_lm_graph_destroy(pfhip_lm_graph* g) { delete g; }

int pfhip_lm_graph_vocab(const pfhip_lm_graph* g) { return g ? g->vocab : 0; }

int pfhip_lm_graph_order(const pfhip_lm_graph* g) { return g ? g->order : 0; }

pfhip_status pfhip_lm_graph_dump(const pfhip_lm_graph* g, int* n_states, int* n_arcs, int* start, int* has_eos, float* uni_w, int32_t* uni_next,
                                 int cap_uni, int32_t* arc_begin, float* backoff_w, int32_t* backoff_state, int cap_states, int32_t* arc_label,
                                 int32_t* arc_next, float* arc_weight, int cap_arcs) {
  if (!g || !n_states || !n_arcs || !start || !has_eos) return PFHIP_ERR_ARG;
  *n_states = g->n_states();
  *n_arcs = g->n_arcs();
  *start = g->start;
  *has_eos = g->has_eos;
  const bool none = !uni_w && !uni_next && !arc_begin && !backoff_w && !backoff_state && !arc_label && !arc_next && !arc_weight;
  if (none) return PFHIP_OK;                                         // the counts alone
  if (!uni_w || !uni_next || !arc_begin || !backoff_w || !backoff_state || !arc_label || !arc_next || !arc_weight) return PFHIP_ERR_ARG;
  if (cap_uni < g->vocab + 1 || cap_states < g->n_states() || cap_arcs < g->n_arcs()) return PFHIP_ERR_CAPACITY;
  std::copy(g->uni_w.begin(), g->uni_w.end(), uni_w);
  std::copy(g->uni_next.begin(), g->uni_next.end(), uni_next);
  std::copy(g->arc_begin.begin(), g->arc_begin.end(), arc_begin);
  std::copy(g->backoff_w.begin(), g->backoff_w.end(), backoff_w);
  std::copy(g->backoff_state.begin(), g->backoff_state.end(), backoff_state);
  std::copy(g->arc_label.begin(), g->arc_label.end(), arc_label);
  std::copy(g->arc_next.begin(), g->arc_next.end(), arc_next);
  std::copy(g->arc_weight.begin(), g->arc_weight.end(), arc_weight);
  return PFHIP_OK;
}

// ---- the ARPA reader: text in, the arrays of pfhip_lm_graph_create out
pfhip_status pfhip_lm_graph_create_from_arpa(const char* path, const char* const* tokens, int vocab, float scale, float token_bonus,
                                             float oov_log10, pfhip_lm_graph** g, long long* n_skipped) {
  if (!g) return refuse("pfhip_lm_graph_create_from_arpa: no output handle");
  *g = nullptr;
  if (n_skipped) *n_skipped = 0;
  if (!path || !tokens) return refuse("pfhip_lm_graph_create_from_arpa: no path or no token strings");
  if (vocab < 1 || vocab > kIndexMax - 3) return refuse("pfhip_lm_graph_create_from_arpa: vocab outside 1 .. 2^30 - 4");
  std::string text;
  {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return refuse(std::string("pfhip_lm_graph_create_from_arpa: cannot open ") + path);
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) return refuse(std::string("pfhip_lm_graph_create_from_arpa: cannot read ") + path);
  }
  std::unordered_map<std::string, int32_t> word_id;
  for (int i = 0; i < vocab; ++i) {
    if (!tokens[i]) return refuse("pfhip_lm_graph_create_from_arpa: a missing token string");
    word_id.emplace(tokens[i], i);                                   // the lowest id of duplicates stays
  }
  word_id["</s>"] = vocab; word_id["<s>"] = vocab + 1; word_id["<unk>"] = vocab + 2;

  size_t pos = 0;
  long long line_no = 0;
  std::vector<std::pair<size_t, size_t>> field;                      // (begin, length) of the fields of the current line
  // the next line, split at blanks and tabs (a trailing \r dropped); false at the end of the text
  auto next_line = [&]() -> bool {
    field.clear();
    if (pos >= text.size()) return false;
    const char* nl = static_cast<const char*>(std::memchr(text.data() + pos, '\n', text.size() - pos));
    size_t end = nl ? (size_t)(nl - text.data()) : text.size();
    const size_t after = nl ? end + 1 : end;
    if (end > pos && text[end - 1] == '\r') --end;
    size_t i = pos;
    while (i < end) {
      while (i < end && (text[i] == ' ' || text[i] == '\t')) ++i;
      const size_t b = i;
      while (i < end && text[i] != ' ' && text[i] != '\t') ++i;
      if (i > b) field.emplace_back(b, i - b);
    }
    pos = after;
    ++line_no;
    return true;
  };
  auto is = [&](size_t k, const char* s) { return field[k].second == std::strlen(s) && std::memcmp(text.data() + field[k].first, s, field[k].second) == 0; };
  auto at_line = [&]() { return " (line " + std::to_string(line_no) + ")"; };
  // a whole field as a finite number
  auto number = [&](size_t k, double* v) {
    const std::string s(text, field[k].first, field[k].second);
    if (s.size() != std::strlen(s.c_str()) || s.size() > 64) return false;        // a NUL inside, or no number is that long
    char* e = nullptr;
    *v = std::strtod(s.c_str(), &e);
    return e == s.c_str() + s.size() && std::isfinite(*v);
  };

  bool data = false;
  while (next_line())
    if (field.size() == 1 && is(0, "\\data\\")) { data = true; break; }
  if (!data) return refuse("pfhip_lm_graph_create_from_arpa: no \\data\\ line");
  // ---- "ngram N=count" lines, N = 1, 2, ... in order
  std::vector<long long> declared;
  bool more = false;
  while ((more = next_line())) {
    if (field.empty()) continue;
    if (!(field.size() == 2 && is(0, "ngram"))) break;
    const std::string s(text, field[1].first, field[1].second);
    const size_t eq = s.find('=');
    if (eq == std::string::npos || eq == 0 || eq + 1 >= s.size() || s.size() > 40 || s.size() != std::strlen(s.c_str()))
      return refuse("pfhip_lm_graph_create_from_arpa: a malformed ngram count" + at_line());
    char *e1 = nullptr, *e2 = nullptr;
    const long long n = std::strtoll(s.c_str(), &e1, 10), c = std::strtoll(s.c_str() + eq + 1, &e2, 10);
    if (e1 != s.c_str() + eq || e2 != s.c_str() + s.size()) return refuse("pfhip_lm_graph_create_from_arpa: a malformed ngram count" + at_line());
    if (n != (long long)declared.size() + 1) return refuse("pfhip_lm_graph_create_from_arpa: ngram orders must be 1, 2, ... in turn" + at_line());
    if (n > PFHIP_LM_ORDER_MAX) return refuse("pfhip_lm_graph_create_from_arpa: an order above " + std::to_string(PFHIP_LM_ORDER_MAX) + at_line());
    if (c < 0) return refuse("pfhip_lm_graph_create_from_arpa: a negative ngram count" + at_line());
    if (c > kIndexMax) return refuse("pfhip_lm_graph_create_from_arpa: an ngram count too large for int32 indices" + at_line());
    declared.push_back(c);
  }
  const int order = (int)declared.size();
  if (order < 1) return refuse("pfhip_lm_graph_create_from_arpa: no ngram counts after \\data\\");
  {
    long long n_labels = 0;
    for (int n = 1; n <= order; ++n) {
      n_labels += declared[n - 1] * n;                               // <= 21 * 2^30
      if (n_labels > kIndexMax) return refuse("pfhip_lm_graph_create_from_arpa: ngram counts too large for int32 indices");
    }
  }
  // ---- the sections; `field` holds the first line behind the counts
  std::vector<int> n_kept((size_t)order, 0);
  std::vector<int32_t> labels;
  std::vector<double> prob, backoff;
  long long skipped = 0;
  bool ended = false;
  for (int n = 1; n <= order; ++n) {
    while (more && field.empty()) more = next_line();
    const std::string head = "\\" + std::to_string(n) + "-grams:";
    if (!more || field.size() != 1 || !is(0, head.c_str())) return refuse("pfhip_lm_graph_create_from_arpa: expected " + head + at_line());
    long long seen = 0;
    std::vector<int32_t> lab((size_t)n);
    while ((more = next_line())) {
      if (field.empty()) continue;
      if (text[field[0].first] == '\\') break;                       // the next section or \end\ (a number never starts so)
      if (field.size() != (size_t)n + 1 && field.size() != (size_t)n + 2)
        return refuse("pfhip_lm_graph_create_from_arpa: a line of " + std::to_string(field.size()) + " fields in " + head + at_line());
      ++seen;
      if (seen > declared[n - 1]) return refuse("pfhip_lm_graph_create_from_arpa: more lines in " + head + " than its count" + at_line());
      double p = 0.0, b = 0.0;
      if (!number(0, &p) || (field.size() == (size_t)n + 2 && !number((size_t)n + 1, &b)))
        return refuse("pfhip_lm_graph_create_from_arpa: not a finite number" + at_line());
      bool known = true;
      for (int j = 0; j < n && known; ++j) {
        const auto it = word_id.find(std::string(text, field[(size_t)j + 1].first, field[(size_t)j + 1].second));
        if (it == word_id.end() || (it->second == vocab + 2 && n > 1)) known = false;
        else lab[(size_t)j] = it->second;
      }
      if (!known) { ++skipped; continue; }
      labels.insert(labels.end(), lab.begin(), lab.end());
      prob.push_back(p); backoff.push_back(b);
      ++n_kept[(size_t)n - 1];
    }
    if (seen != declared[n - 1])
      return refuse("pfhip_lm_graph_create_from_arpa: " + head + " has " + std::to_string(seen) + " lines, its count says " +
                    std::to_string(declared[n - 1]));
  }
  if (more && field.size() == 1 && is(0, "\\end\\")) ended = true;
  if (!ended) return refuse("pfhip_lm_graph_create_from_arpa: no \\end\\ line behind the last section" + at_line());
  if (n_skipped) *n_skipped = skipped;
  return pfhip_lm_graph_create(order, n_kept.data(), labels.data(), prob.data(), backoff.data(), vocab, scale, token_bonus, oov_log10, g);
}

}  // extern "C"
