// test_kmer_wide.cpp -- the multi-word k-mer key (csrc/msgpu_kmer_wide.h) on the host, against vectors worked out on Python
// integers (tests/golden/unitigs_wide/key_vectors.txt, written by tools/make_unitig_wide_fixtures.py, which describes the
// format): the mask, <, ==, the shifts by 2 and by top as operators and as the carried steps the kernels use (push_low,
// push_high), the base at every position, the reverse complement and the rolling window over a sequence with an N in it, at
// k = 65, 66, 95, 96 (three words) and 97, 127, 128 (four).  Built with the undefined-behaviour sanitizer, so a shift by the
// word width or more anywhere in the header ends the run with a report.  A host program: no device code, nothing preloaded.
//   test_kmer_wide <key_vectors.txt>  -> "ok <checks>" and exit status 0, or the first mismatches and 1
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "msgpu_kmer_wide.h"

using namespace msgpu;

static long checks = 0, failures = 0;

static void fail(int k, const char *what, const std::string &line) {
  if (++failures <= 20) fprintf(stderr, "k = %d: %s: %s\n", k, what, line.c_str());
}

// up to 64 hexadecimal digits -> the key; the words above W must be zero
template <int W> static bool parse(const std::string &digits, KfWide<W> &out) {
  if (digits.empty() || digits.size() > 64) return false;
  const std::string hex = std::string(64 - digits.size(), '0') + digits;
  for (int i = 0; i < 4; ++i) {
    const uint64_t w = strtoull(hex.substr(16 * (3 - i), 16).c_str(), nullptr, 16);
    if (i < W) out.w[i] = w;
    else if (w) return false;
  }
  return true;
}

template <int W> static void expect(int k, bool ok, const char *what, const std::string &line) {
  ++checks;
  if (!ok) fail(k, what, line);
}

template <int W> static void run_block(int k, const std::vector<std::string> &lines) {
  typedef KfWide<W> K;
  const int top = 2 * (k - 1);
  const K   mask = kf_mask<K>(k);
  for (size_t at = 0; at < lines.size(); ++at) {
    const std::string &line = lines[at];
    std::istringstream in(line);
    std::string        name;
    in >> name;
    if (name == "mask") {
      std::string m;
      in >> m;
      K want;
      expect<W>(k, parse(m, want) && mask == want && K::mask(k) == want, "mask", line);
      expect<W>(k, mask.w[W - 1] == K::top_word_mask(k) && K::top_word_shift(k) == top - 64 * (W - 1), "top word", line);
    } else if (name == "ops") {
      std::string xs, succ_s, pred_s, down_s, rc_s, text, ys;
      uint32_t    c;
      int         lt, eq;
      in >> xs >> c >> succ_s >> pred_s >> down_s >> rc_s >> text >> ys >> lt >> eq;
      K x, succ, pred, down, rc, y;
      expect<W>(k, parse(xs, x) && parse(succ_s, succ) && parse(pred_s, pred) && parse(down_s, down) && parse(rc_s, rc) && parse(ys, y),
                "parse", line);
      expect<W>(k, (x < y) == (lt != 0) && (y > x) == (lt != 0), "<", line);
      expect<W>(k, (x == y) == (eq != 0) && (x != y) == (eq == 0), "==", line);
      expect<W>(k, ((x | y) & x) == x && ((x & y) | x) == x && (~(~x)) == x && ((x & ~x) == K(0)), "| & ~", line);
      expect<W>(k, (((x << 2) | K(c)) & mask) == succ, "(x << 2 | c) & mask", line);
      expect<W>(k, ((x >> 2) | (K(c) << top)) == pred, "x >> 2 | c << top", line);
      expect<W>(k, (x >> top) == down, "x >> top", line);
      K s = x;
      s.push_low(c, K::top_word_mask(k));
      expect<W>(k, s == succ, "push_low", line);
      s = x;
      s.push_high(c, K::top_word_shift(k));
      expect<W>(k, s == pred, "push_high", line);
      expect<W>(k, ug_rc(x, k) == rc && ug_rc(rc, k) == x, "ug_rc", line);
      std::string got(static_cast<size_t>(k), '?');
      for (int j = 0; j < k; ++j) got[static_cast<size_t>(j)] = "ACGT"[kf_base(x, k - 1 - j)];
      expect<W>(k, got == text && static_cast<uint32_t>(x) == static_cast<uint32_t>(x.w[0]), "kf_base", line);
      uint64_t hi, lo, words[W];
      key_split(x, hi, lo);
      key_words(x, words);
      expect<W>(k, lo == x.w[0] && hi == x.w[1] && words[W - 1] == x.w[W - 1], "key_split", line);
    } else if (name == "roll") {
      std::string seq;
      size_t      n;
      in >> seq >> n;
      KfRoll<K> roll(k);
      K         key;
      size_t    got = 0;
      for (char ch : seq) {
        if (!roll.step(static_cast<uint8_t>(ch), key)) continue;
        K                  want;
        std::istringstream kl(at + 1 + got < lines.size() ? lines[at + 1 + got] : std::string());
        std::string        tag, hex;
        kl >> tag >> hex;
        expect<W>(k, got < n && tag == "key" && parse(hex, want) && key == want, "roll", hex);
        ++got;
      }
      expect<W>(k, got == n && n > 0, "windows", line);
      at += n;
    } else {
      fail(k, "unknown line", line);
    }
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: test_kmer_wide <key_vectors.txt>\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<std::pair<int, std::vector<std::string>>> blocks;
  for (std::string line; std::getline(f, line);) {
    if (line.compare(0, 2, "k ") == 0) blocks.push_back({atoi(line.c_str() + 2), {}});
    else if (!blocks.empty() && !line.empty()) blocks.back().second.push_back(line);
  }
  int seen3 = 0, seen4 = 0;
  for (const auto &b : blocks) {
    if (b.first >= 65 && b.first <= 96) run_block<3>(b.first, b.second), ++seen3;
    else if (b.first >= 97 && b.first <= 128) run_block<4>(b.first, b.second), ++seen4;
    else fail(b.first, "k outside 65..128", "");
  }
  if (!seen3 || !seen4 || failures) {
    fprintf(stderr, "%ld of %ld checks failed (%d blocks of three words, %d of four)\n", failures, checks, seen3, seen4);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
