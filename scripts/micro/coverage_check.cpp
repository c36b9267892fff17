// The text side of --coverage (wfmash_amd/host/coverage_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/coverage_check.cpp -o /tmp/coverage_check && /tmp/coverage_check
// coverage_bedgraph on hand-made intervals with known files (an interval across two sequence boundaries, an untouched sequence, a
// sequence of length 0, no intervals at all, a first interval behind 0), then on 20000 random interval lists held against a dense
// depth array; --coverage-paf's line handling (classify_line) on fixed lines with known answers, then on every prefix of a good line and
// 200000 random mutations of it: one of its five codes, and where it says LINE_ADD the runs' target bases are te - ts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/coverage_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}

static const std::vector<std::string> NAMES = {"t#1#chr1", "t#1#chr2", "t#1#none"};
static const std::vector<uint64_t> LENGTHS = {9000, 500, 70};
static int find_name(const std::string& n) {
  for (size_t i = 0; i < NAMES.size(); ++i) if (NAMES[i] == n) return (int)i;
  return -1;
}
static void expect_line(const std::string& line, int want, const char* what) {
  verify::Line l;
  int t = -1;
  const int got = coverage::classify_line(line, find_name, LENGTHS, l, &t);
  if (got != want) { fprintf(stderr, "FAIL %s: got %d (%s), want %d\n", what, got, coverage::line_reason(got), want); ++fails; }
  if (got == coverage::LINE_ADD && (t < 0 || NAMES[(size_t)t] != l.tname)) { fprintf(stderr, "FAIL %s: target index %d\n", what, t); ++fails; }
}

int main() {
  using coverage::Interval;
  uint64_t lines = 0;
  expect_text(coverage::coverage_bedgraph({"a", "b", "c"}, {5, 4, 6}, {{0, 0}, {3, 2}, {12, 0}}, &lines),
              "a\t0\t3\t0\na\t3\t5\t2\nb\t0\t4\t2\nc\t0\t3\t2\nc\t3\t6\t0\n", "straddling two boundaries");
  if (lines != 5) { fprintf(stderr, "FAIL: %llu lines\n", (unsigned long long)lines); ++fails; }
  expect_text(coverage::coverage_bedgraph({"a", "none", "zero", "b"}, {5, 7, 0, 3}, {{0, 1}, {4, 0}, {13, 3}}, nullptr),
              "a\t0\t4\t1\na\t4\t5\t0\nnone\t0\t7\t0\nb\t0\t1\t0\nb\t1\t3\t3\n", "untouched and empty sequences");
  expect_text(coverage::coverage_bedgraph({"a", "b"}, {2, 3}, {}, nullptr), "a\t0\t2\t0\nb\t0\t3\t0\n", "no intervals");
  expect_text(coverage::coverage_bedgraph({"a", "b"}, {2, 3}, {{1, 4}}, nullptr), "a\t0\t1\t0\na\t1\t2\t4\nb\t0\t3\t4\n", "first interval behind 0");
  expect_text(coverage::coverage_bedgraph({}, {}, {{0, 0}}, &lines), "", "no sequences");
  expect_text(coverage::coverage_bedgraph({"a"}, {3}, {{0, 1}, {3, 0}, {7, 2}}, nullptr), "a\t0\t3\t1\n", "intervals behind the last sequence");

  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int it = 0; it < 20000; ++it) {
    std::vector<std::string> names;
    std::vector<uint64_t> lengths;
    uint64_t total = 0;
    const int nseq = 1 + (int)(rnd() % 5);
    for (int c = 0; c < nseq; ++c) { names.push_back("s" + std::to_string(c)); lengths.push_back(rnd() % 4 ? rnd() % 40 : 0); total += lengths.back(); }
    std::vector<Interval> iv;
    std::vector<uint32_t> dense(total, 0);
    uint64_t at = rnd() % 3 ? 0 : rnd() % (total + 1);
    uint32_t depth = (uint32_t)(rnd() % 3);
    while (at < total + 2) {
      if (!iv.empty() && iv.back().depth == depth) ++depth;  // (neighbours differ, as the device's do)
      iv.push_back(Interval{at, depth});
      const uint64_t len = 1 + rnd() % 30;
      for (uint64_t p = at; p < at + len && p < total; ++p) dense[p] = depth;
      at += len;
      depth = (uint32_t)(rnd() % 4);
    }
    for (uint64_t p = iv.back().start; p < total; ++p) dense[p] = iv.back().depth;
    std::string want;
    uint64_t g0 = 0, n_want = 0;
    for (int c = 0; c < nseq; ++c) {
      for (uint64_t a = 0; a < lengths[(size_t)c];) {
        uint64_t b = a + 1;
        while (b < lengths[(size_t)c] && dense[g0 + b] == dense[g0 + a]) ++b;
        want += names[(size_t)c] + "\t" + std::to_string(a) + "\t" + std::to_string(b) + "\t" + std::to_string(dense[g0 + a]) + "\n";
        ++n_want;
        a = b;
      }
      g0 += lengths[(size_t)c];
    }
    const std::string got = coverage::coverage_bedgraph(names, lengths, iv, &lines);
    if (got != want || lines != n_want) { expect_text(got, want, "random intervals"); if (fails > 5) break; }
  }

  const std::string head = "q#1#chr1\t5000\t100\t140\t-\tt#1#chr1\t9000\t2000\t2042\t37\t44\t60\tgi:f:0.97\t";
  const std::string good = head + "cg:Z:20=1X5=2I10=4D2=\tmd:f:0.9";
  expect_line(good, coverage::LINE_ADD, "good");
  expect_line(head, coverage::LINE_NO_CIGAR, "no tag");
  expect_line(head + "cg:Z:42M", coverage::LINE_NO_CIGAR, "plain M");
  expect_line(head + "cg:Z:0=", coverage::LINE_MALFORMED, "count 0");
  expect_line(head + "cg:Z:41=", coverage::LINE_MALFORMED, "a base short of te - ts");
  expect_line(head + "cg:Z:43=", coverage::LINE_MALFORMED, "a base past te - ts");
  expect_line(head + "cg:Z:42=7I", coverage::LINE_ADD, "I runs take no target base");
  expect_line("q\t5000\t100\t140\t+\tnobody\t9000\t2000\t2042\t37\t44\t60\tcg:Z:42=", coverage::LINE_UNKNOWN_TARGET, "unknown target");
  expect_line("q\t5000\t100\t140\t+\tt#1#chr1\t9001\t2000\t2042\t37\t44\t60\tcg:Z:42=", coverage::LINE_TLEN, "another tlen");
  expect_line("q\t5000\t100\t140\t+\tt#1#chr2\t500\t458\t500\t37\t44\t60\tcg:Z:42=", coverage::LINE_ADD, "to the last base");
  expect_line("q\t5000\t100\t140\t+\tt#1#chr2\t500\t459\t501\t37\t44\t60\tcg:Z:42=", coverage::LINE_MALFORMED, "past the sequence");
  expect_line("", coverage::LINE_MALFORMED, "empty line");
  expect_line("\t\t\t\t\t\t\t\t\t\t\t\t", coverage::LINE_MALFORMED, "empty fields");
  for (size_t n = 0; n <= good.size(); ++n) {
    verify::Line l;
    (void)coverage::classify_line(good.substr(0, n), find_name, LENGTHS, l, nullptr);
  }
  const char alphabet[] = "0123456789=XIDM\t:-+cgZt#hr \n";
  int added = 0;
  for (int it = 0; it < 200000; ++it) {
    std::string s = good;
    const int edits = (int)(rnd() % 4);
    for (int e = 0; e < edits && !s.empty(); ++e) {
      const size_t at = rnd() % s.size();
      switch (rnd() % 3) {
        case 0: s[at] = alphabet[rnd() % (sizeof(alphabet) - 1)]; break;
        case 1: s.erase(at, 1); break;
        default: s.insert(at, 1, s[at]); break;
      }
    }
    verify::Line l;
    int t = -1;
    const int st = coverage::classify_line(s, find_name, LENGTHS, l, &t);
    if (st < 0 || st > 4) { fprintf(stderr, "FAIL: code %d\n", st); ++fails; }
    if (st != coverage::LINE_ADD) continue;
    ++added;
    uint64_t bases = 0;
    for (uint32_t w : l.runs) if ((w & 3u) != 2u) bases += w >> 2;
    // what the device call relies on: the span lies inside the sequence the line names
    if (t < 0 || (size_t)t >= LENGTHS.size() || l.ts < 0 || bases != (uint64_t)(l.te - l.ts) || (uint64_t)l.te > LENGTHS[(size_t)t]) {
      fprintf(stderr, "FAIL: an added line leaves its sequence: %s\n", s.c_str());
      ++fails;
    }
  }
  if (added < 1000) { fprintf(stderr, "FAIL: only %d mutated lines were added\n", added); ++fails; }
  printf(fails ? "%d failures\n" : "coverage_check ok\n", fails);
  return fails ? 1 : 0;
}
