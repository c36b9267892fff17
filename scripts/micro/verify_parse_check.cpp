// The PAF line parser of the verifier (wfmash_amd/host/verify_parse.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/verify_parse_check.cpp -o /tmp/verify_parse_check && /tmp/verify_parse_check
// A handful of fixed lines with known answers, then every prefix of a good line and 200000 random mutations of it (bytes replaced,
// removed and doubled, tabs among them): the parser must answer one of its three codes and, where it says LINE_OK, its runs must
// spell the CIGAR back.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../wfmash_amd/host/verify_parse.hpp"

static int fails = 0;
static void expect(const std::string& line, int want, const char* what) {
  verify::Line l;
  std::string why;
  const int got = verify::parse_line(line, l, &why);
  if (got != want) { fprintf(stderr, "FAIL %s: got %d (%s), want %d\n", what, got, why.c_str(), want); ++fails; }
}

int main() {
  const std::string head = "q#1#chr1\t5000\t100\t140\t-\tt#1#chr2\t9000\t2000\t2042\t37\t44\t60\tgi:f:0.97\t";
  const std::string good = head + "cg:Z:20=1X5=2I10=4D2=\tmd:f:0.9";
  expect(good, verify::LINE_OK, "good");
  expect(head, verify::LINE_UNVERIFIABLE, "no tag");
  expect(head + "cg:Z:40M", verify::LINE_UNVERIFIABLE, "plain M");
  expect(head + "cg:Z:0=", verify::LINE_MALFORMED, "count 0");
  expect(head + "cg:Z:1073741824=", verify::LINE_MALFORMED, "count 2^30");
  expect(head + "cg:Z:1073741823=", verify::LINE_OK, "count 2^30 - 1");
  expect(head + "cg:Z:99999999999999999999999999=", verify::LINE_MALFORMED, "count of 26 digits");
  expect(head + "cg:Z:", verify::LINE_OK, "empty CIGAR");
  expect("", verify::LINE_MALFORMED, "empty line");
  expect("\t\t\t\t\t\t\t\t\t\t\t\t", verify::LINE_MALFORMED, "empty fields");
  for (size_t n = 0; n <= good.size(); ++n) {
    verify::Line l;
    (void)verify::parse_line(good.substr(0, n), l, nullptr);
  }
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const char alphabet[] = "0123456789=XIDM\t:-+cgZ \n";
  for (int it = 0; it < 200000; ++it) {
    std::string s = good;
    const int edits = 1 + (int)(rnd() % 4);
    for (int e = 0; e < edits && !s.empty(); ++e) {
      const size_t at = rnd() % s.size();
      switch (rnd() % 3) {
        case 0: s[at] = alphabet[rnd() % (sizeof(alphabet) - 1)]; break;
        case 1: s.erase(at, 1); break;
        default: s.insert(at, 1, s[at]); break;
      }
    }
    verify::Line l;
    std::string why;
    const int st = verify::parse_line(s, l, &why);
    if (st < 0 || st > 2) { fprintf(stderr, "FAIL: code %d\n", st); ++fails; }
    if (st == verify::LINE_OK) {
      std::string back;
      for (uint32_t w : l.runs) { back += std::to_string(w >> 2); back += "=XID"[w & 3]; }
      // (the line's own CIGAR with the leading zeros of its counts taken off)
      std::string canon;
      for (size_t i = 0; i < s.size();) {
        if (s[i] < '0' || s[i] > '9') { canon += s[i++]; continue; }
        size_t j = i;
        while (j < s.size() && s[j] >= '0' && s[j] <= '9') ++j;
        while (i + 1 < j && s[i] == '0') ++i;
        canon.append(s, i, j - i);
        i = j;
      }
      if (canon.find("cg:Z:" + back) == std::string::npos) { fprintf(stderr, "FAIL: runs %s not in %s\n", back.c_str(), s.c_str()); ++fails; }
    }
  }
  printf(fails ? "%d failures\n" : "verify_parse_check ok\n", fails);
  return fails ? 1 : 0;
}
