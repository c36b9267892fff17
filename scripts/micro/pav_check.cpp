// The text side of --pav (wfmash_amd/host/pav_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/pav_check.cpp -o /tmp/pav_check && /tmp/pav_check
// group_key and columns on hand-made names with known answers (no delimiter, the delimiter first, last and twice, bytes above 127, an
// empty name) and on 20000 random lists of names: every name's column holds its key and the keys ascend bytewise without repeats; windows on
// hand-made lengths with a known answer and on random ones: they tile every sequence exactly; header and rows against known bytes, with
// the largest cells and coordinates the fields can hold.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/pav_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}

static bool bytes_less(const std::string& a, const std::string& b) {
  const size_t n = a.size() < b.size() ? a.size() : b.size();
  for (size_t i = 0; i < n; ++i)
    if ((unsigned char)a[i] != (unsigned char)b[i]) return (unsigned char)a[i] < (unsigned char)b[i];
  return a.size() < b.size();
}

static void check_columns(const std::vector<std::string>& names, const char* what) {
  const pav::Columns c = pav::columns(names);
  bool ok = c.of_seq.size() == names.size();
  for (size_t i = 1; ok && i < c.keys.size(); ++i) ok = bytes_less(c.keys[i - 1], c.keys[i]);
  for (size_t i = 0; ok && i < names.size(); ++i) ok = c.of_seq[i] < c.keys.size() && c.keys[c.of_seq[i]] == pav::group_key(names[i]);
  if (!ok) { fprintf(stderr, "FAIL %s: columns\n", what); ++fails; }
}

static void check_windows(const std::vector<uint64_t>& lengths, uint64_t size, const char* what) {
  std::vector<uint64_t> off(1, 0);
  for (uint64_t l : lengths) off.push_back(off.back() + l);
  const std::vector<lift::Interval> w = pav::windows(lengths, off, size);
  std::vector<uint64_t> at(lengths.size(), 0);
  bool ok = true;
  int last = -1;
  for (size_t j = 0; ok && j < w.size(); ++j) {
    const lift::Interval& v = w[j];
    ok = v.seq >= last && (size_t)v.seq < lengths.size() && v.start == at[(size_t)v.seq] && v.start < v.end && v.end - v.start <= size &&
         v.end <= lengths[(size_t)v.seq] && (v.end - v.start == size || v.end == lengths[(size_t)v.seq]) && v.name == "." && v.order == j &&
         v.gstart == off[(size_t)v.seq] + v.start && v.gend == off[(size_t)v.seq] + v.end;
    if (ok) { at[(size_t)v.seq] = v.end; last = v.seq; }
  }
  for (size_t c = 0; ok && c < lengths.size(); ++c) ok = at[c] == lengths[c];
  if (!ok) { fprintf(stderr, "FAIL %s: windows of %llu\n", what, (unsigned long long)size); ++fails; }
}

int main() {
  struct { const char* name; const char* key; } keys[] = {{"chr1", "chr1"}, {"sample#", "sample"}, {"a#1#chr", "a#1"}, {"#x", ""}, {"", ""}, {"##", "#"}, {"a#", "a"}};
  for (const auto& k : keys)
    if (pav::group_key(k.name) != k.key) { fprintf(stderr, "FAIL group_key(%s)\n", k.name); ++fails; }
  if (pav::group_key("a#1#chr", '\0') != "a#1#chr" || pav::group_key("a.1.chr", '.') != "a.1") { fprintf(stderr, "FAIL group_key: other delimiters\n"); ++fails; }

  const std::vector<std::string> names = {"b#1#x", "a#2#y", "b#1#z", "Z#1#c", "solo", "a#10#y", "a#2#q", "\xc3\xa9#1#c", ""};
  const pav::Columns cols = pav::columns(names);
  std::string listed;
  for (const std::string& k : cols.keys) listed += "[" + k + "]";
  expect_text(listed + "\n", "[][Z#1][a#10][a#2][b#1][solo][\xc3\xa9#1]\n", "columns");
  const uint32_t want_col[] = {4, 3, 4, 1, 5, 2, 3, 6, 0};
  for (size_t i = 0; i < names.size(); ++i)
    if (cols.of_seq[i] != want_col[i]) { fprintf(stderr, "FAIL column of %s\n", names[i].c_str()); ++fails; }
  check_columns(names, "hand names");
  check_columns({}, "no names");
  if (!pav::columns({}).keys.empty()) { fprintf(stderr, "FAIL: no names, yet columns\n"); ++fails; }

  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const char alphabet[] = "##ab1\xff\x80 \t";
  for (int it = 0; it < 20000; ++it) {
    std::vector<std::string> some((size_t)(rnd() % 12));
    for (std::string& n : some)
      for (int k = (int)(rnd() % 7); k > 0; --k) n += alphabet[rnd() % (sizeof alphabet - 1)];
    check_columns(some, "random names");
  }

  // windows: a short last one, an exact multiple, a sequence of length 0, one of length 1, a window longer than everything
  const std::vector<uint64_t> lengths = {2500, 0, 1000, 1};
  const std::vector<uint64_t> offsets = {0, 2500, 2500, 3500, 3501};
  std::string listed_w;
  char num[100];
  for (const lift::Interval& v : pav::windows(lengths, offsets, 1000)) {
    snprintf(num, sizeof num, "%d:%llu-%llu@%llu-%llu ", v.seq, (unsigned long long)v.start, (unsigned long long)v.end, (unsigned long long)v.gstart, (unsigned long long)v.gend);
    listed_w += num;
  }
  expect_text(listed_w + "\n", "0:0-1000@0-1000 0:1000-2000@1000-2000 0:2000-2500@2000-2500 2:0-1000@2500-3500 3:0-1@3500-3501 \n", "windows");
  if (!pav::windows(lengths, offsets, 0).empty() || !pav::windows({}, {0}, 5).empty()) { fprintf(stderr, "FAIL: windows of nothing\n"); ++fails; }
  for (uint64_t size : {1ull, 2ull, 999ull, 1000ull, 2500ull, 2501ull, ~0ull}) check_windows(lengths, size, "hand lengths");
  for (int it = 0; it < 20000; ++it) {
    std::vector<uint64_t> some((size_t)(rnd() % 6));
    for (uint64_t& l : some) l = rnd() % 3 == 0 ? 0 : rnd() % 5000;
    check_windows(some, 1 + rnd() % 1200, "random lengths");
  }
  // (near the top of the coordinates: a - b and a + size must not wrap)
  check_windows({(1ull << 40) - 1}, (1ull << 40) - 2, "a long sequence");
  check_windows({~0ull >> 1}, ~0ull, "the longest window");

  // the header and the rows
  expect_text(pav::header({}), "#tname\ttstart\ttend\tname\tlen\n", "header without groups");
  expect_text(pav::header({"a#1", "b#1"}), "#tname\ttstart\ttend\tname\tlen\ta#1\tb#1\n", "header");
  lift::Interval v;
  v.seq = 0; v.start = 10; v.end = 25; v.name = "gene";
  const uint32_t cells[3] = {0u, 15u, 0xffffffffu};
  std::string out;
  pav::row(out, "t#1#chr1", v, cells, 3);
  pav::row(out, "t#1#chr1", v, cells, 0);
  v.start = 0; v.end = ~0ull; v.name = std::string(500, 'n');
  pav::row(out, std::string(300, 't'), v, cells, 3);
  expect_text(out, "t#1#chr1\t10\t25\tgene\t15\t0\t15\t4294967295\nt#1#chr1\t10\t25\tgene\t15\n" + std::string(300, 't') + "\t0\t18446744073709551615\t" + std::string(500, 'n') +
                       "\t18446744073709551615\t0\t15\t4294967295\n",
              "rows");
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("pav_check ok\n");
  return 0;
}
