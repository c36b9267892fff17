// The host-only parts of the ANI table on their own, for a sanitizer build: the table's rows and text (wfmash_amd/host/ani_rows.hpp)
// and what wfm_sketch_intersections decides before anything touches the device (wfmash_amd/csrc/map_isect_args.h: the checks of
// its CSR arguments, the cut of the matrix into launches).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/ani_rows_check.cpp wfmash_amd/host/map_stats.cpp \
//       -o /tmp/ani_rows_check && /tmp/ani_rows_check
// Random inputs.  The argument arrays are allocated at their exact sizes, so a check that reads one entry too many is caught by the
// sanitizer; a CSR made good must pass, and each single defect planted in it (offsets[0], a decreasing offset, an index out of
// range on either axis, at the first, the last or a random place) must be refused with a message that names it.  The cut must
// tile the matrix exactly with launches of at most max_cells cells.  Every row's text must parse back to its numbers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../wfmash_amd/csrc/map_isect_args.h"
#include "../../wfmash_amd/host/ani_rows.hpp"

static int fails = 0;
static uint64_t x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
static int64_t pick(int64_t n) { return n <= 0 ? 0 : (int64_t)(rnd() % (uint64_t)(n + 1)); }
static void fail(const char* what, int it) { if (++fails < 10) fprintf(stderr, "FAIL (%d): %s\n", it, what); }

static void check_args(int it) {
  const int64_t n = pick(40), nr = pick(30), nc = pick(30);
  std::unique_ptr<int64_t[]> off(new int64_t[(size_t)n + 1]);
  std::unique_ptr<int32_t[]> rows(new int32_t[(size_t)nr]), cols(new int32_t[(size_t)nc]);
  off[0] = 0;
  for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + (rnd() % 4 == 0 ? 0 : pick(it % 50 == 0 ? (int64_t)1 << 31 : 5000));
  for (int64_t i = 0; i < nr; ++i) rows[(size_t)i] = (int32_t)pick(n - 1);
  for (int64_t i = 0; i < nc; ++i) cols[(size_t)i] = (int32_t)pick(n - 1);
  using wfm::isect_check_args;
  const bool indexable = n > 0 || (nr == 0 && nc == 0);
  const std::string good = isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc);
  if (indexable ? !good.empty() : good.empty()) fail("a good CSR refused, or indices into no sketches accepted", it);
  if (!indexable) return;
  {  // offsets[0]
    off[0] = 1 + pick(5);
    if (isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc).find("offsets[0]") == std::string::npos) fail("offsets[0] != 0 accepted", it);
    off[0] = 0;
  }
  if (n > 0) {  // a decreasing offset, at the first, the last or a random place
    const int64_t at = 1 + (it % 3 == 0 ? 0 : it % 3 == 1 ? n - 1 : pick(n - 1));
    const int64_t keep = off[(size_t)at];
    off[(size_t)at] = off[(size_t)at - 1] - 1 - pick(3);
    const std::string m = isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc);
    if (m.find("decrease") == std::string::npos) fail("a decreasing offset accepted", it);
    off[(size_t)at] = off[(size_t)at - 1] + ((int64_t)1 << 32);  // a sketch whose count does not fit 32 bits
    if (isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc).find("2^32") == std::string::npos) fail("a sketch of 2^32 hashes accepted", it);
    off[(size_t)at] = keep;
  }
  for (int axis = 0; axis < 2; ++axis) {  // an index out of range
    int32_t* v = axis ? cols.get() : rows.get();
    const int64_t cnt = axis ? nc : nr;
    if (cnt == 0) continue;
    const int64_t at = it % 3 == 0 ? 0 : it % 3 == 1 ? cnt - 1 : pick(cnt - 1);
    const int32_t keep = v[(size_t)at];
    v[(size_t)at] = rnd() % 2 ? (int32_t)n : rnd() % 2 ? -1 : (int32_t)(n + pick(1000));
    const std::string m = isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc);
    if (m.find(axis ? "cols[" : "rows[") == std::string::npos) fail("an index out of range accepted", it);
    v[(size_t)at] = keep;
  }
  if (isect_check_args(nullptr, n, rows.get(), nr, cols.get(), nc).empty()) fail("NULL offsets accepted", it);
  if (isect_check_args(off.get(), -1, rows.get(), nr, cols.get(), nc).empty()) fail("a negative count accepted", it);
  if (!isect_check_args(off.get(), n, rows.get(), nr, cols.get(), nc).empty()) fail("the restored CSR refused", it);
}

static void check_cut(int it) {
  const int64_t nr = 1 + pick(it % 5 == 0 ? (int64_t)1 << 40 : 300), nc = 1 + pick(it % 7 == 0 ? (int64_t)1 << 40 : 300);
  const int64_t cells = it % 3 == 0 ? (int64_t)64 << 20 : 1 + pick(5000);
  const wfm::IsectCut c = wfm::isect_cut(nr, nc, cells);
  bool ok = c.rows >= 1 && c.cols >= 1 && c.rows <= nr && c.cols <= nc;
  ok = ok && (__int128)c.rows * c.cols <= cells;
  ok = ok && (c.cols == nc || c.rows == 1);                                   // whole rows, or one row in pieces
  ok = ok && (c.rows == nr || (__int128)(c.rows + 1) * c.cols > cells);       // as many rows as fit
  if (!ok) fail("the cut does not tile the matrix within the bound", it);
  const wfm::IsectCut z = wfm::isect_cut(0, nc, cells), w = wfm::isect_cut(nr, 0, cells);
  if (z.rows != 0 || w.cols != 0 || w.rows != 0) fail("an empty matrix got a launch", it);
}

static void check_rows(int it) {
  using namespace skch::Stat;
  std::vector<AniRow> rows;
  const int n = (int)pick(6);
  for (int i = 0; i < n; ++i) {
    const uint64_t qn = (uint64_t)pick(it % 4 == 0 ? 5 : 20000), tn = (uint64_t)pick(it % 4 == 1 ? 5 : 20000);
    const uint64_t smaller = qn < tn ? qn : tn;
    const uint64_t shared = rnd() % 3 == 0 ? 0 : rnd() % 3 == 0 ? smaller : (uint64_t)pick((int64_t)smaller);
    std::string a(1 + (size_t)pick(12), 'g'), b(1 + (size_t)pick(300), '#');   // long names must not be cut
    a[a.size() / 2] = '#';
    rows.push_back(ani_row(a, b, qn, tn, shared));
    const AniRow& r = rows.back();
    bool ok = r.jaccard >= 0 && r.jaccard <= 1 && r.ani >= 0 && r.ani <= 1;
    ok = ok && ((shared == 0 || smaller == 0) ? (r.jaccard == 0 && r.ani == 0) : (r.ani > 0));
    ok = ok && (shared != smaller || smaller == 0 || r.ani == 1.0);
    if (!ok) fail("a row's numbers leave their range", it);
  }
  const std::string text = ani_tsv(rows);
  size_t pos = text.find('\n');
  if (pos == std::string::npos || text.compare(0, pos + 1, ani_tsv_header()) != 0) { fail("no header line", it); return; }
  for (const AniRow& r : rows) {
    const size_t end = text.find('\n', pos + 1);
    if (end == std::string::npos) { fail("a row is missing", it); return; }
    const std::string line = text.substr(pos + 1, end - pos - 1);
    pos = end;
    const std::string names = r.query_group + "\t" + r.target_group + "\t";
    unsigned long long qn = 0, tn = 0, sh = 0; double j = -1, a = -1;
    if (line.compare(0, names.size(), names) != 0 || sscanf(line.c_str() + names.size(), "%llu\t%llu\t%llu\t%lf\t%lf", &qn, &tn, &sh, &j, &a) != 5 ||
        qn != r.query_hashes || tn != r.target_hashes || sh != r.shared || j < r.jaccard - 1e-6 || j > r.jaccard + 1e-6 || a < r.ani - 1e-6 || a > r.ani + 1e-6)
      fail("a row's text does not parse back to its numbers", it);
  }
  if (pos + 1 != text.size()) fail("text after the last row", it);
}

int main() {
  for (int it = 0; it < 200000; ++it) { check_args(it); check_cut(it); }
  for (int it = 0; it < 20000; ++it) check_rows(it);
  printf(fails ? "%d failures\n" : "ani_rows_check ok\n", fails);
  return fails ? 1 : 0;
}
