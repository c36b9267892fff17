// The text side of --lift (wfmash_amd/host/lift_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/lift_check.cpp -o /tmp/lift_check && /tmp/lift_check
// parse_bed on a hand-made file with every kind of skipped line and a known answer (sorting, duplicates, the missing name column), on
// every prefix of it and on 200000 random mutations of it: whatever is kept lies inside its sequence and the list is sorted; the strand
// arithmetic and lift_line on fixed lifts with known lines, on both strands, and at the largest coordinates the fields can hold.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/lift_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}

static const std::vector<std::string> NAMES = {"t#1#chr1", "t#1#chr2", "track1"};
static const std::vector<uint64_t> LENGTHS = {1000, 400, 50};
static const std::vector<uint64_t> OFFSETS = {0, 1000, 1400, 1450};
static int find_name(const std::string& n) {
  for (size_t i = 0; i < NAMES.size(); ++i) if (NAMES[i] == n) return (int)i;
  return -1;
}

// what must hold of anything the parser keeps
static void check_bed(const lift::Bed& bed, const char* what) {
  for (size_t i = 0; i < bed.iv.size(); ++i) {
    const lift::Interval& v = bed.iv[i];
    bool ok = v.seq >= 0 && (size_t)v.seq < LENGTHS.size() && v.start < v.end && v.end <= LENGTHS[(size_t)v.seq] && !v.name.empty() &&
              v.gstart == OFFSETS[(size_t)v.seq] + v.start && v.gend == OFFSETS[(size_t)v.seq] + v.end && v.order < bed.iv.size();
    if (i) {
      const lift::Interval& u = bed.iv[i - 1];
      ok = ok && (u.gstart < v.gstart || (u.gstart == v.gstart && (u.gend < v.gend || (u.gend == v.gend && u.order < v.order))));
    }
    if (!ok) { fprintf(stderr, "FAIL %s: interval %zu\n", what, i); ++fails; return; }
  }
}

int main() {
  const std::string bed_text =
      "# a comment\ntrack name=genes\nbrowser position chr1:1-100\n\n \t \n"
      "t#1#chr2\t10\t50\tgeneB\t0\t+\n"
      "t#1#chr1\t100\t200\tgeneA\n"
      "t#1#chr1\t100\t200\tgeneA.dup\n"
      "t#1#chr1\t0\t1000\n"
      "t#1#chr1\t150\t160\t\n"
      "t#1#chr9\t1\t2\tunknown\n"
      "t#1#chr1\t7\t7\tempty\n"
      "t#1#chr1\t9\t7\tbackwards\n"
      "t#1#chr2\t390\t401\tbeyond\n"
      "t#1#chr2\t390\t400\tto_the_end\r\n"
      "t#1#chr1\t1\t2x\tjunk\n"
      "t#1#chr1\t-1\t2\tjunk\n"
      "t#1#chr1\t1\n"
      "t#1#chr1 5 9 spaces\n"
      "track1\t0\t50\tnamed like a track line\n"
      "t#1#chr1\t5\t1234567890123456789\ttoo_long\n";
  const lift::Bed bed = lift::parse_bed(bed_text, find_name, LENGTHS, OFFSETS);
  check_bed(bed, "hand file");
  expect_text(lift::bed_dump(bed),
              "#skipped\t14\n"
              "#iv\t0\t0\t1000\t.\t3\t0\t1000\n"
              "#iv\t0\t100\t200\tgeneA\t1\t100\t200\n"
              "#iv\t0\t100\t200\tgeneA.dup\t2\t100\t200\n"
              "#iv\t0\t150\t160\t.\t4\t150\t160\n"
              "#iv\t1\t10\t50\tgeneB\t0\t1010\t1050\n"
              "#iv\t1\t390\t400\tto_the_end\t5\t1390\t1400\n"
              "#iv\t2\t0\t50\tnamed like a track line\t6\t1400\t1450\n",
              "hand file");
  expect_text(lift::bed_dump(lift::parse_bed("", find_name, LENGTHS, OFFSETS)), "#skipped\t0\n", "empty file");
  expect_text(lift::bed_dump(lift::parse_bed("\n", find_name, LENGTHS, OFFSETS)), "#skipped\t1\n", "one blank line");
  expect_text(lift::bed_dump(lift::parse_bed("t#1#chr1\t1\t2", find_name, LENGTHS, OFFSETS)), "#skipped\t0\n#iv\t0\t1\t2\t.\t0\t1\t2\n", "no newline at the end");
  // every prefix, then random mutations: the parser reads nothing beyond the text and keeps only what holds
  for (size_t n = 0; n <= bed_text.size(); ++n) check_bed(lift::parse_bed(bed_text.substr(0, n), find_name, LENGTHS, OFFSETS), "prefix");
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const char alphabet[] = "\t\n\r 0123456789#-tchr1x";
  for (int it = 0; it < 200000; ++it) {
    std::string t = bed_text.substr((size_t)(rnd() % 200), (size_t)(rnd() % 300));
    for (int k = (int)(rnd() % 4); k > 0 && !t.empty(); --k) {
      const size_t at = (size_t)(rnd() % t.size());
      switch (rnd() % 3) {
        case 0: t[at] = alphabet[rnd() % (sizeof alphabet - 1)]; break;
        case 1: t.erase(at, 1); break;
        default: t.insert(at, 1, alphabet[rnd() % (sizeof alphabet - 1)]); break;
      }
    }
    check_bed(lift::parse_bed(t, find_name, LENGTHS, OFFSETS), "mutation");
  }
  // the strand arithmetic and the lines
  lift::Record fwd, rev;
  fwd.qname = "q#1#a"; fwd.tname = "t#1#chr1"; fwd.qs = 1000; fwd.qe = 1300; fwd.ts = 90; fwd.rev = false;
  rev = fwd; rev.qname = "q#1#b"; rev.qs = 500; rev.qe = 800; rev.rev = true;
  std::string out;
  lift::lift_line(out, fwd, bed.iv[1], 10, 110, 12, 115, 95, 3);
  lift::lift_line(out, rev, bed.iv[1], 10, 110, 12, 115, 95, 3);
  lift::lift_line(out, fwd, bed.iv[3], 60, 60, 70, 70, 0, 0);
  lift::lift_line(out, rev, bed.iv[3], 60, 60, 70, 70, 0, 0);
  expect_text(out,
              "q#1#a\t1012\t1115\tgeneA\t+\tt#1#chr1\t100\t200\t100\t200\t95\t3\t5\t2\n"
              "q#1#b\t685\t788\tgeneA\t-\tt#1#chr1\t100\t200\t100\t200\t95\t3\t5\t2\n"
              "q#1#a\t1070\t1070\t.\t+\tt#1#chr1\t150\t150\t150\t160\t0\t0\t0\t0\n"
              "q#1#b\t730\t730\t.\t-\tt#1#chr1\t150\t150\t150\t160\t0\t0\t0\t0\n",
              "lines");
  // the largest fields: 32-bit offsets on 64-bit coordinates, a long name
  lift::Record big;
  big.qname = std::string(300, 'q'); big.tname = std::string(300, 't'); big.qs = 1ull << 40; big.qe = (1ull << 40) + 0xffffffffull; big.ts = 1ull << 41;
  lift::Interval wide = bed.iv[0];
  wide.name = std::string(500, 'n'); wide.start = 0; wide.end = 999999999999999999ull;
  for (int strand = 0; strand < 2; ++strand) {
    big.rev = strand == 1;
    out.clear();
    lift::lift_line(out, big, wide, 0u, 0xffffffffu, 0u, 0xffffffffu, 0xfffffff0u, 0xfu);
    uint64_t a, b;
    lift::query_range(big, 0u, 0xffffffffu, &a, &b);
    if (a != big.qs || b != big.qe || out.size() < 1100 || out.back() != '\n') { fprintf(stderr, "FAIL: the largest fields\n"); ++fails; }
  }
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("lift_check ok\n");
  return 0;
}
