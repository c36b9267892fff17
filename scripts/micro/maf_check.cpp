// The text side of --maf (wfmash_amd/host/maf_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan scripts/micro/maf_check.cpp -o /tmp/maf_check && /tmp/maf_check
// (tests/test_maf_cpu.py builds and runs it so; the runtimes are linked in, nothing is preloaded)
// The header; block on fixed records with known paragraphs on both strands, with blocks at offsets inside a larger row buffer, a block
// without a base in one row, the largest coordinates the fields can hold, many blocks appended to one string, and record_bytes against
// what block appends.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/maf_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}

int main() {
  expect_text(maf::header(), "##maf version=1\n", "header");
  const std::string tname = "t#1#chr1", qname = "q#1#chr1";
  // 2= 2I 3D 2= over ACTTGGA x ACCAGA, behind 4 bytes of another block's rows
  const std::string rows = std::string("ACAC") + "AC--TTGGA" + "ACCA---GA";
  const maf::Block b{4, 0, 0, 0, 7, 6, 9, 4, 0};
  maf::Line l{&tname, 500, 2000, &qname, 100, 106, 1000, false};
  std::string out;
  maf::block(out, l, b, rows.data());
  expect_text(out, "a score=4\ns t#1#chr1 500 7 + 2000 AC--TTGGA\ns q#1#chr1 100 6 + 1000 ACCA---GA\n\n", "plain +");
  // the same rows on -: the query start counts from the end of the reverse-complemented source, 1000 - 106
  l.rev = true;
  out.clear();
  maf::block(out, l, b, rows.data());
  expect_text(out, "a score=4\ns t#1#chr1 500 7 + 2000 AC--TTGGA\ns q#1#chr1 894 6 - 1000 ACCA---GA\n\n", "plain -");
  // a later block of the same record: p and t move both starts, on - forward from the same end
  const std::string rows2 = "GAGA";
  const maf::Block b2{0, 0, 5, 4, 2, 2, 2, 2, 0};
  out.clear();
  maf::block(out, l, b2, rows2.data());
  expect_text(out, "a score=2\ns t#1#chr1 505 2 + 2000 GA\ns q#1#chr1 898 2 - 1000 GA\n\n", "second block -");
  l.rev = false;
  out.clear();
  maf::block(out, l, b2, rows2.data());
  expect_text(out, "a score=2\ns t#1#chr1 505 2 + 2000 GA\ns q#1#chr1 104 2 + 1000 GA\n\n", "second block +");
  // a block without a pattern base (the raw call allows it)
  const std::string rows3 = "----ACGN";
  const maf::Block b3{0, 0, 0, 0, 0, 4, 4, 0, 0};
  out.clear();
  maf::block(out, l, b3, rows3.data());
  expect_text(out, "a score=0\ns t#1#chr1 500 0 + 2000 ----\ns q#1#chr1 100 4 + 1000 ACGN\n\n", "no pattern base");
  // the largest coordinates: 64-bit starts and lengths, 32-bit sizes
  const std::string one = "AC";
  const maf::Block big{0, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 1, 0xffffffffu, 0};
  maf::Line far{&tname, 0xfffffffeffffffffull, 0xffffffffffffffffull, &qname, 0xfffffffeffffffffull, 0xfffffffeffffffffull, 0xffffffffffffffffull, false};
  out.clear();
  maf::block(out, far, big, one.data());
  expect_text(out, "a score=4294967295\ns t#1#chr1 18446744073709551614 4294967295 + 18446744073709551615 A\n"
                   "s q#1#chr1 18446744073709551614 4294967295 + 18446744073709551615 C\n\n", "largest coordinates");
  // many blocks behind one another in one string: every paragraph ends with an empty line, nothing is lost between them
  std::string many;
  std::vector<char> wide(2 * 70000, 'A');
  for (int k = 0; k < 70000; ++k) wide[70000 + (size_t)k] = k % 7 ? 'C' : '-';
  const maf::Block wb{0, 0, 0, 0, 70000, 60000, 70000, 0, 60000};
  for (int k = 0; k < 50; ++k) maf::block(many, l, k % 2 ? wb : b2, k % 2 ? wide.data() : rows2.data());
  size_t paragraphs = 0;
  for (size_t at = 0; (at = many.find("\n\n", at)) != std::string::npos; at += 2) ++paragraphs;
  if (paragraphs != 50 || many.size() < 25 * 2 * 70000 || many.compare(many.size() - 2, 2, "\n\n") != 0) { fprintf(stderr, "FAIL many blocks\n"); ++fails; }
  // record_bytes is an upper bound of what block appends, block by block: a record's string reserved once never grows
  {
    const std::vector<maf::Block> bl = {b2, wb, b3};
    const char* rw[3] = {rows2.data(), wide.data(), rows3.data()};
    std::string rec;
    rec.reserve(maf::record_bytes(l, bl.data(), bl.size()));
    const size_t cap = rec.capacity();
    const char* at = rec.data();
    for (size_t k = 0; k < bl.size(); ++k) maf::block(rec, l, bl[k], rw[k]);
    if (rec.capacity() != cap || rec.data() != at || rec.size() > maf::record_bytes(l, bl.data(), bl.size())) { fprintf(stderr, "FAIL record_bytes\n"); ++fails; }
    if (maf::record_bytes(far, &big, 1) < out.size()) { fprintf(stderr, "FAIL record_bytes at the largest coordinates\n"); ++fails; }
  }
  if (fails) return 1;
  printf("maf_check: ok\n");
  return 0;
}
