// The text side of --chain-net (wfmash_amd/host/chain_text.hpp: net_body, net_file) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/chain_net_check.cpp -o /tmp/chain_net_check && /tmp/chain_net_check
// net_body and number on fixed records with known files: one piece, pieces with gaps on both sides, a - record, a target sequence that
// does not begin the concatenation, a record whose first piece lies deep inside its runs, the largest coordinates the fields can hold,
// a record without pieces, and many chains numbered in one pass; net_file on a table of those cases with a record that won nothing, on
// tables that are not the records added, and on more than a MiB of chains.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/chain_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}

static std::string file_of(const std::string& body, uint64_t first = 1) {
  std::string out;
  uint64_t next = first;
  chain::number(body, &next, out);
  return out;
}

int main() {
  chain::Record r;
  r.qname = "q#1#chr1"; r.tname = "t#1#chr1"; r.qsize = 1000; r.tsize = 2000; r.qs = 100; r.qe = 400; r.ts = 500; r.te = 800;
  // the whole record, one piece: what --chain writes for 300=
  const std::vector<chain::Piece> whole = {{0, 500, 0, 300}};
  std::string body;
  chain::net_body(body, r, 0, 300, whole.data(), whole.size());
  expect_text(file_of(body), "chain 300 t#1#chr1 2000 + 500 800 q#1#chr1 1000 + 100 400 1\n300\n\n", "one piece");
  // cut in three: [500, 520), [550, 600), [790, 800); the middle went to others on both sides alike, an insertion lay before the last
  const std::vector<chain::Piece> three = {{0, 500, 0, 20}, {0, 550, 50, 50}, {0, 790, 295, 10}};
  body.clear();
  chain::net_body(body, r, 0, 41, three.data(), three.size());
  expect_text(file_of(body, 9), "chain 41 t#1#chr1 2000 + 500 800 q#1#chr1 1000 + 100 405 9\n20\t30\t30\n50\t190\t195\n10\n\n", "three pieces");
  // the same on -: the query side begins at qsize - qe on the reverse strand
  r.rev = true;
  body.clear();
  chain::net_body(body, r, 0, 41, three.data(), three.size());
  expect_text(file_of(body), "chain 41 t#1#chr1 2000 + 500 800 q#1#chr1 1000 - 600 905 1\n20\t30\t30\n50\t190\t195\n10\n\n", "three pieces on -");
  // a sequence that begins at 7000 in the concatenation, and a first piece deep inside the runs: both starts move
  const std::vector<chain::Piece> deep = {{0, 7000 + 640, 163, 5}};
  body.clear();
  chain::net_body(body, r, 7000, 255, deep.data(), deep.size());
  expect_text(file_of(body), "chain 255 t#1#chr1 2000 + 640 645 q#1#chr1 1000 - 763 768 1\n5\n\n", "deep first piece");
  // the largest coordinates: a target near 2^40, pieces of 2^32 - 1 and a gap of nearly 2^40 between two of them
  chain::Record big;
  big.qname = "q"; big.tname = "t"; big.qsize = (1ull << 62); big.tsize = (1ull << 40) - 1; big.qs = 5; big.qe = 5 + 0xffffffffull;
  const std::vector<chain::Piece> huge = {{0, 0, 0, 1}, {0, (1ull << 40) - 2, 0xfffffffeu, 1}};
  body.clear();
  chain::net_body(body, big, 0, 0xffffffffu, huge.data(), huge.size());
  expect_text(file_of(body), "chain 4294967295 t 1099511627775 + 0 1099511627775 q 4611686018427387904 + 5 4294967300 1\n1\t1099511627773\t4294967293\n1\n\n", "largest coordinates");
  const std::vector<chain::Piece> one = {{0, 0, 0, 0xffffffffu}};
  body.clear();
  chain::net_body(body, big, 0, 7, one.data(), one.size());
  expect_text(file_of(body), "chain 7 t 1099511627775 + 0 4294967295 q 4611686018427387904 + 5 4294967300 1\n4294967295\n\n", "largest piece");
  // no pieces: nothing; many chains: forty headers, ids 1 .. 40
  body.clear();
  chain::net_body(body, r, 0, 1, nullptr, 0);
  expect_text(body, "", "no pieces");
  std::string many;
  for (int k = 0; k < 40; ++k) {
    std::vector<chain::Piece> pieces;
    for (int j = 0; j <= k % 5; ++j) pieces.push_back(chain::Piece{0, 500 + (uint64_t)j * 50, (uint32_t)j * 55, (uint32_t)(k + 1)});
    chain::net_body(many, r, 0, (uint32_t)k, pieces.data(), pieces.size());
  }
  const std::string all = file_of(many);
  size_t headers = 0;
  for (size_t at = 0; at < all.size(); at = all.find('\n', at) + 1) headers += all[at] == 'c';
  if (headers != 40 || all.find(" 40\n") == std::string::npos) { fprintf(stderr, "FAIL forty chains\n"); ++fails; }
  // the whole file (net_file) from a table of the hand cases above: the - record with three pieces, a record that won nothing, the deep
  // piece behind a sequence that begins at 7000; ids in the order of the orders, the chains and the lost counted
  {
    chain::Record fwd = r;
    fwd.rev = false;
    const std::vector<chain::NetHead> heads = {{3, 0, r}, {4, 0, fwd}, {(1ull << 32) | 0, 7000, r}};
    std::vector<chain::Piece> pieces = three;
    pieces.push_back(deep[0]);
    const std::vector<chain::NetCall> per = {{3, 41, 0, 0, 3, 0, 0}, {4, 9, 0, 3, 0, 0, 0}, {(1ull << 32) | 0, 255, 0, 3, 1, 0, 0}};
    std::ostringstream file;
    uint64_t chains = 0, lost = 0;
    const bool same = chain::net_file(file, heads, per.data(), per.size(), pieces.data(), &chains, &lost);
    if (!same || chains != 2 || lost != 1) { fprintf(stderr, "FAIL net_file: %d, %llu chains, %llu lost\n", (int)same, (unsigned long long)chains, (unsigned long long)lost); ++fails; }
    expect_text(file.str(),
                "chain 41 t#1#chr1 2000 + 500 800 q#1#chr1 1000 - 600 905 1\n20\t30\t30\n50\t190\t195\n10\n\n"
                "chain 255 t#1#chr1 2000 + 640 645 q#1#chr1 1000 - 763 768 2\n5\n\n",
                "net_file");
    // a table whose records are not the heads: another order, one record fewer
    std::vector<chain::NetCall> other = per;
    other[1].order = 5;
    std::ostringstream none;
    if (chain::net_file(none, heads, other.data(), other.size(), pieces.data(), &chains, &lost)) { fprintf(stderr, "FAIL net_file took another order\n"); ++fails; }
    if (chain::net_file(none, heads, per.data(), per.size() - 1, pieces.data(), &chains, &lost)) { fprintf(stderr, "FAIL net_file took fewer records\n"); ++fails; }
    // more than a MiB of chains: flushed in parts, numbered through
    std::vector<chain::NetHead> many_heads;
    std::vector<chain::NetCall> many_per;
    for (uint64_t k = 0; k < 40000; ++k) { many_heads.push_back({k, 0, fwd}); many_per.push_back({k, 1, 0, 0, 3, 0, 0}); }
    std::ostringstream big_file;
    chain::net_file(big_file, many_heads, many_per.data(), many_per.size(), pieces.data(), &chains, &lost);
    const std::string big_text = big_file.str();
    const std::string last = "chain 1 t#1#chr1 2000 + 500 800 q#1#chr1 1000 + 100 405 40000\n20\t30\t30\n50\t190\t195\n10\n\n";
    if (chains != 40000 || lost != 0 || big_text.size() < (2u << 20) || big_text.compare(big_text.size() - last.size(), last.size(), last) != 0) {
      fprintf(stderr, "FAIL net_file over a MiB\n");
      ++fails;
    }
  }
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("chain_net_check: ok\n");
  return 0;
}
