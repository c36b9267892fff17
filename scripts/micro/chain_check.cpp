// The text side of --chain (wfmash_amd/host/chain_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/chain_check.cpp -o /tmp/chain_check && /tmp/chain_check
// flags_of on the four cases; chain_body and number on fixed records with known files, on both strands, plain and swapped, with and
// without bases before the first and behind the last block, at the largest coordinates the fields can hold, and a record without blocks;
// number on every prefix of a file of many chains and on empty text.
#include <cstdio>
#include <cstdlib>
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
  if (chain::flags_of(false, false) != 0u || chain::flags_of(false, true) != 0u || chain::flags_of(true, false) != 1u || chain::flags_of(true, true) != 3u) {
    fprintf(stderr, "FAIL flags_of\n");
    ++fails;
  }
  chain::Record r;
  r.qname = "q#1#chr1"; r.tname = "t#1#chr1"; r.qsize = 1000; r.tsize = 2000; r.qs = 100; r.qe = 112; r.ts = 500; r.te = 513;
  // 4= 3D 2I 6=: the plain blocks, and what the device gives with SWAP and with SWAP | REVERSE
  const std::vector<chain::Block> plain = {{4, 3, 2, 4}, {6, 0, 0, 6}}, swapped = {{4, 2, 3, 4}, {6, 0, 0, 6}}, both = {{6, 2, 3, 6}, {4, 0, 0, 4}};
  chain::Ends e;
  e.eq = 10;
  std::string body;
  chain::chain_body(body, r, false, e, plain.data(), plain.size());
  expect_text(file_of(body), "chain 10 t#1#chr1 2000 + 500 513 q#1#chr1 1000 + 100 112 1\n4\t3\t2\n6\n\n", "plain +");
  body.clear();
  chain::chain_body(body, r, true, e, swapped.data(), swapped.size());
  expect_text(file_of(body, 7), "chain 10 q#1#chr1 1000 + 100 112 t#1#chr1 2000 + 500 513 7\n4\t2\t3\n6\n\n", "swapped +");
  r.rev = true;
  body.clear();
  chain::chain_body(body, r, false, e, plain.data(), plain.size());
  expect_text(file_of(body), "chain 10 t#1#chr1 2000 + 500 513 q#1#chr1 1000 - 888 900 1\n4\t3\t2\n6\n\n", "plain -");
  body.clear();
  chain::chain_body(body, r, true, e, both.data(), both.size());
  expect_text(file_of(body), "chain 10 q#1#chr1 1000 + 100 112 t#1#chr1 2000 - 1487 1500 1\n6\t2\t3\n4\n\n", "swapped -");
  // bases before the first and behind the last block: 1I 2D | 5= | 3I, on -
  chain::Record g = r;
  g.qs = 10; g.qe = 19; g.ts = 40; g.te = 47;
  const std::vector<chain::Block> one = {{5, 0, 0, 5}};
  chain::Ends lead;
  lead.eq = 5; lead.lead_dt = 2; lead.lead_dq = 1; lead.trail_dt = 0; lead.trail_dq = 3;
  body.clear();
  chain::chain_body(body, g, false, lead, one.data(), one.size());
  expect_text(file_of(body), "chain 5 t#1#chr1 2000 + 42 47 q#1#chr1 1000 - 982 987 1\n5\n\n", "ends moved, plain -");
  chain::Ends back;  // the same problem with SWAP | REVERSE
  back.eq = 5; back.lead_dt = 3; back.lead_dq = 0; back.trail_dt = 1; back.trail_dq = 2;
  body.clear();
  chain::chain_body(body, g, true, back, one.data(), one.size());
  expect_text(file_of(body), "chain 5 q#1#chr1 1000 + 13 18 t#1#chr1 2000 - 1953 1958 1\n5\n\n", "ends moved, swapped -");
  // the largest coordinates: sizes near 2^62, blocks of 2^32 - 1
  chain::Record big;
  big.qname = "q"; big.tname = "t"; big.rev = true;
  big.qsize = (1ull << 62); big.tsize = (1ull << 62) + 5;
  big.qs = 0; big.qe = 0xffffffffull; big.ts = (1ull << 62) + 5 - 0xffffffffull; big.te = (1ull << 62) + 5;
  const std::vector<chain::Block> huge = {{0xffffffffu, 0, 0, 0xffffffffu}};
  chain::Ends he;
  he.eq = 0xffffffffu;
  body.clear();
  chain::chain_body(body, big, false, he, huge.data(), huge.size());
  expect_text(file_of(body), "chain 4294967295 t 4611686018427387909 + 4611686014132420614 4611686018427387909 q 4611686018427387904 - 4611686014132420609 4611686018427387904 1\n4294967295\n\n", "largest coordinates");
  // no blocks: nothing; many chains: ids ascend over every prefix of the text and nothing else changes
  body.clear();
  chain::chain_body(body, r, false, e, nullptr, 0);
  expect_text(body, "", "no blocks");
  expect_text(file_of(""), "", "empty text");
  std::string many;
  for (int k = 0; k < 40; ++k) {
    std::vector<chain::Block> blocks((size_t)(1 + k % 5), chain::Block{(uint32_t)(k + 1), (uint32_t)k, (uint32_t)(k % 3), 1u});
    chain::chain_body(many, r, (k & 1) != 0, e, blocks.data(), blocks.size());
  }
  for (size_t cut = 0; cut <= many.size(); ++cut) {
    std::string out;
    uint64_t next = 5;
    const uint64_t n = chain::number(many.substr(0, cut), &next, out);
    if (next != 5 + n || out.size() < cut) { fprintf(stderr, "FAIL number on the prefix of %zu bytes\n", cut); ++fails; break; }
  }
  const std::string all = file_of(many);
  size_t headers = 0;
  for (size_t at = 0; at < all.size(); at = all.find('\n', at) + 1) headers += all[at] == 'c';
  if (headers != 40 || all.find(" 40\n") == std::string::npos) { fprintf(stderr, "FAIL forty chains\n"); ++fails; }
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("chain_check: ok\n");
  return 0;
}
