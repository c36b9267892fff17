// The text side of --transitive (wfmash_amd/host/transitive_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/transitive_check.cpp -o /tmp/transitive_check && /tmp/transitive_check
// The world of a target and a query that share names and hold a sequence without bases; parse_seeds on a hand-made BED with every kind of
// skipped line and a known answer, on every prefix of it and on 100000 random mutations of it (whatever is kept lies inside its sequence
// and the list is in input order); lines() on intervals with known lines, across one, two and all sequence boundaries, at a sequence
// without bases and at the world's end, and on random intervals (the pieces abut, stay inside their sequences and add up to the interval);
// file() on the same intervals shared out over the seeds, without a closure (every seed reaches itself) and on more than a MiB of lines;
// the strand arithmetic of a record's place in the world.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/transitive_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}
static void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "FAIL %s\n", what); ++fails; }
}

static void check_seeds(const transitive::World& w, const lift::Bed& bed, const char* what) {
  for (size_t i = 0; i < bed.iv.size(); ++i) {
    const lift::Interval& v = bed.iv[i];
    const bool ok = v.seq >= 0 && (size_t)v.seq < w.lengths.size() && v.start < v.end && v.end <= w.lengths[(size_t)v.seq] && !v.name.empty() &&
                    v.gstart == w.offsets[(size_t)v.seq] + v.start && v.gend == w.offsets[(size_t)v.seq] + v.end && v.order == i && v.gend <= w.n_bases();
    if (!ok) { fprintf(stderr, "FAIL %s: seed %zu\n", what, i); ++fails; return; }
  }
}

int main() {
  const transitive::World w = transitive::make_world({"chrA", "chrB", "empty", "chrC"}, {100, 50, 0, 70}, {"chrB", "hapX", "chrA", "hapY"}, {50, 30, 100, 40});
  expect(w.names == std::vector<std::string>({"chrA", "chrB", "empty", "chrC", "hapX", "hapY"}), "the world's names");
  expect(w.offsets == std::vector<uint64_t>({0, 100, 150, 150, 220, 250, 290}) && w.n_bases() == 290, "the world's offsets");
  expect(w.find("hapX") == 4 && w.find("chrB") == 1 && w.find("nobody") == -1, "find");
  expect(w.seq_of(0) == 0 && w.seq_of(99) == 0 && w.seq_of(100) == 1 && w.seq_of(149) == 1 && w.seq_of(150) == 3 && w.seq_of(289) == 5, "seq_of");

  const std::string bed =
      "# a comment\nchrA\t10\t20\tgene1\nhapY\t0\t40\n\ntrack name=x\nbrowser position\nchrA\t5\nchrA\t5\tx\nchrQ\t1\t2\nchrB\t7\t7\nchrB\t40\t51\n"
      "hapX\t29\t30\tlast\textra\r\nchrA\t10\t20\tgene1\nchrA 1 2\n";
  const lift::Bed seeds = transitive::parse_seeds(bed, w);
  expect_text(lift::bed_dump(seeds),
              "#skipped\t10\n#iv\t0\t10\t20\tgene1\t0\t10\t20\n#iv\t5\t0\t40\t.\t1\t250\t290\n#iv\t4\t29\t30\tlast\t2\t249\t250\n#iv\t0\t10\t20\tgene1\t3\t10\t20\n",
              "the seeds in input order");
  for (size_t n = 0; n <= bed.size(); ++n) check_seeds(w, transitive::parse_seeds(bed.substr(0, n), w), "a prefix of the BED");
  unsigned long long rng = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  const char alphabet[] = "\t\n\r 0123456789#chrABXYhap";
  for (int it = 0; it < 100000; ++it) {
    std::string m = bed;
    for (int k = 0, e = 1 + (int)(next() % 4); k < e; ++k) {
      const size_t at = (size_t)(next() % m.size());
      switch (next() % 3) {
        case 0: m[at] = alphabet[next() % (sizeof alphabet - 1)]; break;
        case 1: m.erase(at, 1 + (size_t)(next() % 3)); break;
        default: m.insert(at, 1, alphabet[next() % (sizeof alphabet - 1)]); break;
      }
      if (m.empty()) m = "x";
    }
    check_seeds(w, transitive::parse_seeds(m, w), "a mutated BED");
  }

  // the lines of world intervals: split where a sequence ends
  const lift::Interval& g = seeds.iv[0];
  std::string out;
  uint64_t n = transitive::lines(out, w, g, 10, 20);
  n += transitive::lines(out, w, g, 95, 105);
  n += transitive::lines(out, w, g, 99, 151);
  n += transitive::lines(out, w, seeds.iv[1], 0, 290);
  n += transitive::lines(out, w, seeds.iv[2], 289, 290);
  n += transitive::lines(out, w, g, 150, 150);
  expect(n == 1 + 2 + 3 + 5 + 1 + 0, "the number of lines");
  expect_text(out,
              "chrA\t10\t20\tgene1\tchrA\t10\t20\n"
              "chrA\t95\t100\tgene1\tchrA\t10\t20\nchrB\t0\t5\tgene1\tchrA\t10\t20\n"
              "chrA\t99\t100\tgene1\tchrA\t10\t20\nchrB\t0\t50\tgene1\tchrA\t10\t20\nchrC\t0\t1\tgene1\tchrA\t10\t20\n"
              "chrA\t0\t100\t.\thapY\t0\t40\nchrB\t0\t50\t.\thapY\t0\t40\nchrC\t0\t70\t.\thapY\t0\t40\nhapX\t0\t30\t.\thapY\t0\t40\nhapY\t0\t40\t.\thapY\t0\t40\n"
              "hapY\t39\t40\tlast\thapX\t29\t30\n",
              "the lines");
  // the whole file (file) on the same intervals: seed 0 reaches the first three, seed 1 the whole world, seed 2 the last base, seed 3
  // nothing -- the lines above in the order of the seeds; without a closure (no record was added) every seed reaches itself
  {
    const std::vector<transitive::ClosureIv> ivs = {{10, 20, 0, 0}, {95, 105, 0, 0}, {99, 151, 0, 0}, {0, 290, 1, 0}, {289, 290, 2, 0}};
    const std::vector<transitive::SeedCall> per = {{0, 3, 72}, {3, 1, 290}, {4, 1, 1}, {0, 0, 0}};
    std::ostringstream file;
    expect(transitive::file(file, w, seeds.iv, per.data(), ivs.data()) == 12, "file: the number of lines");
    expect_text(file.str(), out, "file: the lines");
    std::ostringstream alone;
    expect(transitive::file(alone, w, seeds.iv, per.data(), nullptr) == 4, "file without a closure: the number of lines");
    expect_text(alone.str(), "chrA\t10\t20\tgene1\tchrA\t10\t20\nhapY\t0\t40\t.\thapY\t0\t40\nhapX\t29\t30\tlast\thapX\t29\t30\nchrA\t10\t20\tgene1\tchrA\t10\t20\n",
                "file without a closure");
    // more than a MiB: flushed in parts, nothing lost
    std::vector<transitive::ClosureIv> many(50000, transitive::ClosureIv{10, 20, 0, 0});
    const std::vector<transitive::SeedCall> all = {{0, many.size(), 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    std::ostringstream big;
    expect(transitive::file(big, w, seeds.iv, all.data(), many.data()) == many.size(), "file over a MiB: the number of lines");
    expect(big.str().size() == many.size() * 28, "file over a MiB: the bytes");
  }
  for (int it = 0; it < 100000; ++it) {
    uint64_t a = next() % 290, b = a + 1 + next() % (290 - a);
    std::string text;
    const uint64_t k = transitive::lines(text, w, g, a, b);
    uint64_t sum = 0, lines = 0;
    for (size_t at = 0; at < text.size();) {
      const size_t nl = text.find('\n', at), t1 = text.find('\t', at), t2 = text.find('\t', t1 + 1), t3 = text.find('\t', t2 + 1);
      uint64_t s = 0, e = 0;
      const int seq = w.find(text.substr(at, t1 - at));
      if (seq < 0 || !lift::decimal(text, t1 + 1, t2, &s) || !lift::decimal(text, t2 + 1, t3, &e) || s >= e || e > w.lengths[(size_t)seq] ||
          w.offsets[(size_t)seq] + s != a + sum) { fprintf(stderr, "FAIL a random interval [%llu, %llu)\n", (unsigned long long)a, (unsigned long long)b); ++fails; break; }
      sum += e - s;
      ++lines;
      at = nl + 1;
    }
    if (sum != b - a || lines != k) { fprintf(stderr, "FAIL the pieces of [%llu, %llu) do not add up\n", (unsigned long long)a, (unsigned long long)b); ++fails; }
    if (fails) break;
  }

  // a record's place in the world: the first base of its forward query window, whatever the strand; the largest coordinates
  expect(transitive::query_world(220, 7) == 227, "query_world");
  expect(transitive::query_world(((uint64_t)1 << 40) - 100, 99) == ((uint64_t)1 << 40) - 1, "query_world at the world's end");

  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("transitive_check: ok\n");
  return 0;
}
