// emit_plan_check.cpp -- the chunk plan of the passes that emit lists (wfmash_amd/csrc/wfa_emit_plan.h) against a planner that walks problem by
// problem, on the shapes a shared frame can get wrong and on seeded random offsets.  A program of its own, built with
// -fsanitize=address,undefined by tests/test_emit_plan_cpu.py and run directly; it needs no device and no library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../wfmash_amd/csrc/wfa_emit_plan.h"

namespace {

typedef unsigned long long u64;
typedef std::vector<u64> Offsets;  // n + 1 prefix sums

int failures = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++failures;                                                     \
      fprintf(stderr, "emit_plan_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "\n");                                          \
    }                                                                 \
  } while (0)

// the plan, one problem at a time: a chunk takes the next problem while the cost with it fits, and one problem in any case
template <class Cost, class Size>
wfm::EmitPlan linear_plan(size_t n, u64 cap, Cost cost, Size size) {
  wfm::EmitPlan plan;
  size_t ka = 0;
  while (ka < n) {
    size_t kb = ka + 1;
    while (kb < n && cost(ka, kb + 1) <= cap) ++kb;
    if (cost(ka, kb) != 0) {
      plan.chunks.push_back(std::make_pair(ka, kb));
      if (size(ka, kb) > plan.widest) plan.widest = size(ka, kb);
    }
    ka = kb;
  }
  return plan;
}

Offsets prefix(const std::vector<u64>& counts, u64 base = 0) {
  Offsets off(counts.size() + 1);
  off[0] = base;
  for (size_t i = 0; i < counts.size(); ++i) off[i + 1] = off[i] + counts[i];
  return off;
}

// one stream of `elem` bytes an element, sized to `round`; with a second stream of bytes sized to whole slices (as wfm_call_variants
// and wfm_maf_rows place theirs)
struct Streams {
  const Offsets* recs;
  u64 elem, round;
  const Offsets* bytes;  // (or null)
  u64 slice;
  u64 cost(size_t a, size_t b) const { return ((*recs)[b] - (*recs)[a]) * elem + (bytes ? (*bytes)[b] - (*bytes)[a] : 0); }
  u64 size(size_t a, size_t b) const {
    const u64 r = (((*recs)[b] - (*recs)[a]) * elem + round - 1) / round * round;
    return r + (bytes ? ((*bytes)[b] - (*bytes)[a] + slice - 1) / slice * slice : 0);
  }
};

// both planners on one case; what every plan must hold besides
wfm::EmitPlan compare(const char* what, size_t n, u64 cap, const Streams& st) {
  auto cost = [&](size_t a, size_t b) { return st.cost(a, b); };
  auto size = [&](size_t a, size_t b) { return st.size(a, b); };
  const wfm::EmitPlan got = wfm::emit_plan(n, cap, cost, size), want = linear_plan(n, cap, cost, size);
  CHECK(got.chunks == want.chunks, "%s: %zu chunks, the linear planner has %zu", what, got.chunks.size(), want.chunks.size());
  CHECK(got.widest == want.widest, "%s: widest %llu, the linear planner has %llu", what, got.widest, want.widest);
  u64 covered = 0;
  size_t at = 0;
  for (const auto& c : got.chunks) {
    CHECK(c.first >= at && c.first < c.second && c.second <= n, "%s: chunk [%zu, %zu) out of order or out of range", what, c.first, c.second);
    CHECK(st.cost(c.first, c.second) > 0, "%s: chunk [%zu, %zu) is empty", what, c.first, c.second);
    CHECK(st.cost(c.first, c.second) <= cap || c.second == c.first + 1, "%s: chunk [%zu, %zu) exceeds the cap with more than one problem", what, c.first, c.second);
    CHECK(c.second == n || st.cost(c.first, c.second + 1) > cap, "%s: chunk [%zu, %zu) could hold the next problem", what, c.first, c.second);
    CHECK(st.cost(at, c.first) == 0, "%s: output between %zu and %zu is in no chunk", what, at, c.first);
    CHECK(st.size(c.first, c.second) <= got.widest, "%s: chunk [%zu, %zu) is wider than the widest", what, c.first, c.second);
    covered += st.cost(c.first, c.second);
    at = c.second;
  }
  CHECK(st.cost(at, n) == 0, "%s: output behind %zu is in no chunk", what, at);
  CHECK(covered == st.cost(0, n), "%s: the chunks hold %llu of %llu", what, covered, st.cost(0, n));
  return got;
}

wfm::EmitPlan compare1(const char* what, const Offsets& off, u64 elem, u64 cap) {
  return compare(what, off.size() - 1, cap, Streams{&off, elem, 1, nullptr, 1});
}

typedef std::vector<std::pair<size_t, size_t>> Chunks;

}  // namespace

int main() {
  // one problem
  {
    const Offsets off = prefix({7});
    CHECK(compare1("n = 1", off, 32, 1000).chunks == Chunks({{0, 1}}), "n = 1: not one chunk");
    CHECK(compare1("n = 1, over the cap", off, 32, 1).chunks == Chunks({{0, 1}}), "n = 1 over the cap: not one chunk");
    const Offsets none = prefix({0});
    const wfm::EmitPlan p = compare1("n = 1, empty", none, 32, 1000);
    CHECK(p.chunks.empty() && p.widest == 0, "n = 1, empty: a plan of %zu chunks, widest %llu", p.chunks.size(), p.widest);
  }
  // every problem larger than the cap: each is its own chunk
  {
    const Offsets off = prefix({9, 5, 12, 5, 40});
    const wfm::EmitPlan p = compare1("all over the cap", off, 16, 64);
    CHECK(p.chunks == Chunks({{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}}) && p.widest == 40 * 16, "all over the cap: %zu chunks, widest %llu", p.chunks.size(), p.widest);
  }
  // empty problems at the start, at the end and between chunks, and a run of empties that is a chunk of its own where the cap holds one
  // problem: no empty chunk in the plan, and no output lost
  {
    const Offsets off = prefix({0, 20, 0, 0, 20, 0});
    const wfm::EmitPlan own = compare1("empties at the edges, one problem a chunk", off, 32, 1);
    CHECK(own.chunks.size() == 2 && own.widest == 20 * 32, "empties at the edges: %zu chunks, widest %llu", own.chunks.size(), own.widest);
    for (const auto& c : own.chunks) CHECK(off[c.second] - off[c.first] == 20, "empties at the edges: a chunk of %llu", off[c.second] - off[c.first]);
    const wfm::EmitPlan one = compare1("empties at the edges, one chunk", off, 32, 40 * 32);
    CHECK(one.chunks == Chunks({{0, 6}}), "empties at the edges under a wide cap: not one chunk");
    std::vector<u64> counts(40, 0);
    counts[3] = 5; counts[4] = 6; counts[30] = 4;  // 25 empties between: whole chunks of nothing where a chunk ends at a full problem
    const Offsets wide = prefix(counts);
    const wfm::EmitPlan gap = compare1("a run of empties", wide, 8, 5 * 8);
    CHECK(gap.chunks.size() == 3 && gap.widest == 6 * 8, "a run of empties: %zu chunks, widest %llu", gap.chunks.size(), gap.widest);
    compare1("a run of empties, cap below a problem", wide, 8, 1);
  }
  // all problems empty
  {
    const Offsets off = prefix(std::vector<u64>(17, 0));
    const wfm::EmitPlan p = compare1("all empty", off, 16, 1);
    CHECK(p.chunks.empty() && p.widest == 0, "all empty: a plan of %zu chunks, widest %llu", p.chunks.size(), p.widest);
  }
  // two streams, records x size + bytes, where one stream is empty in a chunk and the other is not
  {
    const Offsets recs = prefix({0, 3, 0, 2, 0, 0}), bytes = prefix({0, 100, 50, 0, 0, 7});
    const Streams st{&recs, 40, 16, &bytes, 64};
    const wfm::EmitPlan p = compare("two streams", 6, 230, st);
    // [0, 2): 3 * 40 + 100 = 220; [2, 4): 50 + 80 = 130 (with [4, 6): 137 fits too)
    CHECK(p.chunks == Chunks({{0, 2}, {2, 6}}), "two streams: %zu chunks", p.chunks.size());
    CHECK(p.widest == 128 + 128, "two streams: widest %llu", p.widest);
    const wfm::EmitPlan each = compare("two streams, one problem a chunk", 6, 1, st);
    CHECK(each.chunks == Chunks({{1, 2}, {2, 3}, {3, 4}, {5, 6}}), "two streams, one problem a chunk: %zu chunks", each.chunks.size());
  }
  // offsets near 2^40
  {
    const u64 big = (u64)1 << 40;
    const Offsets off = prefix({big - 3, 5, 0, big + 1, 2, 0}, 0);
    compare1("offsets near 2^40", off, 32, big * 32);
    compare1("offsets near 2^40, narrow cap", off, 32, 64);
    const Offsets based = prefix({4, 0, 9, 1}, big - 6);  // a list whose offsets begin there
    CHECK(compare1("offsets from 2^40 on", based, 16, 10 * 16).chunks == Chunks({{0, 2}, {2, 4}}), "offsets from 2^40 on: another plan");
  }
  // seeded random offsets, one and two streams
  for (unsigned seed = 1; seed <= 4000; ++seed) {
    std::mt19937_64 rng(0x3e11700ull + seed);
    const size_t n = 1 + rng() % 48;
    std::vector<u64> a(n), b(n);
    const unsigned zero_of = 1 + rng() % 4;
    for (size_t i = 0; i < n; ++i) {
      a[i] = rng() % zero_of == 0 ? 0 : rng() % 50;
      b[i] = rng() % zero_of == 0 ? 0 : rng() % 3000;
    }
    const Offsets recs = prefix(a), bytes = prefix(b);
    const u64 cap = 1 + rng() % (seed % 3 == 0 ? 200 : 20000);
    if (seed % 2) compare("random, one stream", n, cap, Streams{&recs, 32, 1, nullptr, 1});
    else compare("random, two streams", n, cap, Streams{&recs, 40, 16, &bytes, 64});
    if (failures) { fprintf(stderr, "emit_plan_check: seed %u\n", seed); break; }
  }
  if (failures) return 1;
  printf("emit_plan_check: ok\n");
  return 0;
}
