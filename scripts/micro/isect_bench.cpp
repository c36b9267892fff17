// Times wfm_sketch_intersections against the estimate's host merge loop on synthetic pooled sketches (profiles/ani_matrix.md).
//   g++ -O3 -std=c++17 scripts/micro/isect_bench.cpp -Iinclude -Lwfmash_amd -lwfmash_hip -Wl,-rpath,$PWD/wfmash_amd -o isect_bench
//   ./isect_bench G [device|both]
// G groups of 4096 hashes each: every group is one common set of 4096 random 64-bit values with a random fifth of them replaced by
// values of its own, sorted -- related haplotypes, two of which share about two thirds of a sketch.  "device": one warm-up call,
// then three timed calls of the whole G x G matrix; the clock is the host's and stops after the call has returned, which it does
// with the counts on the host (its last step is a stream synchronise).  "both": the same, then the G x G merges of
// estimate_identity_for_groups (wfmash_amd/host/ani_estimate.cpp: the `while` over two sketches, restated below word for word) in
// one thread, and every cell compared.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wfmash_hip.h"

static uint64_t x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }

int main(int argc, char** argv) {
  const int64_t G = argc > 1 ? atoll(argv[1]) : 64;
  const bool host_too = argc > 2 && !strcmp(argv[2], "both");
  const int S = 4096;
  std::vector<uint64_t> common((size_t)S);
  for (auto& v : common) v = rnd();
  std::vector<uint64_t> hashes((size_t)G * S);
  std::vector<int64_t> offsets((size_t)G + 1);
  std::vector<int32_t> all((size_t)G);
  for (int64_t g = 0; g < G; ++g) {
    uint64_t* s = hashes.data() + g * S;
    for (int i = 0; i < S; ++i) s[i] = rnd() % 5 == 0 ? rnd() : common[(size_t)i];
    std::sort(s, s + S);
    offsets[(size_t)g] = g * S;
    all[(size_t)g] = (int32_t)g;
  }
  offsets[(size_t)G] = G * S;
  wfm_handle_t* h = nullptr;
  if (wfm_create(0, &h) != WFM_OK) { fprintf(stderr, "no device\n"); return 2; }
  std::vector<uint32_t> dev((size_t)G * G);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  double best = 1e300, worst = 0;
  for (int rep = 0; rep < 4; ++rep) {
    const auto t0 = now();
    const int rc = wfm_sketch_intersections(h, hashes.data(), offsets.data(), G, all.data(), G, all.data(), G, dev.data());
    const double t = ms(t0, now());
    if (rc != WFM_OK) { fprintf(stderr, "wfm_sketch_intersections: %s\n", wfm_last_error(h)); return 1; }
    if (rep == 0) { printf("G %lld: warm-up call %.2f ms\n", (long long)G, t); continue; }
    best = std::min(best, t); worst = std::max(worst, t);
  }
  printf("G %lld: device call (upload, check, %lld cells, download) best %.2f ms, worst %.2f ms of 3\n", (long long)G, (long long)(G * G), best, worst);
  fflush(stdout);
  if (host_too) {
    int64_t differ = 0;
    uint64_t total = 0;
    const auto t0 = now();
    for (int64_t a = 0; a < G; ++a) {
      for (int64_t b = 0; b < G; ++b) {
        const uint64_t *qs = hashes.data() + a * S, *ts = hashes.data() + b * S;
        const size_t qn = S, tn = S;
        size_t shared = 0, i = 0, j = 0;
        while (i < qn && j < tn) {
          if (qs[i] == ts[j]) { ++shared; ++i; ++j; }
          else if (qs[i] < ts[j]) ++i;
          else ++j;
        }
        total += shared;
        if (shared != dev[(size_t)(a * G + b)]) ++differ;
      }
      if (G >= 1024 && a % 256 == 255) { printf("  host merge: %lld of %lld rows after %.0f ms\n", (long long)a + 1, (long long)G, ms(t0, now())); fflush(stdout); }
    }
    printf("G %lld: host merge loop, one thread %.2f ms; mean shared %.1f; cells that differ from the device: %lld\n", (long long)G, ms(t0, now()),
           (double)total / (double)(G * G), (long long)differ);
    if (differ) return 1;
  }
  wfm_destroy(h);
  return 0;
}
