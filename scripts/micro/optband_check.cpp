// The band planner of wfm_check_optimal (wfmash_amd/csrc/wfa_optband.h) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/optband_check.cpp -o /tmp/optband_check && /tmp/optband_check
// Random problems up to the ABI's limits (plen + tlen <= 2^29, penalties up to 32767, claims up to 2^29 - 1, free lengths of any
// sign and size): the band must be one interval inside [-plen, tlen] that holds every start and end diagonal, its ends must be
// exactly where the lemma's test flips, and the closed-form cell count must equal the sum over diagonals (taken directly where the band
// is narrow enough to walk).  No signed overflow anywhere: the arithmetic is 64-bit and the build traps on it.
#include <cstdio>
#include <cstdlib>

#include "../../wfmash_amd/csrc/wfa_optband.h"

static int fails = 0;
static uint64_t x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
static int64_t pick(int64_t n) { return n <= 0 ? 0 : (int64_t)(rnd() % (uint64_t)(n + 1)); }

int main() {
  using wfm::OptBand; using wfm::OptPen; using wfm::opt_band; using wfm::opt_gap;
  for (int it = 0; it < 300000; ++it) {
    const int big = it % 7 == 0;
    const int64_t cap = big ? ((int64_t)1 << 29) : 3000;
    const int64_t plen = pick(cap / 2), tlen = pick(cap - plen > cap / 2 ? cap / 2 : cap - plen);
    const int64_t pmax = it % 3 == 0 ? 32767 : 60;
    const OptPen pen{1 + pick(pmax - 1), pick(pmax), 1 + pick(pmax - 1), pick(pmax), 1 + pick(pmax - 1)};
    int64_t f[4];
    for (int q = 0; q < 4; ++q) {
      const int64_t n = q < 2 ? plen : tlen;
      switch (rnd() % 5) { case 0: f[q] = 0; break; case 1: f[q] = n; break; case 2: f[q] = pick(8); break; case 3: f[q] = pick(n); break; default: f[q] = (int64_t)(rnd() % 4000000000ull) - 2000000000; }
    }
    const int64_t S = it % 5 == 0 ? ((int64_t)1 << 29) - 1 : pick(big ? 200000 : 5000);
    const OptBand b = opt_band(pen, plen, tlen, f[0], f[1], f[2], f[3], S);
    auto clampf = [](int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; };
    const int64_t pbf = clampf(f[0], plen), pef = clampf(f[1], plen), tbf = clampf(f[2], tlen), tef = clampf(f[3], tlen), kf = tlen - plen;
    const int64_t hi0 = tbf > kf + pef ? tbf : kf + pef, lo0 = -pbf < kf - tef ? -pbf : kf - tef;
    auto above = [&](int64_t k) { return opt_gap(pen, k - tbf) + opt_gap(pen, k - kf - pef) <= S; };
    auto below = [&](int64_t k) { return opt_gap(pen, -pbf - k) + opt_gap(pen, kf - tef - k) <= S; };
    bool ok = -plen <= b.lo && b.lo <= lo0 && hi0 <= b.hi && b.hi <= tlen;
    ok = ok && (b.hi == hi0 || above(b.hi)) && (b.hi == tlen || !above(b.hi + 1));
    ok = ok && (b.lo == lo0 || below(b.lo)) && (b.lo == -plen || !below(b.lo - 1));
    if (ok && b.hi - b.lo < 20000) {
      uint64_t cells = 0;
      for (int64_t k = b.lo; k <= b.hi; ++k) cells += (uint64_t)((plen < tlen - k ? plen : tlen - k) - (k < 0 ? -k : 0) + 1);
      ok = cells == b.cells;
    }
    if (ok && b.lo == -plen && b.hi == tlen) ok = b.cells == (uint64_t)(plen + 1) * (uint64_t)(tlen + 1);
    if (!ok) {
      if (++fails < 10) fprintf(stderr, "FAIL: plen %lld tlen %lld free %lld %lld %lld %lld S %lld -> [%lld, %lld] %llu cells\n", (long long)plen, (long long)tlen, (long long)f[0],
                                (long long)f[1], (long long)f[2], (long long)f[3], (long long)S, (long long)b.lo, (long long)b.hi, (unsigned long long)b.cells);
    }
  }
  printf(fails ? "%d failures\n" : "optband_check ok\n", fails);
  return fails ? 1 : 0;
}
