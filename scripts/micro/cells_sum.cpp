// cells_sum of wfmash_amd/csrc/wfa_plan.h against the row-by-row sum:  g++ -std=c++17 -O1 scripts/micro/cells_sum.cpp && ./a.out
#include <cstdio>
#include <cstdlib>

#include "../../wfmash_amd/csrc/wfa_plan.h"
using namespace wfm;
int main() {
  srand(1);
  long bad = 0, n = 0;
  for (int it = 0; it < 400000; ++it) {
    int pl = rand() % 3000 + (rand() % 4 == 0 ? 0 : 1), tl = rand() % 3000 + 1;
    if (rand() % 3 == 0) { pl = rand() % 60 + 1; tl = rand() % 60 + 1; }
    int sub = rand() % 3 == 0 ? SUB_NONE : rand() % 4000;
    int a = rand() % 3500, b = a + rand() % 400 - 5;
    if (rand() % 5 == 0) { a = 0; b = rand() % 6000; }
    const Rng rg = make_rng(pl, tl, sub);
    int64_t want = 0;
    for (int s = a; s <= b; ++s) want += std::max(0, rng_hi(rg, s) - rng_lo(rg, s) + 1);
    int64_t got = cells_sum(pl, tl, sub, a, b);
    ++n;
    if (got != want) { if (bad < 10) printf("pl %d tl %d sub %d a %d b %d: got %lld want %lld\n", pl, tl, sub, a, b, (long long)got, (long long)want); ++bad; }
  }
  printf("%ld cases, %ld bad\n", n, bad);
  return bad != 0;
}
