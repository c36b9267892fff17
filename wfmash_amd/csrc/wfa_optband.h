// wfa_optband.h -- the band of wfm_check_optimal (include/wfmash_hip.h): the diagonals an alignment of price <= S can touch, and the
// DP cells that lie on them.  Host only, no device types: the C ABI plans with it and the CPU suite holds it against a full-matrix
// DP through wfmh_test_opt_band (tests/test_optcheck_cpu.py).  It shares nothing with the aligners' planners (wfa_plan.h).
#ifndef WFMASH_AMD_WFA_OPTBAND_H_
#define WFMASH_AMD_WFA_OPTBAND_H_

#include <stdint.h>

#include <algorithm>

namespace wfm {

struct OptPen { int64_t x, o1, e1, o2, e2; };

// the price of one gap run of L bases (0 for L <= 0): non-decreasing and subadditive in L
inline int64_t opt_gap(const OptPen& p, int64_t L) {
  if (L <= 0) return 0;
  return std::min(p.o1 + p.e1 * L, p.o2 + p.e2 * L);
}

struct OptBand { int64_t lo, hi; uint64_t cells; };

// Diagonals k = j - i (i: pattern index, j: text index).  Start diagonals [-pbf, tbf], end diagonals [kf - tef, kf + pef] with
// kf = tlen - plen; the free lengths are taken clamped to their sequence (end-to-end: all 0).  Everything between the lowest and
// the highest of those is in the band; a diagonal k above needs k - tbf inserted bases to be reached and k - kf - pef deleted ones
// to come back from, in runs of their own, and is in the band iff g(k - tbf) + g(k - kf - pef) <= S; below likewise with the
// roles swapped.  Both tests are monotone in k, so the band is one interval; it is cut to the matrix, [-plen, tlen].
// cells = the (i, j) with 0 <= i <= plen, 0 <= j <= tlen on those diagonals.
inline OptBand opt_band(const OptPen& pen, int64_t plen, int64_t tlen, int64_t pbf, int64_t pef, int64_t tbf, int64_t tef, int64_t S) {
  pbf = std::min(std::max<int64_t>(pbf, 0), plen); pef = std::min(std::max<int64_t>(pef, 0), plen);
  tbf = std::min(std::max<int64_t>(tbf, 0), tlen); tef = std::min(std::max<int64_t>(tef, 0), tlen);
  const int64_t kf = tlen - plen;
  const int64_t hi0 = std::max(tbf, kf + pef), lo0 = std::min(-pbf, kf - tef);
  // the last k in (hi0, tlen] that passes (binary search on a monotone test)
  int64_t a = hi0, b = tlen;  // a passes (or is hi0), everything above b fails or is outside the matrix
  while (a < b) {
    const int64_t mid = a + (b - a + 1) / 2;
    if (opt_gap(pen, mid - tbf) + opt_gap(pen, mid - kf - pef) <= S) a = mid; else b = mid - 1;
  }
  const int64_t hi = a;
  a = -plen; b = lo0;  // b passes (or is lo0)
  while (a < b) {
    const int64_t mid = a + (b - a) / 2;
    if (opt_gap(pen, -pbf - mid) + opt_gap(pen, kf - tef - mid) <= S) b = mid; else a = mid + 1;
  }
  const int64_t lo = b;
  // cells of diagonal k: i from max(0, -k) to min(plen, tlen - k).  Piecewise linear in k; summed in closed form over the (at most
  // three) pieces between the breakpoints 0 and kf
  auto count = [&](int64_t k) { return std::min(plen, tlen - k) - std::max<int64_t>(0, -k) + 1; };
  auto sum_piece = [&](int64_t k0, int64_t k1) -> uint64_t {  // count() is linear on [k0, k1]
    if (k0 > k1) return 0;
    return (uint64_t)((count(k0) + count(k1)) * (k1 - k0 + 1) / 2);
  };
  int64_t cuts[4] = {lo, std::min(std::max(std::min<int64_t>(0, kf), lo), hi), std::min(std::max(std::max<int64_t>(0, kf), lo), hi), hi};
  uint64_t cells = sum_piece(cuts[0], cuts[1]);
  if (cuts[1] < cuts[2]) cells += sum_piece(cuts[1] + 1, cuts[2]);
  if (cuts[2] < cuts[3]) cells += sum_piece(cuts[2] + 1, cuts[3]);
  return OptBand{lo, hi, cells};
}

}  // namespace wfm

#endif
