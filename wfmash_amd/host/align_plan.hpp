// align_plan.hpp -- what the align driver (aligner.cpp) decides without a device: how many workers a GPU gets, how the
// mapping file is cut into batches, and the union of the workers' device-busy intervals.  Pure arithmetic, held by
// tests/test_host_logic_cpu.py through wfmh_test_plan_batch_bytes and wfmh_test_align_plan.
#pragma once

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace align {

// Workers (batches in flight) per GPU when there are host threads for it: the host stages of a batch (sequence fetches, CIGAR
// surgery, PAF text) run while the device works on another.  override_ > 0 (WFM_ALIGN_WORKERS, A/B runs) wins.
// (four since round 5 where the host has 16 threads per GPU: with the round's kernels a batch of a pangenome rank is 100 ms of device time in 170 ms
// of its worker's, and a full-size rank went from 1.37 - 1.42 s on three workers to 1.18 - 1.29 s on four -- gpurun_out/r5i.log; six gain nothing more)
// (six since round 6 where the host has 48 threads per GPU: on the all-vs-all job at north_star's size -- 187 batches -- the device's busy time went from 7.58 to 7.30 s
// and the align phase from 8.3 - 8.45 to 7.8 - 8.1 s, eight workers 8.2 - 8.3 s: gpurun_out/r6cb; a rank's 28 batches are the same 1.08 - 1.12 s on four, five or six)
inline size_t workers_per_gpu(size_t threads, size_t ngpu, size_t override_) {
  if (override_) return override_;
  if (threads >= 48 * ngpu) return 6;
  if (threads >= 16 * ngpu) return 4;
  if (threads >= 12 * ngpu) return 3;
  return threads >= 2 * ngpu ? 2 : 1;
}

// bases a mapping row will align, padding aside (the reader sizes batches by it)
inline uint64_t row_bases(const std::string& line) {
  uint64_t v[9] = {0};
  size_t pos = 0;
  for (int col = 0; col < 9; ++col) {
    while (pos < line.size() && std::isspace((unsigned char)line[pos])) ++pos;
    const size_t st = pos;
    while (pos < line.size() && !std::isspace((unsigned char)line[pos])) ++pos;
    if (st == pos) return 0;
    if (col == 2 || col == 3 || col == 7 || col == 8) v[col] = strtoull(line.c_str() + st, nullptr, 10);
  }
  return (v[3] > v[2] ? v[3] - v[2] : 0) + (v[8] > v[7] ? v[8] - v[7] : 0);
}

// Batches the caps on records and bases demand of a file of file_bytes, judged by its first rows (rows > 0, row_bytes > 0).
inline uint64_t batches_needed(uint64_t file_bytes, uint64_t rows, uint64_t row_bytes, uint64_t row_bases_sum, uint64_t batch_records, uint64_t batch_bases) {
  const double est_rows = (double)file_bytes / ((double)row_bytes / (double)rows);
  const double est_bases = est_rows * ((double)row_bases_sum / (double)rows);
  return (uint64_t)std::ceil(std::max(est_rows / (double)std::max<uint64_t>(1, batch_records), est_bases / (double)std::max<uint64_t>(1, batch_bases)));
}

// Bytes of the mapping file one batch may hold (~0: no limit beyond batch_records / batch_bases).  file_bytes = 0: the file
// cannot be rewound or is empty.  rows / row_bytes / row_bases_sum: the first rows looked at (rows = 0: none).
// Several GPUs: no batch may hold more than an eighth of one GPU's share of the file.  One GPU: a file of one batch stays one
// batch (min_batches, WFM_ALIGN_MIN_BATCHES, cuts it for A/B runs); a file of a few batches is cut into a multiple of the
// workers' number, level ones -- four batches on three workers are two rounds of which the second leaves the device to one
// batch's tails.
inline uint64_t plan_batch_bytes(uint64_t file_bytes, uint64_t rows, uint64_t row_bytes, uint64_t row_bases_sum, uint64_t batch_records,
                                 uint64_t batch_bases, uint64_t nworkers, uint64_t ngpu, uint64_t min_batches, bool level) {
  if (file_bytes == 0) return ~0ull;
  uint64_t want = ngpu > 1 ? 8 * ngpu : std::max<uint64_t>(1, min_batches);
  if (level && nworkers > 1 && rows > 0 && row_bytes > 0) {
    const uint64_t need = batches_needed(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases);
    if (need >= 2 && need < 8 * nworkers) want = std::max<uint64_t>(want, (need + nworkers - 1) / nworkers * nworkers);
  }
  return want > 1 ? std::max<uint64_t>(1, file_bytes / want + 1) : ~0ull;
}

// The number of batches the file will come to, or ~0 when no rows were looked at (a stream, or one worker): never fewer than
// the caps demand, nor than batch_bytes cuts.
inline uint64_t estimate_batches(uint64_t file_bytes, uint64_t rows, uint64_t row_bytes, uint64_t row_bases_sum, uint64_t batch_records,
                                 uint64_t batch_bases, uint64_t batch_bytes) {
  if (rows == 0 || row_bytes == 0) return ~0ull;
  uint64_t need = batches_needed(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases);
  if (batch_bytes != ~0ull) need = std::max<uint64_t>(need, (file_bytes + batch_bytes - 1) / batch_bytes);
  return std::max<uint64_t>(1, need);
}

using Interval = std::pair<double, double>;

// The union of intervals as disjoint ones in rising order (v is sorted in place); empty and inverted ones add nothing.
inline std::vector<Interval> interval_union(std::vector<Interval>& v) {
  std::sort(v.begin(), v.end());
  std::vector<Interval> u;
  double lo = 0, hi = -1;
  for (const auto& x : v) {
    if (x.first > hi) { if (hi > lo) u.emplace_back(lo, hi); lo = x.first; hi = x.second; }
    else hi = std::max(hi, x.second);
  }
  if (hi > lo) u.emplace_back(lo, hi);
  return u;
}
inline double total_length(const std::vector<Interval>& u) {
  double total = 0;
  for (const auto& x : u) total += x.second - x.first;
  return total;
}
// (first start, length) of the span from the first interval's start to the last end, of intervals sorted by start; the length is
// at least 1e-6 so that it can be divided by
inline Interval span_of(const std::vector<Interval>& sorted) {
  double lo = sorted.front().first, hi = lo;
  for (const auto& x : sorted) hi = std::max(hi, x.second);
  return Interval(lo, std::max(hi - lo, 1e-6));
}
// how much of each of the `bins` equal parts of [from, from + span) the disjoint intervals cover
inline std::vector<double> covered_per_bin(const std::vector<Interval>& u, double from, double span, int bins) {
  std::vector<double> covered((size_t)bins, 0.0);
  for (const auto& x : u)
    for (int q = 0; q < bins; ++q) {
      const double qa = from + span * q / bins, qb = from + span * (q + 1) / bins;
      const double o = std::min(x.second, qb) - std::max(x.first, qa);
      if (o > 0) covered[(size_t)q] += o;
    }
  return covered;
}

}  // namespace align
