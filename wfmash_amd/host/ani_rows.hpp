// ani_rows.hpp -- one row of the group-by-group ANI table (--ani-matrix) and its text form.  Plain C++ without a device, so
// that the CPU test-suite and scripts/micro/ani_rows_check.cpp can drive it on their own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "map_stats.hpp"

namespace skch {
namespace Stat {

constexpr int kAniTableK = 21;  // the estimate's k (map_stats.hpp:328)

struct AniRow {
  std::string query_group, target_group;  // SequenceIdManager::getGroupPrefix
  uint64_t query_hashes = 0, target_hashes = 0;  // sizes of the two pooled sketches
  uint64_t shared = 0;                    // their multiset intersection
  double jaccard = 0, ani = 0;
};

// The estimate's arithmetic on one pair (map_stats.hpp:735-741): shared over the smaller sketch, through j2md(float, int).  A pair
// without a shared hash, or with an empty sketch, is a row of zeros -- the estimate drops such pairs, the table shows them.
inline AniRow ani_row(std::string query_group, std::string target_group, uint64_t query_hashes, uint64_t target_hashes, uint64_t shared) {
  AniRow r;
  r.query_group = std::move(query_group);
  r.target_group = std::move(target_group);
  r.query_hashes = query_hashes;
  r.target_hashes = target_hashes;
  r.shared = shared;
  const uint64_t smaller = std::min(query_hashes, target_hashes);
  if (shared > 0 && smaller > 0) {
    r.jaccard = static_cast<double>(shared) / static_cast<double>(smaller);
    const double mash_dist = j2md((float)r.jaccard, kAniTableK);
    r.ani = 1.0 - mash_dist;
  }
  return r;
}

inline const char* ani_tsv_header() { return "#query_group\ttarget_group\tquery_hashes\ttarget_hashes\tshared\tjaccard\tani\n"; }

inline std::string ani_tsv(const std::vector<AniRow>& rows) {
  std::string out = ani_tsv_header();
  char num[160];
  for (const AniRow& r : rows) {
    out += r.query_group;
    out += '\t';
    out += r.target_group;
    snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%.6f\t%.6f\n", (unsigned long long)r.query_hashes, (unsigned long long)r.target_hashes,
             (unsigned long long)r.shared, r.jaccard, r.ani);
    out += num;
  }
  return out;
}

}  // namespace Stat
}  // namespace skch
