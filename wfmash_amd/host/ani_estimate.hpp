// ani_estimate.hpp -- automatic identity threshold: skch::Stat::estimate_identity_for_groups
// (src/map/include/map_stats.hpp:325-822), the default `-p ani50-2` path of main.cpp:72-128.
// Every sequence gets a bottom-4096 MinHash at k = 21 on the GPU (wfm_minhash_sketch); sketches are
// pooled per PanSN group, all query-group x target-group pairs of different groups give a Mash ANI,
// and the requested percentile of those, plus the adjustment, becomes the identity threshold.
// The table those ANIs come from (the reference prints it to stderr, map_stats.hpp:746-752) is ani_matrix: the same pooled
// sketches, their shared-hash counts from one wfm_sketch_intersections call on the device.
#pragma once

#include <map>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "ani_rows.hpp"
#include "map_types.hpp"
#include "sequence_ids.hpp"

namespace skch {
namespace Stat {

// returns the adjusted ANI in [0, 1]; fixed::percentage_identity (0.70) when nothing can be compared
double estimate_identity_for_groups(const Parameters& params, const SequenceIdManager& idManager, wfm_handle_t* h);
// the same with the sequences spread over several GPUs of the node (one sketch per sequence, independent of each other)
double estimate_identity_for_groups(const Parameters& params, const SequenceIdManager& idManager, const std::vector<wfm_handle_t*>& hs);

// The pooled sketch of every query group and of every target group, by group id, and how many sequences went into either side:
// roles, preload, one sketch per sequence over the handles, pooling.  What the estimate and the table are both made from.
struct GroupSketches {
  std::map<int, std::vector<hash_t>> query_groups, target_groups;
  int query_seq_count = 0, target_seq_count = 0;
};
GroupSketches sketch_groups(const Parameters& params, const SequenceIdManager& idManager, const std::vector<wfm_handle_t*>& hs);
// the estimate from sketches that are already made: the host merge of every pair, the percentile, the adjustment
double estimate_identity_from(const GroupSketches& gs, const Parameters& params);

// One row per ordered pair (query group q, target group t), q != t, ascending (q, t) group ids -- the estimate's walk.  The counts
// come from one wfm_sketch_intersections call on h (the query groups' sketches as rows, the target groups' as columns).
std::vector<AniRow> ani_matrix_from(const GroupSketches& gs, const SequenceIdManager& idManager, wfm_handle_t* h);
// sketch_groups over hs, then ani_matrix_from on hs[0]
std::vector<AniRow> ani_matrix(const Parameters& params, const SequenceIdManager& idManager, const std::vector<wfm_handle_t*>& hs);

}  // namespace Stat
}  // namespace skch
