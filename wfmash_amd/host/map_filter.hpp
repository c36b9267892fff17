// map_filter.hpp -- post-processing of a query's L2 mappings, host side.
//
// Restates, with the reference's integer/float behaviour and libstdc++ container semantics:
//   skch::Filter::query::filterMappings / ref::filterMappings   src/map/include/filter.hpp:172-235, :471-535
//   MappingFilterUtils::{filterWeakMappings :154, filterFalseHighIdentity :184, sparsifyMappings :203,
//     filterByGroup :220, mergeMappingsInRangeWithChains :382, mergeMappingsInRange :580,
//     filterByScaffolds :831}                                     src/map/include/mappingFilter.hpp
//   Map::filterSubsetMappings                                    src/map/include/computeMap.hpp:1076-1165
//   MappingOutput::{mappingBoundarySanityCheck :31, reportReadMappings :74}   src/map/include/mappingOutput.hpp
// This stage is serial per query in the reference and stays on the host; the GPU produces its input.
#pragma once

#include <ostream>
#include <string>

#include "map_types.hpp"
#include "sequence_ids.hpp"

namespace skch {

namespace Filter {
namespace query {
// plane sweep over the query axis: keeps, at every query position, the best-scoring mappings
void filterMappings(MappingResultsVector_t& readMappings, int secondaryToKeep, bool dropRand, double overlapThreshold);
}  // namespace query
namespace ref {
// plane sweep over the concatenated reference axis (one-to-one mode)
void filterMappings(MappingResultsVector_t& readMappings, const SequenceIdManager& idManager, uint16_t secondaryToKeep, bool dropRand,
                    double overlapThreshold);
}  // namespace ref
}  // namespace Filter

class MappingFilterUtils {
 public:
  static void filterWeakMappings(MappingResultsVector_t& readMappings, int64_t min_count, const Parameters& param,
                                 const SequenceIdManager& idManager, offset_t queryLen);
  static void filterFalseHighIdentity(MappingResultsVector_t& readMappings, const Parameters& param);
  static void sparsifyMappings(MappingResultsVector_t& readMappings, const Parameters& param);
  static void filterByGroup(MappingResultsVector_t& unfilteredMappings, MappingResultsVector_t& filteredMappings, int n_mappings,
                            bool filter_ref, const SequenceIdManager& idManager, const Parameters& param);
  static MappingsWithChains mergeMappingsInRangeWithChains(MappingResultsVector_t& readMappings, int max_dist, const Parameters& param,
                                                           const uint32_t* presorted_orig = nullptr);
  static MappingResultsVector_t mergeMappingsInRange(MappingResultsVector_t& readMappings, int max_dist, const Parameters& param);
  // chains_out (optional): receives the scaffold chains the reference writes to --scaffold-out (mappingFilter.hpp:911-945) --
  // the chains after the length cut and their own sweep, and only when anchors were found
  static void filterByScaffolds(MappingResultsVector_t& readMappings, const Parameters& param, const SequenceIdManager& idManager,
                                MappingResultsVector_t* chains_out = nullptr);
};

struct FilteredMappingsResult {
  MappingResultsVector_t nonMergedMappings, mergedMappings;
  ChainInfoVector_t nonMergedChainInfo, mergedChainInfo;
  MappingResultsVector_t scaffoldChains;  // filled only when param.scaffold_output_file is set
};
// host threads the CALLING thread may use inside filterSubsetMappings (default 1): a batch with a single long query
void set_filter_threads(int threads);

// Map::filterSubsetMappings: everything between a query's raw L2 mappings and what is printed.
// presorted_orig (f3, first step; null: none): the caller built `mappings` in chaining order from the device's permutation
// (wfm_map_fragments_ordered); presorted_orig[i] = mapping i's position in the reference's input order (fragment order), one entry per
// mapping.  It goes to the first chaining call only, which checks the order, skips its own sort if it holds and undoes it if not; it is
// read during this call alone.
FilteredMappingsResult filterSubsetMappings(MappingResultsVector_t& mappings, const Parameters& param, const SequenceIdManager& idManager,
                                            offset_t queryLen, const uint32_t* presorted_orig = nullptr);

class MappingOutput {
 public:
  static void mappingBoundarySanityCheck(offset_t queryLen, MappingResultsVector_t& readMappings, const SequenceIdManager& idManager);
  static void reportReadMappings(MappingResultsVector_t& readMappings, const ChainInfoVector_t& chainInfo, const std::string& queryName,
                                 std::ostream& outstrm, const SequenceIdManager& idManager, const Parameters& param, offset_t queryLen);
  static void reportReadMappings(MappingResultsVector_t& readMappings, const std::string& queryName, std::ostream& outstrm,
                                 const SequenceIdManager& idManager, const Parameters& param, offset_t queryLen);
  // the --scaffold-out lines of one query's scaffold chains (mappingFilter.hpp:925-941)
  static std::string scaffoldText(const MappingResultsVector_t& chains, const std::string& queryName, offset_t queryLen,
                                  const SequenceIdManager& idManager);
};

}  // namespace skch
