// external_seeds.hpp -- -K / --input-seeds: PAF records of another tool (FastGA, minimap2, ...) in place of the MinHash mapper,
// restating skch::ExternalSeeder (src/map/include/externalSeeder.hpp) on top of the filters of map_filter.hpp.
//
//   parse    externalSeeder.hpp:370-490   tab fields, >= 12 of them, strand + or -, a known target; blockLength = tend - tstart;
//                                         identity 0.9 unless dv:f: (1 - dv) or id:f: (the later tag wins); kc 1, conserved 0
//   group    :54-130, :490-505            by query name in std::map order; the query length from column 2 (the id manager's when 0)
//   filter   :248-366                     no chaining (seed i is chain i.1.1), filterByGroup, sparsifyMappings, filterByScaffolds
//   output   :150-246                     by query start; id, kc, ch (merging on), cg (the seed's), st:Z:scaffold|rescued
// Host only: none of these stages reads the identity threshold or the sketch size (filterFalseHighIdentity, the one filter that reads
// percentageIdentity, is not part of the seeder's sequence), so the identity estimate the reference runs first is not run here.
#pragma once

#include <cstdint>
#include <ostream>
#include <string>

#include "map_types.hpp"
#include "sequence_ids.hpp"

namespace skch {

struct SeedSummary {
  uint64_t seeds = 0;     // seed records read
  uint64_t skipped = 0;   // lines skipped (too few fields, bad strand, unknown target, a number that does not parse)
  uint64_t queries = 0;   // query groups
  uint64_t written = 0;   // mapping records written
  double ms_read = 0, ms_filter = 0;
};

// ExternalSeeder::processExternalSeeds.  seed_file "-" (or an unreadable "/dev/stdin") reads standard input.  scaffold_out (may be
// NULL): receives the scaffold chains of every query (param.scaffold_output_file names it; the caller opens it).  Throws
// std::runtime_error when the seed file cannot be opened.
void processExternalSeeds(const Parameters& param, const std::string& seed_file, const SequenceIdManager& idManager, std::ostream& out,
                          std::ostream* scaffold_out, SeedSummary* summary);

}  // namespace skch
