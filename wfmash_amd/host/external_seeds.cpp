// external_seeds.cpp -- -K / --input-seeds (external_seeds.hpp; skch::ExternalSeeder, src/map/include/externalSeeder.hpp)
#include "external_seeds.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <map>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <unordered_set>
#include <vector>

#include "map_filter.hpp"

namespace skch {

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct PAFSeed {  // externalSeeder.hpp:34-41 (the ends it keeps are never read)
  MappingResult mapping;
  std::string queryName;
  offset_t queryLen = 0;
  std::string cigar;
};

// parsePAFLine (externalSeeder.hpp:410-490).  false: the line is skipped.  The reference's std::stoull / std::stof throw out of the
// program on a field that is not a number; such a line is skipped here like any other invalid one.
bool parse_seed(const std::string& line, const SequenceIdManager& ids, PAFSeed& s) {
  std::vector<std::string> fields;
  {
    std::stringstream ss(line);
    for (std::string f; std::getline(ss, f, '\t');) fields.push_back(f);
  }
  if (fields.size() < 12) return false;
  MappingResult& m = s.mapping;
  try {
    s.queryName = fields[0];
    s.queryLen = (offset_t)std::stoull(fields[1]);
    m.queryStartPos = (uint32_t)std::stoull(fields[2]);
    (void)std::stoull(fields[3]);  // the query end is parsed and not used: the printed end is queryStartPos + blockLength
    if (fields[4] == "+") m.setStrand(strnd::FWD);
    else if (fields[4] == "-") m.setStrand(strnd::REV);
    else return false;
    const std::string& target = fields[5];
    (void)std::stoull(fields[6]);
    m.refStartPos = (uint32_t)std::stoull(fields[7]);
    const uint64_t ref_end = std::stoull(fields[8]);
    try {
      m.refSeqId = (uint32_t)ids.getSequenceId(target);
    } catch (...) {
      std::cerr << "[wfmash::externalSeeder] Warning: Unknown target sequence '" << target << "'" << std::endl;
      return false;
    }
    m.blockLength = (uint32_t)(ref_end - m.refStartPos);  // the target span, on both axes (base_types.hpp:215-221)
    m.setNucIdentity(0.9);
    for (size_t i = 12; i < fields.size(); ++i) {
      if (fields[i].size() < 5) continue;
      const std::string tag = fields[i].substr(0, 5);
      if (tag == "dv:f:") m.setNucIdentity((float)(1.0 - std::stof(fields[i].substr(5))));
      else if (tag == "id:f:") m.setNucIdentity(std::stof(fields[i].substr(5)));
      else if (tag == "cg:Z:") s.cigar = fields[i].substr(5);
    }
  } catch (const std::logic_error&) {  // std::invalid_argument, std::out_of_range
    return false;
  }
  m.setKmerComplexity(1.0);
  m.conservedSketches = 0;
  m.n_merged = 1;
  return true;
}

// loadPAFSeeds (externalSeeder.hpp:370-408): a file warns about every line it skips, standard input does not
std::vector<PAFSeed> load_seeds(const std::string& seed_file, const SequenceIdManager& ids, uint64_t* skipped) {
  std::vector<PAFSeed> all;
  auto read = [&](std::istream& in, bool warn) {
    size_t line_no = 0;
    for (std::string line; std::getline(in, line);) {
      ++line_no;
      PAFSeed s;
      if (parse_seed(line, ids, s)) { all.push_back(std::move(s)); continue; }
      ++*skipped;
      if (warn) std::cerr << "[wfmash::externalSeeder] Warning: Skipping invalid PAF line " << line_no << std::endl;
    }
  };
  std::ifstream in;
  if (seed_file != "-") in.open(seed_file);
  if (in.is_open()) {
    read(in, true);
  } else if (seed_file == "-" || seed_file == "/dev/stdin") {
    read(std::cin, false);
  } else {
    throw std::runtime_error("Cannot open seed file " + seed_file);
  }
  return all;
}

// The reference marks a printed mapping "scaffold" when this key of its coordinates is the key of a mapping that survived the scaffold
// filter and is at least scaffold_min_length long (externalSeeder.hpp:186-197, :343-352).  The key there is std::hash<offset_t>(q) ^
// std::hash<offset_t>(r) << 1 ^ std::hash<seqno_t>(target) << 2 ^ std::hash<bool>(forward) << 3; libstdc++'s std::hash of an integer
// is the integer itself, so the key below is that hash, and what it decides -- an XOR collision included -- is the same.
size_t scaffold_key(const MappingResult& m) {
  return (size_t)(offset_t)m.queryStartPos ^ ((size_t)(offset_t)m.refStartPos << 1) ^ ((size_t)(seqno_t)m.refSeqId << 2) ^
         ((size_t)(m.strand() == strnd::FWD) << 3);
}

}  // namespace

void processExternalSeeds(const Parameters& param, const std::string& seed_file, const SequenceIdManager& idManager, std::ostream& out,
                          std::ostream* scaffold_out, SeedSummary* summary) {
  SeedSummary sum;
  double t0 = now_ms();
  std::cerr << "[wfmash::externalSeeder] Reading external seeds from " << seed_file << std::endl;
  std::vector<PAFSeed> all = load_seeds(seed_file, idManager, &sum.skipped);
  sum.seeds = all.size();
  sum.ms_read = now_ms() - t0;
  t0 = now_ms();
  if (all.empty()) {
    std::cerr << "[wfmash::externalSeeder] Warning: No valid seeds found in " << seed_file << std::endl;
    if (summary) *summary = sum;
    return;
  }
  std::cerr << "[wfmash::externalSeeder] Loaded " << all.size() << " seeds" << std::endl;
  std::map<std::string, std::vector<PAFSeed>> grouped;  // groupByQuery (:493-505)
  for (auto& s : all) grouped[s.queryName].push_back(std::move(s));
  all.clear();
  sum.queries = grouped.size();
  std::cerr << "[wfmash::externalSeeder] Processing " << grouped.size() << " query sequences" << std::endl;
  set_filter_threads(std::max(1, param.threads));

  for (const auto& [query_name, seeds] : grouped) {
    MappingResultsVector_t mappings;
    mappings.reserve(seeds.size());
    for (const auto& s : seeds) mappings.push_back(s.mapping);
    offset_t queryLen = seeds.front().queryLen;
    // the scaffold lines name the query by its id, which stays 0 (the first sequence the manager knows) for a query it does not know
    // (processExternalSeeds, :83-100; mappingFilter.hpp:925)
    seqno_t querySeqId = 0;
    try {
      querySeqId = idManager.getSequenceId(query_name);
      if (queryLen == 0) queryLen = idManager.getSequenceLength(querySeqId);
    } catch (...) {
    }

    // filterSubsetMappings of the seeder (:248-366): no chaining, seed i of the filtered vector prints as chain i+1.1.1
    MappingResultsVector_t working = mappings;
    if (param.filterMode == filter::MAP || param.filterMode == filter::ONETOONE) {
      // the query-axis sweep only, also with -o (the reference applies no reference-axis pass to external seeds)
      MappingResultsVector_t kept;
      MappingFilterUtils::filterByGroup(working, kept, param.numMappingsForSegment - 1, false, idManager, param);
      working = std::move(kept);
    }
    MappingFilterUtils::sparsifyMappings(working, param);
    std::unordered_set<size_t> scaffold_keys;
    if (param.scaffold_min_length > 0 && param.filterMode != filter::NONE) {
      MappingResultsVector_t chains;
      MappingFilterUtils::filterByScaffolds(working, param, idManager, scaffold_out ? &chains : nullptr);
      if (!chains.empty()) *scaffold_out << MappingOutput::scaffoldText(chains, idManager.getSequenceName(querySeqId), queryLen, idManager);
      for (const auto& m : working)
        if (m.blockLength >= param.scaffold_min_length) scaffold_keys.insert(scaffold_key(m));
    }

    // outputMappingsWithAnnotations (:150-246).  -M prints the seeds as they came, unfiltered, as the reference does.
    const MappingResultsVector_t& fin = param.mergeMappings ? working : mappings;
    std::vector<size_t> order(fin.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return fin[a].queryStartPos < fin[b].queryStartPos; });
    for (const size_t idx : order) {
      const MappingResult& e = fin[idx];
      const std::string* cigar = nullptr;  // the first seed of the query at the same place
      for (const auto& s : seeds)
        if (s.mapping.queryStartPos == e.queryStartPos && s.mapping.refStartPos == e.refStartPos && s.mapping.refSeqId == e.refSeqId &&
            s.mapping.strand() == e.strand()) {
          cigar = &s.cigar;
          break;
        }
      const char* st = scaffold_keys.empty() ? "" : scaffold_keys.count(scaffold_key(e)) ? "scaffold" : "rescued";
      const float fakeMapQ = e.getNucIdentity() == 1 ? 255 : std::round(-10.0 * std::log10(1 - (e.getNucIdentity())));
      out << query_name << '\t' << queryLen << '\t' << e.queryStartPos << '\t' << e.queryEndPos() << '\t' << (e.strand() == strnd::FWD ? "+" : "-")
          << '\t' << idManager.getSequenceName(e.refSeqId) << '\t' << idManager.getSequenceLength(e.refSeqId) << '\t' << e.refStartPos << '\t'
          << e.refEndPos() << '\t' << e.conservedSketches << '\t' << e.blockLength << '\t' << fakeMapQ << "\tid:f:" << e.getNucIdentity()
          << "\tkc:f:" << e.getKmerComplexity();
      if (param.mergeMappings) out << "\tch:Z:" << idx + 1 << ".1.1";
      if (cigar && !cigar->empty()) out << "\tcg:Z:" << *cigar;
      out << "\tst:Z:" << st << '\n';
      ++sum.written;
    }
  }
  set_filter_threads(1);
  out.flush();
  if (scaffold_out) scaffold_out->flush();
  sum.ms_filter = now_ms() - t0;
  std::cerr << "[wfmash::externalSeeder] External seed processing complete" << std::endl;
  if (summary) *summary = sum;
}

}  // namespace skch
