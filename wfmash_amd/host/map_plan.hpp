// map_plan.hpp -- what the map driver (mapper.cpp) decides without a device: which names take part, how the targets fall into
// subsets, where a query's fragments lie, which queries share a batch, how much room a batch's mappings get and how they are
// handed to each query's post-processing.  Plain functions over lengths and indexes: no handle, no I/O, no thread of their own
// (query_results' long form runs on the process's pool with the thread count it is given).  tests/test_map_plan_cpu.py holds
// them through wfmh_test_map_plan, scripts/micro/map_plan_check.cpp without Python.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "map_types.hpp"
#include "parallel.hpp"

namespace skch {
namespace map_plan {

constexpr int64_t kBatchBases = 256ll << 20;      // query bases per wfm_map_fragments call
constexpr int64_t kCopyBases = 64ll << 20;        // the most a batch of several sequences copies (see plan_batch)
constexpr int64_t kDefaultSubsetBases = 5000000;  // createTargetSubsets without --index-by (computeMap.hpp:295-327)
constexpr size_t kEarlyFilterFrags = (size_t)1 << 16;  // a single query of this many fragments: its filter thread starts before it is mapped
constexpr size_t kSpareMappings = (size_t)1 << 17;     // a single query of this many mappings: reused vector, fill on several threads

// names as Map's constructor selects them (computeMap.hpp:162-190): all without a prefix, else those that begin with one of them
inline std::vector<std::string> select_by_prefix(const std::vector<std::string>& names, const std::vector<std::string>& prefixes) {
  std::vector<std::string> out;
  for (const auto& n : names) {
    bool ok = prefixes.empty();
    for (const auto& pre : prefixes) ok = ok || n.compare(0, pre.size(), pre) == 0;
    if (ok) out.push_back(n);
  }
  return out;
}

// createTargetSubsets (computeMap.hpp:295-327): names in order, a subset is closed once it holds `batch` bases or more
inline std::vector<std::vector<std::string>> target_subsets(const std::vector<std::string>& names, const std::vector<int64_t>& lengths, int64_t batch) {
  std::vector<std::vector<std::string>> subsets;
  std::vector<std::string> cur;
  uint64_t cur_size = 0;
  for (size_t i = 0; i < names.size(); ++i) {
    cur.push_back(names[i]);
    cur_size += (uint64_t)lengths[i];
    if (cur_size >= (uint64_t)batch || i + 1 == names.size()) { subsets.push_back(cur); cur.clear(); cur_size = 0; }
  }
  return subsets;
}

// one query of a batch: sequence `qi` of the run's queries at `base` of the batch's bases, fragments [first_frag, first_frag + nfrag)
struct BatchQuery { size_t qi; seqno_t id; offset_t len; int64_t base; int64_t first_frag; int nfrag; };

// a query's fragments (computeMap.hpp:560-631): len / w whole windows, one more anchored at the end when len is no multiple
// of w and there is a whole one, none for len < w; offsets count from the batch's first base
struct FragLayout { int64_t first_frag; int nfrag; std::vector<int64_t> offsets; };
inline FragLayout layout_fragments(int64_t len, int64_t w, int64_t base, int64_t first_frag) {
  FragLayout fl{first_frag, 0, {}};
  const int whole = (int)(len / w);
  for (int i = 0; i < whole; ++i) fl.offsets.push_back(base + (int64_t)i * w);
  if (whole >= 1 && len % w != 0) fl.offsets.push_back(base + len - w);  // anchored at the end
  fl.nfrag = (int)fl.offsets.size();
  return fl;
}

// The next batch of whole query sequences from position `qi` of the run's queries, by their lengths (<= 0: not found or empty,
// "skipping", computeMap.hpp:534-537 -- consumed, never a member): until batch_bases is reached, at least one.
// (a batch of ONE sequence is mapped where the FASTA store holds it; a second one makes the batch a copy of both.  For chromosome-sized
// queries that copy -- 2 x 249 MB into fresh pages, on the device thread, before every batch of the all-vs-all job -- was 170 ms per batch
// beside 150 ms of mapping: a sequence that would push the copy past kCopyBases begins a batch of its own)
struct BatchPlan {
  std::vector<size_t> members;  // indexes into the run's queries, ascending
  size_t next = 0;              // where the batch after this one begins
  int64_t n_bases = 0;
  bool in_place = false;        // one sequence: mapped where it lies; several: laid end to end in a buffer
};
inline BatchPlan plan_batch(const int64_t* lengths, size_t n, size_t qi, int64_t batch_bases) {
  BatchPlan p;
  while (qi < n && (p.n_bases < batch_bases || p.members.empty())) {
    const int64_t len = lengths[qi];
    if (len <= 0) { ++qi; continue; }
    if (!p.members.empty() && p.n_bases + len > kCopyBases) break;
    p.members.push_back(qi++);
    p.n_bases += len;
  }
  p.next = qi;
  p.in_place = p.members.size() == 1;
  return p;
}

// several devices: batches small enough that every device gets a few
inline int64_t batch_bases_for(size_t n_handles, uint64_t query_bp) {
  if (n_handles <= 1) return kBatchBases;
  return std::max<int64_t>(1, std::min<int64_t>(kBatchBases, (int64_t)(query_bp / (2 * n_handles))));
}

// room for a batch's mappings: a fragment of a pangenome maps about once per target haplotype; a too small buffer costs a
// second pass over the batch, so be generous
inline int64_t mapping_cap(int64_t nfrag, int64_t subset_size) {
  return nfrag * std::min<int64_t>(256, std::max<int64_t>(16, 2 * subset_size)) + (1 << 16);
}

// what a chromosome-sized query's result vector will about hold
// (a pangenome's fragment maps about once per target sequence of another group: one per target sequence is room enough; a vector that
// turns out too small grows as any vector does)
inline size_t spare_hint(size_t nfrag, int64_t subset_size) { return nfrag * (size_t)std::min<int64_t>(16, std::max<int64_t>(1, subset_size)); }

// first_map[qn] = the first of a batch's n mappings (grouped by fragment, mfrag ascending) that belongs to query qn; [nq] = n
inline std::vector<size_t> split_by_query(const int32_t* mfrag, size_t n, const std::vector<BatchQuery>& bq) {
  std::vector<size_t> first_map(bq.size() + 1, n);
  size_t m = 0;
  for (size_t qn = 0; qn < bq.size(); ++qn) {
    first_map[qn] = m;
    while (m < n && mfrag[m] < bq[qn].first_frag + bq[qn].nfrag) ++m;
  }
  return first_map;
}

// a device mapping as the filters take it: queryStartPos += fragmentIndex * windowLength, also for the anchored one (computeMap.hpp:124-128)
inline MappingResult to_result(const wfm_mapping_t& map, int32_t mfrag, int64_t first_frag, int64_t w) {
  MappingResult r;
  std::memcpy((void*)&r, &map, sizeof(r));
  r.queryStartPos += (uint32_t)((mfrag - first_frag) * w);
  return r;
}

// The mappings [m0, m0 + nq) of one query into `out`.  perm (null: none) is the batch's permutation into chaining order
// (wfm_map_fragments_ordered; its queries are consecutive there as here), taken for nq >= 2 unless perm[0] = ~0u: out is then in that
// order and orig[i] = the position out[i] had in fragment order, within the query.  Otherwise, and when an entry of the permutation
// leaves the query (a permutation that mixes queries would be a bug: sort on the host then), out is in fragment order and orig empty.
// A query of kSpareMappings or more is filled by up to `threads` threads of the process's pool.
inline void query_results(const wfm_mapping_t* maps, const int32_t* mfrag, const uint32_t* perm, size_t m0, size_t nq, int64_t first_frag, int64_t w,
                          MappingResultsVector_t& out, std::vector<uint32_t>& orig, int threads) {
  orig.clear();
  if (!(perm && perm[0] != 0xffffffffu && nq >= 2)) {
    out.clear();
    out.reserve(nq);
    for (size_t m = m0; m < m0 + nq; ++m) out.push_back(to_result(maps[m], mfrag[m], first_frag, w));
    return;
  }
  out.resize(nq);
  orig.resize(nq);
  std::atomic<bool> inside{true};
  const size_t T = nq >= kSpareMappings ? (size_t)std::max(1, threads) : 1;
  wfmash_host::parallel_for(T, (int)T, [&](size_t t) {
    for (size_t i = nq * t / T; i < nq * (t + 1) / T; ++i) {
      const size_t m = perm[m0 + i];
      if (m < m0 || m - m0 >= nq) { inside.store(false); continue; }
      out[i] = to_result(maps[m], mfrag[m], first_frag, w);
      orig[i] = (uint32_t)(m - m0);
    }
  });
  if (!inside.load()) {
    for (size_t i = 0; i < nq; ++i) out[i] = to_result(maps[m0 + i], mfrag[m0 + i], first_frag, w);
    orig.clear();
  }
}

}  // namespace map_plan
}  // namespace skch
