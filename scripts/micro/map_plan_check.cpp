// map_plan_check.cpp -- the map driver's planner (wfmash_amd/host/map_plan.hpp) on random inputs, for the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread scripts/micro/map_plan_check.cpp -o map_plan_asan && ./map_plan_asan
//
// Over random length lists: a query's fragments cover [0, len) and none passes its end; the batches partition the queries that have
// bases, in order, and a copied batch stays within kCopyBases; the subsets partition the targets and all but the last reach the
// batch size; split_by_query and query_results give back every mapping of a query once, in the permutation's order or in fragment
// order.  Exit status 0 = all held.
#include <cstdio>
#include <numeric>
#include <random>

#include "../../wfmash_amd/host/map_plan.hpp"

namespace mp = skch::map_plan;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s (list %ld)\n", __FILE__, __LINE__, #c, it); return 1; } } while (0)

int main() {
  std::mt19937_64 rng(2026);
  auto below = [&](uint64_t n) { return (int64_t)(rng() % n); };
  long fragments = 0, batches = 0, mappings = 0, it = 0;
  for (it = 0; it < 4000; ++it) {
    const int64_t windows[] = {16, 100, 1000};
    const int64_t w = windows[below(3)];
    std::vector<int64_t> len((size_t)below(14));
    for (auto& l : len) l = below(5) == 0 ? 0 : 1 + below(12 * w);
    if (it % 40 == 0 && !len.empty()) len[(size_t)below(len.size())] = mp::kCopyBases - below(3 * w);

    // fragments
    for (int64_t l : len) {
      if (l > (1 << 20)) continue;
      const mp::FragLayout fl = mp::layout_fragments(l, w, 7, 3);
      CHECK(fl.first_frag == 3 && fl.nfrag == (int)fl.offsets.size() && fl.nfrag == (l < w ? 0 : l / w + (l % w != 0)));
      std::vector<char> covered((size_t)l, 0);
      for (int64_t o : fl.offsets) {
        CHECK(o - 7 >= 0 && o - 7 + w <= l);
        for (int64_t i = o - 7; i < o - 7 + w; ++i) covered[(size_t)i] = 1;
      }
      if (l >= w) for (char c : covered) CHECK(c);
      fragments += fl.nfrag;
    }

    // batches
    const int64_t sizes[] = {1, 3 * w, 20 * w, mp::kBatchBases};
    const int64_t batch_bases = sizes[below(4)];
    std::vector<size_t> seen;
    for (size_t qi = 0;;) {
      const mp::BatchPlan p = mp::plan_batch(len.data(), len.size(), qi, batch_bases);
      if (p.members.empty()) { CHECK(p.next == len.size()); break; }
      CHECK(p.next > qi && p.in_place == (p.members.size() == 1));
      int64_t bases = 0;
      for (size_t m : p.members) { CHECK(m >= qi && m < p.next && len[m] > 0); bases += len[m]; seen.push_back(m); }
      CHECK(bases == p.n_bases && (p.in_place || bases <= mp::kCopyBases));
      CHECK(bases - len[p.members.back()] < batch_bases);  // it was not yet full when the last one came
      qi = p.next;
      ++batches;
    }
    size_t k = 0;
    for (size_t i = 0; i < len.size(); ++i) if (len[i] > 0) { CHECK(k < seen.size() && seen[k] == i); ++k; }
    CHECK(k == seen.size());

    // subsets
    std::vector<std::string> names;
    for (size_t i = 0; i < len.size(); ++i) names.push_back("t" + std::to_string(i));
    const int64_t subset_bases = 1 + below(30 * w);
    const auto subsets = mp::target_subsets(names, len, subset_bases);
    size_t at = 0;
    for (size_t s = 0; s < subsets.size(); ++s) {
      int64_t bases = 0;
      CHECK(!subsets[s].empty());
      for (const auto& n : subsets[s]) { CHECK(n == names[at]); bases += len[at++]; }
      CHECK(s + 1 == subsets.size() || (bases >= subset_bases && bases - len[at - 1] < subset_bases));
    }
    CHECK(at == names.size());

    // a batch's mappings by query, and each query's vector from a permutation that stays inside it
    std::vector<mp::BatchQuery> bq;
    int64_t nfrag = 0;
    for (size_t i = 0; i < len.size() && len[i] <= (1 << 20); ++i) {
      const int nf = mp::layout_fragments(len[i], w, 0, nfrag).nfrag;
      bq.push_back({i, (skch::seqno_t)i, len[i], 0, nfrag, nf});
      nfrag += nf;
    }
    std::vector<wfm_mapping_t> maps;
    std::vector<int32_t> mfrag;
    for (int64_t f = 0; f < nfrag; ++f)
      for (int64_t c = below(4); c > 0; --c) { wfm_mapping_t m{}; m.refStartPos = (uint32_t)maps.size(); m.queryStartPos = (uint32_t)below(w); maps.push_back(m); mfrag.push_back((int32_t)f); }
    const std::vector<size_t> first = mp::split_by_query(mfrag.data(), maps.size(), bq);
    CHECK(first.size() == bq.size() + 1 && first.back() == maps.size());
    std::vector<uint32_t> perm(maps.size());
    std::iota(perm.begin(), perm.end(), 0u);
    for (size_t q = 0; q < bq.size(); ++q) std::shuffle(perm.begin() + (long)first[q], perm.begin() + (long)first[q + 1], rng);
    const bool mixes = maps.size() >= 2 && below(4) == 0;  // sometimes a permutation that leaves its query
    if (mixes) std::swap(perm.front(), perm.back());
    for (size_t q = 0; q < bq.size(); ++q) {
      const size_t m0 = first[q], nq = first[q + 1] - first[q];
      for (size_t m = m0; m < m0 + nq; ++m) CHECK(mfrag[m] >= bq[q].first_frag && mfrag[m] < bq[q].first_frag + bq[q].nfrag);
      skch::MappingResultsVector_t out(5);
      std::vector<uint32_t> orig(1);
      mp::query_results(maps.data(), mfrag.data(), perm.data(), m0, nq, bq[q].first_frag, w, out, orig, 4);
      CHECK(out.size() == nq && (orig.empty() || orig.size() == nq));
      CHECK(mixes || nq < 2 || orig.size() == nq);  // a sound order is taken
      for (size_t i = 0; i < nq; ++i) {
        const size_t m = orig.empty() ? m0 + i : m0 + orig[i];
        CHECK(orig.empty() || perm[m0 + i] == m);
        CHECK(out[i].refStartPos == m && out[i].queryStartPos == maps[m].queryStartPos + (uint32_t)((mfrag[m] - bq[q].first_frag) * w));
      }
      mappings += (long)nq;
    }
  }
  CHECK(mp::batch_bases_for(1, 5) == mp::kBatchBases && mp::batch_bases_for(2, 3) == 1 && mp::batch_bases_for(2, 4000) == 1000);
  CHECK(mp::select_by_prefix({"A#1", "B#1", "AB"}, {}).size() == 3 && mp::select_by_prefix({"A#1", "B#1", "AB"}, {"A"}).size() == 2);
  CHECK((mp::select_by_prefix({"A#1", "B#1", "AB"}, {"B", "AB"}) == std::vector<std::string>{"B#1", "AB"}));
  printf("map_plan_check: ok, %ld lists: %ld fragments, %ld batches, %ld mappings\n", it, fragments, batches, mappings);
  return 0;
}
