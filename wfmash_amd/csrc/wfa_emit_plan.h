// wfa_emit_plan.h -- how the record passes (wfa_passes.hip) cut a list of problems, tiles or rows into chunks that fit a cap: the end of
// one chunk, and for the passes that emit lists the whole plan of a call.  Host code without a device header: scripts/micro/emit_plan_check.cpp
// holds it against a linear planner.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace wfm {

// The largest kb in (ka, n] whose cost(ka, kb) fits the cap, ka + 1 at least (one problem, tile or row larger than the cap is a chunk of its
// own).  cost grows with kb.
template <class Cost>
size_t chunk_end(size_t ka, size_t n, unsigned long long cap, Cost cost) {
  size_t lo = ka + 1, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (cost(ka, mid) <= cap) lo = mid; else hi = mid - 1;
  }
  return lo;
}
inline size_t chunk_end(size_t ka, const std::vector<unsigned long long>& off, unsigned long long cap) {
  return chunk_end(ka, off.size() - 1, cap, [&](size_t a, size_t b) { return off[b] - off[a]; });
}

// The chunks of problems [0, n) in order, each chunk_end's, without those that cost nothing; widest: the largest size(ka, kb) among them
// (what one block has to hold to serve every chunk; 0 without chunks)
struct EmitPlan {
  std::vector<std::pair<size_t, size_t>> chunks;
  unsigned long long widest = 0;
};
template <class Cost, class Size>
EmitPlan emit_plan(size_t n, unsigned long long cap, Cost cost, Size size) {
  EmitPlan plan;
  for (size_t ka = 0, kb; ka < n; ka = kb) {
    kb = chunk_end(ka, n, cap, cost);
    if (cost(ka, kb) == 0) continue;
    plan.chunks.emplace_back(ka, kb);
    plan.widest = std::max<unsigned long long>(plan.widest, size(ka, kb));
  }
  return plan;
}

}  // namespace wfm
