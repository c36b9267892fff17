// map_isect.hip -- wfm_sketch_intersections: the multiset intersection sizes of all (row sketch, column sketch) pairs of a set of
// ascending MinHash sketches, the counts the ANI table is made of (estimate_identity_for_groups' pairwise merge,
// map_stats.hpp:719-731, for every pair at once).
//
// The two-pointer merge of two ascending multisets A and B counts sum over v of min(count of v in A, count of v in B).  Element by
// element: A[i] is counted iff B holds at least as many copies of its value as A holds up to and including i, that is iff
//   p = lbB(A[i]) + (i - lbA(A[i]))  lies inside B  and  B[p] == A[i]
// with lbX(v) the first index of v in X.  Every element of A decides on its own: one lane per element, no order between lanes.
//
// isect_kernel: one workgroup (kIsectThreads lanes) owns one column sketch B and kIsectRows row sketches and writes those cells
// itself; nothing is shared between workgroups.  B is loaded once into LDS when it holds at most WFM_ISECT_LDS_MAX hashes (32 KB,
// static: four workgroups per CU by LDS) and searched there with 8-byte reads; a longer B is searched where it lies in global
// memory (it stays in L2 while the workgroups of its column run).  A streams from global memory, lane l reading element
// base + l (coalesced 8-byte loads).  The rank i - lbA(A[i]) is 0 whenever A[i - 1] differs, which one more (cached) load
// tells; inside a run of equal values it is a binary search of A[0, i), never a walk: a run may span the whole sketch.  The
// binary search of B starts on one address for all lanes (a broadcast) and fans out by halves; its last steps touch
// neighbouring slots, because neighbouring lanes carry neighbouring values of an ascending A.  No padding of the LDS image
// changes which banks a search meets, so the image is plain.  Counts are summed per wave by shuffles, per workgroup through
// LDS.
//
// isect_ascending_kernel: the check that every sketch ascends, one pass over the hashes before any intersection runs; a
// descent between two neighbours is an error unless the second one begins another sketch, and the lowest offending sketch wins.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../../include/wfmash_hip.h"
#include "map_device.h"
#include "map_isect_args.h"

#define HIPCHK(h, call)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      wfm_set_error((h), std::string(#call) + ": " + hipGetErrorString(e_));            \
      return e_ == hipErrorOutOfMemory ? WFM_E_NOMEM : WFM_E_HIP;                       \
    }                                                                                   \
  } while (0)

namespace {

constexpr int kIsectThreads = 256;
constexpr int kIsectRows = 8;                        // row sketches per workgroup: the column's load is paid once for them
constexpr int64_t kIsectCells = (int64_t)64 << 20;   // cells of one launch: the device output buffer is at most 256 MB

// first index in a[0, n) whose value is not below v
template <typename Ptr, typename Idx>
__device__ __forceinline__ Idx isect_lower_bound(Ptr a, Idx n, uint64_t v) {
  Idx lo = 0;
  while (n > 0) {
    const Idx half = n >> 1;
    if (a[lo + half] < v) { lo += half + 1; n -= half + 1; }
    else n = half;
  }
  return lo;
}

__global__ __launch_bounds__(kIsectThreads) void isect_kernel(const uint64_t* __restrict__ hashes, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int64_t n_rows,
                                                              int64_t n_cols, uint32_t* __restrict__ out /* n_rows x n_cols */) {
  __shared__ uint64_t s_b[WFM_ISECT_LDS_MAX];
  __shared__ uint32_t s_part[kIsectThreads / 64];
  const int tid = (int)threadIdx.x;
  const int64_t row_groups = (n_rows + kIsectRows - 1) / kIsectRows;
  const int64_t c = (int64_t)blockIdx.x / row_groups, rg = (int64_t)blockIdx.x % row_groups;
  if (c >= n_cols) return;
  const int64_t b0 = offsets[cols[c]], nb = offsets[cols[c] + 1] - b0;
  const uint64_t* __restrict__ gb = hashes + b0;
  const bool in_lds = nb <= WFM_ISECT_LDS_MAX;
  if (in_lds) {
    for (int i = tid; i < (int)nb; i += kIsectThreads) s_b[i] = gb[i];
    __syncthreads();
  }
  const int64_t r_end = (rg + 1) * kIsectRows < n_rows ? (rg + 1) * kIsectRows : n_rows;
  for (int64_t r = rg * kIsectRows; r < r_end; ++r) {
    const int64_t a0 = offsets[rows[r]], na = offsets[rows[r] + 1] - a0;
    const uint64_t* __restrict__ ga = hashes + a0;
    uint32_t count = 0;
    if (nb > 0) {
      for (int64_t i = tid; i < na; i += kIsectThreads) {
        const uint64_t v = ga[i];
        int64_t rank = 0;  // copies of v in A before i
        if (i > 0 && ga[i - 1] == v) rank = i - isect_lower_bound(ga, i, v);
        if (in_lds) {
          const int64_t p = (int64_t)isect_lower_bound(s_b, (int)nb, v) + rank;
          if (p < nb && s_b[p] == v) ++count;
        } else {
          const int64_t p = isect_lower_bound(gb, nb, v) + rank;
          if (p < nb && gb[p] == v) ++count;
        }
      }
    }
    for (int d = 32; d > 0; d >>= 1) count += __shfl_down(count, d, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
      uint32_t total = 0;
      for (int w = 0; w < kIsectThreads / 64; ++w) total += s_part[w];
      out[r * n_cols + c] = total;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void isect_ascending_kernel(const uint64_t* __restrict__ hashes, int64_t total, const int64_t* __restrict__ offsets,
                                                              int64_t n_sketches, unsigned long long* first_bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < total; i += stride) {
    if (hashes[i] <= hashes[i + 1]) continue;
    // the sketch that holds i: the last s with offsets[s] <= i (empty sketches before it share its offset and come earlier)
    int64_t lo = 0, n = n_sketches + 1;
    while (n > 0) {
      const int64_t half = n >> 1;
      if (offsets[lo + half] <= i) { lo += half + 1; n -= half + 1; }
      else n = half;
    }
    const int64_t s = lo - 1;
    if (s >= 0 && s < n_sketches && i + 1 < offsets[s + 1]) atomicMin(first_bad, (unsigned long long)s);
  }
}

}  // namespace

extern "C" int wfm_sketch_intersections(wfm_handle_t* h, const uint64_t* hashes, const int64_t* offsets, int64_t n_sketches, const int32_t* rows,
                                        int64_t n_rows, const int32_t* cols, int64_t n_cols, uint32_t* shared) {
  if (!h) return WFM_E_ARG;
  const std::string bad = wfm::isect_check_args(offsets, n_sketches, rows, n_rows, cols, n_cols);
  if (!bad.empty()) { wfm_set_error(h, "wfm_sketch_intersections: " + bad); return WFM_E_ARG; }
  if (n_rows == 0 || n_cols == 0) return WFM_OK;
  const int64_t total = offsets[n_sketches];
  if ((total > 0 && !hashes) || !shared) { wfm_set_error(h, "wfm_sketch_intersections: hashes or shared is NULL"); return WFM_E_ARG; }
  int64_t max_cells = kIsectCells;
  if (const char* e = getenv("WFM_ISECT_CELLS")) {  // read per call: a test switch, small values make a small matrix take many launches
    const long long v = atoll(e);
    if (v >= 1) max_cells = v;
  }
  const wfm::IsectCut cut = wfm::isect_cut(n_rows, n_cols, max_cells);

  HIPCHK(h, hipSetDevice(wfm_device(h)));
  hipStream_t st = wfm_stream(h);
  MapScratch sc;
  uint64_t* d_hashes = nullptr; int64_t* d_offsets = nullptr; int32_t *d_rows = nullptr, *d_cols = nullptr;
  uint32_t* d_out = nullptr; unsigned long long* d_bad = nullptr;
  HIPCHK(h, sc.alloc(&d_hashes, (size_t)total));
  HIPCHK(h, sc.alloc(&d_offsets, (size_t)n_sketches + 1));
  HIPCHK(h, sc.alloc(&d_rows, (size_t)n_rows));
  HIPCHK(h, sc.alloc(&d_cols, (size_t)n_cols));
  HIPCHK(h, sc.alloc(&d_out, (size_t)cut.rows * (size_t)cut.cols));
  HIPCHK(h, sc.alloc(&d_bad, 1));
  if (total) HIPCHK(h, hipMemcpyAsync(d_hashes, hashes, (size_t)total * 8, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_offsets, offsets, ((size_t)n_sketches + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_rows, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_cols, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
  if (total > 1) {
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(isect_ascending_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_hashes, total, d_offsets, n_sketches, d_bad);
    HIPCHK(h, hipGetLastError());
  }
  unsigned long long first_bad = ~0ull;
  HIPCHK(h, hipMemcpyAsync(&first_bad, d_bad, sizeof(first_bad), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (first_bad != ~0ull) {
    wfm_set_error(h, "wfm_sketch_intersections: sketch " + std::to_string(first_bad) + " is not ascending");
    return WFM_E_ARG;
  }
  for (int64_t r0 = 0; r0 < n_rows; r0 += cut.rows) {
    const int64_t nr = std::min(cut.rows, n_rows - r0);
    for (int64_t c0 = 0; c0 < n_cols; c0 += cut.cols) {
      const int64_t nc = std::min(cut.cols, n_cols - c0);
      const int64_t blocks = nc * ((nr + kIsectRows - 1) / kIsectRows);  // <= nr * nc <= max(max_cells, one cell)
      if (blocks > 0x7fffffffll) { wfm_set_error(h, "wfm_sketch_intersections: WFM_ISECT_CELLS is too large"); return WFM_E_ARG; }
      hipLaunchKernelGGL(isect_kernel, dim3((unsigned)blocks), dim3(kIsectThreads), 0, st, d_hashes, d_offsets, d_rows + r0, d_cols + c0, nr, nc, d_out);
      HIPCHK(h, hipGetLastError());
      uint32_t* dst = shared + r0 * n_cols + c0;
      if (nc == n_cols) HIPCHK(h, hipMemcpyAsync(dst, d_out, (size_t)nr * (size_t)nc * 4, hipMemcpyDeviceToHost, st));
      else HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)n_cols * 4, d_out, (size_t)nc * 4, (size_t)nc * 4, (size_t)nr, hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));  // d_out is written again by the next launch
    }
  }
  return WFM_OK;
}
