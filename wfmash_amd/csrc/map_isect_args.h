// map_isect_args.h -- what wfm_sketch_intersections (map_isect.hip) decides before anything touches the device: the checks of its
// CSR arguments and the cut of the matrix into launches.  Plain C++, no HIP: scripts/micro/ani_rows_check.cpp builds it on its own.
#ifndef WFM_MAP_ISECT_ARGS_H_
#define WFM_MAP_ISECT_ARGS_H_
#include <stdint.h>

#include <string>

namespace wfm {

// Empty string: the arguments are good.  Otherwise the message of the WFM_E_ARG the call returns.  offsets has n_sketches + 1
// entries; nothing is read beyond offsets[n_sketches], rows[n_rows - 1], cols[n_cols - 1].
inline std::string isect_check_args(const int64_t* offsets, int64_t n_sketches, const int32_t* rows, int64_t n_rows, const int32_t* cols,
                                    int64_t n_cols) {
  if (n_sketches < 0 || n_rows < 0 || n_cols < 0) return "negative count";
  if (!offsets) return "offsets is NULL";
  if ((n_rows && !rows) || (n_cols && !cols)) return "rows or cols is NULL";
  if (offsets[0] != 0) return "offsets[0] must be 0, got " + std::to_string(offsets[0]);
  for (int64_t i = 0; i < n_sketches; ++i) {
    if (offsets[i + 1] < offsets[i])
      return "offsets decrease at sketch " + std::to_string(i) + " (" + std::to_string(offsets[i]) + " > " + std::to_string(offsets[i + 1]) + ")";
    if (offsets[i + 1] - offsets[i] > (int64_t)0xffffffffll)  // a count is 32 bits wide
      return "sketch " + std::to_string(i) + " holds more than 2^32 - 1 hashes";
  }
  for (int64_t i = 0; i < n_rows; ++i)
    if (rows[i] < 0 || rows[i] >= n_sketches)
      return "rows[" + std::to_string(i) + "] = " + std::to_string(rows[i]) + " is outside [0, " + std::to_string(n_sketches) + ")";
  for (int64_t i = 0; i < n_cols; ++i)
    if (cols[i] < 0 || cols[i] >= n_sketches)
      return "cols[" + std::to_string(i) + "] = " + std::to_string(cols[i]) + " is outside [0, " + std::to_string(n_sketches) + ")";
  return std::string();
}

// One launch covers rows [r0, r0 + rows) x columns [c0, c0 + cols) with rows * cols <= max_cells (max_cells >= 1): whole rows
// where a row fits, otherwise a single row in pieces of max_cells columns.
struct IsectCut { int64_t rows, cols; };
inline IsectCut isect_cut(int64_t n_rows, int64_t n_cols, int64_t max_cells) {
  if (max_cells < 1) max_cells = 1;
  IsectCut c;
  c.cols = n_cols < max_cells ? n_cols : max_cells;
  c.rows = c.cols > 0 ? max_cells / c.cols : 0;
  if (c.rows > n_rows) c.rows = n_rows;
  if (c.rows < 1 && n_rows > 0 && n_cols > 0) c.rows = 1;
  return c;
}

}  // namespace wfm
#endif
