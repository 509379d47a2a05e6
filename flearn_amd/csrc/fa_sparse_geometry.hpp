// fa_sparse_geometry.hpp — the launch geometry of the sparse ordered sum (fa_sparse_fold_f32,
// DESIGN.md section 23).  Host-only, on fa_geometry.hpp alone, as fa_mx_geometry.hpp.
#pragma once

#include "fa_geometry.hpp"
#include "flearn_amd.h"

namespace fa {

// A wave's window: kSparseWC accumulator columns in LDS (4 * WC bytes per wave), kSparseW waves per
// block.  What occupies a CU is LDS: 160 KiB hold 160 / (4 * W * WC / 1024) blocks.  FA_SPARSE_WC and
// FA_SPARSE_DEPTH rebuild the unit for the sweep (tools/bench_sparse.py --lib); the sweep is
// profiles/sparse/sweep.txt and DESIGN.md section 23 says what ships and why.
#ifndef FA_SPARSE_WC
#define FA_SPARSE_WC FA_SPARSE_WINDOW  // what ships: the header's
#endif
#ifndef FA_SPARSE_DEPTH
#define FA_SPARSE_DEPTH 8
#endif
constexpr int kSparseWC = FA_SPARSE_WC, kSparseDepth = FA_SPARSE_DEPTH, kSparseW = 4;
constexpr int kSparseLdsPerCU = 160 * 1024;
constexpr int kSparseBlocksPerCU = kSparseLdsPerCU / (4 * kSparseW * kSparseWC);
static_assert(kSparseBlocksPerCU >= 1, "a block's tiles fit a CU's LDS");
constexpr int64_t kSparseBoundsGridCap = 4096;
constexpr int64_t kSparseMaxRowPairs = (int64_t)1 << 27;   // byte offsets of a row stay far inside int32
constexpr int64_t kSparseMaxColumn = 0xFFFFFFFFll;         // columns are uint32 and 0xFFFFFFFF is the padding

struct SparsePlan {
  int64_t nwin;         // windows of kSparseWC columns
  int64_t grid;         // window_fold_kernel's blocks
  int64_t bounds_grid;  // bounds_kernel's blocks of 256 threads
};

inline int64_t sparse_windows(int64_t ncols) { return ceil_div(ncols, kSparseWC); }

// What fa_sparse_workspace returns: the bounds table, int32 [n][nwin + 1], rounded up to 16 bytes
inline int64_t sparse_workspace_bytes(int n_clients, int64_t ncols) {
  return (((int64_t)n_clients * (sparse_windows(ncols) + 1) * 4) + 15) & ~(int64_t)15;
}

// Every resident wave slot the LDS leaves gets windows (forced: fa_set_reduce_grid), never more
// blocks than there are groups of kSparseW windows.
inline SparsePlan plan_sparse_window(int n_clients, int64_t ncols, int cus, int forced = 0) {
  SparsePlan p;
  p.nwin = sparse_windows(ncols);
  p.grid = forced > 0 ? forced : (int64_t)cus * kSparseBlocksPerCU;
  const int64_t groups = ceil_div(p.nwin, kSparseW);
  if (p.grid > groups) p.grid = groups;
  if (p.grid < 1) p.grid = 1;
  p.bounds_grid = ceil_div((int64_t)n_clients * (p.nwin + 1), 256);
  if (p.bounds_grid > kSparseBoundsGridCap) p.bounds_grid = kSparseBoundsGridCap;
  return p;
}

}  // namespace fa
