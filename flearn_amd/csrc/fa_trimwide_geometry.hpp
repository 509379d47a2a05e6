// fa_trimwide_geometry.hpp — the launch geometry of the wide trimmed sums (fa_trim_sum_wide,
// DESIGN.md section 19): 129 .. 1024 clients.  Host-only, on fa_geometry.hpp alone, as
// fa_quant4_geometry.hpp; plan_trim_window is unchanged.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// A column's NP slots (the smallest of 256, 512, 1024 that holds n_clients) are R = NP / 128 runs of
// kTrimWideRun slots; a thread owns one run of one column, so a block of kTrimWideThreads threads
// owns pieces of C = kTrimWideThreads / R consecutive columns and strides over the window's pieces
// by the grid.  One block per CU: its exchange buffer (every thread's run, 128 KiB) takes most of a
// CU's LDS.
constexpr int kTrimWideMaxClients = FA_TRIM_WIDE_MAX_CLIENTS;
constexpr int kTrimWideRun = 128, kTrimWideThreads = 256;

struct TrimWidePlan {
  int np;          // sort slots per column (0: n_clients outside 129 .. 1024)
  int c;           // columns per piece
  int64_t pieces;  // c-column pieces of the window
  int64_t grid;
};

inline int trim_wide_np(int n) {
  if (n <= kTrimMaxClients || n > kTrimWideMaxClients) return 0;
  int np = 2 * kTrimWideRun;
  while (np < n) np *= 2;
  return np;
}

constexpr int trim_wide_cols(int np) { return kTrimWideThreads * kTrimWideRun / np; }

inline TrimWidePlan plan_trim_wide_window(int n_clients, int64_t n_cols, int cus, int forced_grid) {
  const int np = trim_wide_np(n_clients);
  if (np == 0) return TrimWidePlan{0, 0, 0, 0};
  const int c = trim_wide_cols(np);
  const int64_t pieces = ceil_div(n_cols, c);
  int64_t grid = forced_grid > 0 ? forced_grid : (int64_t)cus;
  if (grid > pieces) grid = pieces;
  if (grid < 1) grid = 1;
  return TrimWidePlan{np, c, pieces, grid};
}

}  // namespace fa
