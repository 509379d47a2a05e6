// fa_gramwide_geometry.hpp — the launch geometry of the wide client Gram matrix (fa_gram_f32_wide,
// DESIGN.md section 24): 129 .. 1024 clients.  Host-only, on fa_geometry.hpp alone, as
// fa_trimwide_geometry.hpp; plan_gram_window is unchanged.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// The clients' rows are padded to whole 32-row MFMA tiles and grouped into R = ceil(n / 128) panels
// of kGramWidePanel rows; G is symmetric, so only the R (R + 1) / 2 panel pairs (I <= J) are
// computed, numbered (0,0), (0,1), ..., (0,R-1), (1,1), ...  The window is cut into chunks of
// kGramWideKc columns (one LDS fill) and the chunks into `slices` contiguous shares (slice s:
// chunks [s * chunks / slices, (s + 1) * chunks / slices)); a block of 256 threads owns one
// (slice, pair) unit and stores its [128][128] fp32 partial to workspace slot slice * pairs + pair.
// The natural slice count fills kGramWideRounds rounds of one block per CU; a launch never has more
// than kGramWideUnitCap units, which is what the workspace is sized for on any device.  chain: as
// plan_gram_window's, the longest sequence of fp32 roundings behind one entry of a partial.
constexpr int kGramWideMaxClients = FA_GRAM_WIDE_MAX_CLIENTS;
constexpr int kGramWidePanel = 128;
constexpr int kGramWideKc = 64;
constexpr int kGramWideRounds = 4;
constexpr int kGramWideUnitCap = 2048;
constexpr int64_t kGramWideSlotBytes = (int64_t)kGramWidePanel * kGramWidePanel * 4;

struct GramWidePlan {
  int tiles;        // 32-row tiles of the padded rows (0: n_clients out of range)
  int panels;       // R
  int pairs;        // R (R + 1) / 2
  int kc;           // columns per LDS chunk
  int lc;           // columns per inner chain
  int64_t chunks;   // Kc-column chunks of the window
  int64_t slices;   // column shares; the grid is slices * pairs blocks
  int64_t share;    // the widest slice's columns (whole chunks)
  int64_t chain;    // lc + ceil(share / lc)
  int64_t workspace_bytes;  // slices * pairs partial tiles
};

inline GramWidePlan plan_gram_wide(int n_clients, int64_t n_cols, int cus, int forced_grid) {
  if (n_clients < 1 || n_clients > kGramWideMaxClients) return GramWidePlan{0, 0, 0, kGramWideKc, kGramLc, 0, 0, 0, 0, 0};
  const int tiles = (n_clients + kGramTile - 1) / kGramTile;
  const int panels = (n_clients + kGramWidePanel - 1) / kGramWidePanel, pairs = panels * (panels + 1) / 2;
  const int64_t chunks = ceil_div(n_cols < 1 ? 1 : n_cols, kGramWideKc);
  int64_t slices = forced_grid > 0 ? forced_grid : (int64_t)kGramWideRounds * cus / pairs;
  if (slices > kGramWideUnitCap / pairs) slices = kGramWideUnitCap / pairs;
  if (slices > chunks) slices = chunks;
  if (slices < 1) slices = 1;
  const int64_t share = ceil_div(chunks, slices) * kGramWideKc;
  return GramWidePlan{tiles, panels, pairs, kGramWideKc, kGramLc, chunks, slices, share,
                      kGramLc + ceil_div(share, kGramLc), slices * pairs * kGramWideSlotBytes};
}

// What fa_gram_wide_workspace answers past FA_GRAM_MAX_CLIENTS: enough for every launch of the
// shape (slices * pairs <= min(chunks * pairs, kGramWideUnitCap)), and never smaller for more
// clients or more columns.
inline int64_t gram_wide_workspace_bytes(int n_clients, int64_t n_cols) {
  const int panels = (n_clients + kGramWidePanel - 1) / kGramWidePanel, pairs = panels * (panels + 1) / 2;
  if (n_cols > (int64_t)kGramWideUnitCap * kGramWideKc) n_cols = (int64_t)kGramWideUnitCap * kGramWideKc;
  const int64_t units = ceil_div(n_cols < 1 ? 1 : n_cols, kGramWideKc) * pairs;
  return (units < kGramWideUnitCap ? units : kGramWideUnitCap) * kGramWideSlotBytes;
}

}  // namespace fa
