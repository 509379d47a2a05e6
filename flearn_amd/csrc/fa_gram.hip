// fa_gram.hip — the Gram entries of the C ABI (include/flearn_amd.h): fa_gram_workspace and
// fa_gram_f32 (fa_gram.hpp: one MFMA tile kernel per padded client count, then the float64 sum of
// the blocks' partial tiles).  Host side only, as fa_reduce.hip; a unit of its own so that it
// compiles beside the others and no existing kernel shares a unit with it.
#include <string>

#include "fa_geometry.hpp"
#include "fa_gram.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;

// The most blocks a launch uses, whatever the device and the forced grid: what the workspace is
// sized for, so that its size is known without asking for a device.
constexpr int kGramGridCap = 512;

int launch_gram(const GramPlan& p, const float* stack, int64_t stride, int n, const float* center, int64_t col0,
                int64_t ncols, float* partials, double* gram_out, hipStream_t s) {
#define FA_GRAM_TILE(NP)                                                                                      \
  case NP:                                                                                                    \
    if (center)                                                                                               \
      FA_LAUNCH_AS(TInst, gram_kernel_tile, (NP, true, kNT), p.grid, 256, s, stack, stride, n, center, col0,  \
                   ncols, p.chunks, partials);                                                                \
    else                                                                                                      \
      FA_LAUNCH_AS(TInst, gram_kernel_tile, (NP, false, kNT), p.grid, 256, s, stack, stride, n, center, col0, \
                   ncols, p.chunks, partials);                                                                \
    break
  switch (p.np) {
    FA_GRAM_TILE(32);
    FA_GRAM_TILE(64);
    FA_GRAM_TILE(96);
    FA_GRAM_TILE(128);
    default: return no_kernel("gram_kernel_tile");
  }
#undef FA_GRAM_TILE
  if (int rc = launch_check()) return rc;
  // the record keeps naming the tile kernel and its grid
  hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((n * n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     partials, p.grid, p.np, n, gram_out);
  ++g_last_launch.launches;
  return launch_check();
}

int64_t gram_workspace(int n_clients, int64_t n_cols) {
  // past one widest chunk per block of the cap the size no longer grows (and n_cols near 2^63 must not
  // reach the plan's roundings)
  if (n_cols > (int64_t)kGramGridCap * 512) n_cols = (int64_t)kGramGridCap * 512;
  return plan_gram_window(n_clients, n_cols, kGramGridCap, 0).workspace_bytes;
}

}  // namespace

extern "C" {

int64_t fa_gram_workspace(int32_t n_clients, int64_t n_cols) {
  if (n_clients < 1 || n_clients > FA_GRAM_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients must be in [1, FA_GRAM_MAX_CLIENTS (128)]");
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  return gram_workspace(n_clients, n_cols);
}

int fa_gram_f32(const float* stack, int64_t row_stride, int32_t n_clients, const float* center, int64_t col_begin,
                int64_t n_cols, void* workspace, int64_t workspace_bytes, double* gram_out, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !workspace || !gram_out) return fail(FA_ERR_ARG, "null stack, workspace or gram_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_GRAM_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_GRAM_MAX_CLIENTS (128)");
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  if (col_begin < 0 || col_begin > row_stride || n_cols > row_stride - col_begin) return fail(FA_ERR_ARG, "bad column window");
  const int64_t need = gram_workspace(n_clients, n_cols);
  if (workspace_bytes < need)
    return fail(FA_ERR_SIZE, ("workspace too small: fa_gram_workspace gives " + std::to_string(need) + " bytes").c_str());
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(center, 16) || !aligned_to(workspace, 16) || !aligned_to(gram_out, 8))
    return fail(FA_ERR_ALIGN, "center and workspace must be 16-B aligned, gram_out 8-B aligned");
  int forced = g_reduce_grid.load(std::memory_order_relaxed);
  if (forced > kGramGridCap) forced = kGramGridCap;
  const int cus = device_cus();
  const GramPlan p = plan_gram_window(n_clients, n_cols, cus < kGramGridCap ? cus : kGramGridCap, forced);
  return launch_gram(p, stack, row_stride, n_clients, center, col_begin, n_cols, static_cast<float*>(workspace),
                     gram_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
