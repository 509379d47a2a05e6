// fa_gramwide.hip — the wide Gram entries of the C ABI (include/flearn_amd.h): fa_gram_wide_workspace
// and fa_gram_f32_wide (fa_gramwide.hpp: up to 1024 clients, one block per column slice and pair of
// 128-row panels, then the float64 sum of the slices' partial tiles).  Host side only, as
// fa_trimwide.hip; a unit of its own so that it compiles beside the others and no existing kernel
// shares a unit with it.  It instantiates panel_pair_kernel and panel_finish_kernel alone: the depths
// fa_gram_f32 serves go to fa_gram_f32.
#include <string>

#include "fa_gramwide.hpp"
#include "fa_gramwide_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::gramwide::panel_finish_kernel;
using fa::gramwide::panel_pair_kernel;

constexpr int kGramWideCuCap = kGramWideUnitCap / kGramWideRounds;  // the natural grid stays under the unit cap

int launch_gram_wide(const GramWidePlan& p, const float* stack, int64_t stride, int n, const float* center,
                     int64_t col0, int64_t ncols, float* partials, double* gram_out, hipStream_t s) {
  const int64_t grid = p.slices * p.pairs;
  if (center)
    FA_LAUNCH_AS(TInst, panel_pair_kernel, (true), grid, 256, s, stack, stride, n, center, col0, ncols, p.chunks,
                 (int)p.slices, p.panels, (int)fa::gramwide::kPairMajor, partials);
  else
    FA_LAUNCH_AS(TInst, panel_pair_kernel, (false), grid, 256, s, stack, stride, n, center, col0, ncols, p.chunks,
                 (int)p.slices, p.panels, (int)fa::gramwide::kPairMajor, partials);
  if (int rc = launch_check()) return rc;
  // the record keeps naming the pair kernel and its grid
  hipLaunchKernelGGL(panel_finish_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, s, partials,
                     (int)p.slices, p.panels, n, gram_out);
  ++g_last_launch.launches;
  return launch_check();
}

}  // namespace

extern "C" {

int64_t fa_gram_wide_workspace(int32_t n_clients, int64_t n_cols) {
  if (n_clients < 1 || n_clients > FA_GRAM_WIDE_MAX_CLIENTS)
    return fail(FA_ERR_ARG, "n_clients must be in [1, FA_GRAM_WIDE_MAX_CLIENTS (1024)]");
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  if (n_clients <= FA_GRAM_MAX_CLIENTS) return fa_gram_workspace(n_clients, n_cols);
  return gram_wide_workspace_bytes(n_clients, n_cols);
}

int fa_gram_f32_wide(const float* stack, int64_t row_stride, int32_t n_clients, const float* center, int64_t col_begin,
                     int64_t n_cols, void* workspace, int64_t workspace_bytes, double* gram_out, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !workspace || !gram_out) return fail(FA_ERR_ARG, "null stack, workspace or gram_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_GRAM_WIDE_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_GRAM_WIDE_MAX_CLIENTS (1024)");
  if (n_clients <= FA_GRAM_MAX_CLIENTS)  // the one-block tile kernel: the same checks, plan, launch and record
    return fa_gram_f32(stack, row_stride, n_clients, center, col_begin, n_cols, workspace, workspace_bytes, gram_out,
                       stream);
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  if (col_begin < 0 || col_begin > row_stride || n_cols > row_stride - col_begin) return fail(FA_ERR_ARG, "bad column window");
  const int64_t need = gram_wide_workspace_bytes(n_clients, n_cols);
  if (workspace_bytes < need)
    return fail(FA_ERR_SIZE, ("workspace too small: fa_gram_wide_workspace gives " + std::to_string(need) + " bytes").c_str());
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(center, 16) || !aligned_to(workspace, 16) || !aligned_to(gram_out, 8))
    return fail(FA_ERR_ALIGN, "center and workspace must be 16-B aligned, gram_out 8-B aligned");
  int forced = g_reduce_grid.load(std::memory_order_relaxed);
  if (forced > kGramWideUnitCap) forced = kGramWideUnitCap;
  const int cus = device_cus();
  const GramWidePlan p = plan_gram_wide(n_clients, n_cols, cus < kGramWideCuCap ? cus : kGramWideCuCap, forced);
  return launch_gram_wide(p, stack, row_stride, n_clients, center, col_begin, n_cols, static_cast<float*>(workspace),
                          gram_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
