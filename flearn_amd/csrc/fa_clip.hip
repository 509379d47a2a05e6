// fa_clip.hip — the norm-clipping entries of the C ABI (include/flearn_amd.h): fa_rownorm_workspace,
// fa_rownorm2_f32 (fa_clip.hpp: the clients' squared update norms, one fp32 partial per client and
// block, then their float64 sum) and fa_clip_sum_f32 (the sum of the clipped uploads, an FA_ACC_F32
// accumulator for fa_fold_finish), and fa_clip_fold_f32 (fa_clipfold.hpp: the clipped sum of one chunk
// of a streamed round, opening or continuing the accumulator).  Host side only, as fa_gram.hip; a unit of its own so that it
// compiles beside the others and no existing kernel shares a unit with it.
#include <string>

#include "fa_clip.hpp"
#include "fa_clipfold.hpp"
#include "fa_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using namespace fa::clip;
using fa::clipfold::clip_fold_kernel;

int launch_rownorm(const RownormPlan& p, const float* stack, int64_t stride, int n, const float* center, int64_t col0,
                   int64_t ncols, float* partials, double* norm2_out, hipStream_t s) {
#define FA_ROWNORM(V)                                                                                           \
  case V:                                                                                                       \
    FA_LAUNCH_AS(TInst, rownorm_kernel, (V, kPieceChunks / (V * kFoldW), kFoldW, kNT), p.grid, 64 * kFoldW, s,  \
                 stack, stride, n, center, col0, ncols, p.pc, partials);                                        \
    break
  if (p.W != kFoldW || p.D != kPieceChunks / ((p.V ? p.V : 1) * kFoldW)) return no_kernel("rownorm_kernel");
  switch (p.V) {
    FA_ROWNORM(1);
    FA_ROWNORM(2);
    FA_ROWNORM(4);
    FA_ROWNORM(8);
    FA_ROWNORM(16);
    default: return no_kernel("rownorm_kernel");
  }
#undef FA_ROWNORM
  if (int rc = launch_check()) return rc;
  // the record keeps naming the sweep and its grid
  hipLaunchKernelGGL(rownorm_finish_kernel, dim3(1), dim3(128), 0, s, partials, (int)p.grid, n, norm2_out);
  ++g_last_launch.launches;
  return launch_check();
}

int launch_clip_sum(const Plan& p, const float* stack, int64_t stride, int n, const float* center, const float* scale,
                    float* acc_out, int64_t col0, int64_t ncols, hipStream_t s) {
#define FA_CLIP_SUM(V)                                                                                          \
  case V:                                                                                                       \
    FA_LAUNCH_AS(TInst, clip_sum_kernel, (V, kPieceChunks / (V * kFoldW), kFoldW, kNT), p.grid, 64 * kFoldW, s, \
                 stack, stride, n, center, scale, acc_out, col0, ncols);                                        \
    return launch_check()
  if (p.W == kFoldW && p.D == kPieceChunks / (p.V * kFoldW)) {
    switch (p.V) {
      FA_CLIP_SUM(1);
      FA_CLIP_SUM(2);
      FA_CLIP_SUM(4);
      FA_CLIP_SUM(8);
      FA_CLIP_SUM(16);
    }
  }
#undef FA_CLIP_SUM
  return no_kernel("clip_sum_kernel");
}

int launch_clip_fold(const Plan& p, const float* stack, int64_t stride, int n, const float* center, const float* scale,
                     const float* acc_in, float* acc_out, int64_t col0, int64_t ncols, hipStream_t s) {
#define FA_CLIP_FOLD(V)                                                                                          \
  case V:                                                                                                        \
    FA_LAUNCH_AS(TInst, clip_fold_kernel, (V, kPieceChunks / (V * kFoldW), kFoldW, kNT), p.grid, 64 * kFoldW, s, \
                 stack, stride, n, center, scale, acc_in, acc_out, col0, ncols);                                 \
    return launch_check()
  if (p.W == kFoldW && p.D == kPieceChunks / (p.V * kFoldW)) {
    switch (p.V) {
      FA_CLIP_FOLD(1);
      FA_CLIP_FOLD(2);
      FA_CLIP_FOLD(4);
      FA_CLIP_FOLD(8);
      FA_CLIP_FOLD(16);
    }
  }
#undef FA_CLIP_FOLD
  return no_kernel("clip_fold_kernel");
}

bool bad_window(int64_t row_stride, int64_t col_begin, int64_t n_cols) {
  return col_begin < 0 || col_begin > row_stride || n_cols > row_stride - col_begin;
}

}  // namespace

extern "C" {

int64_t fa_rownorm_workspace(int32_t n_clients, int64_t n_cols) {
  if (n_clients < 1 || n_clients > FA_CLIP_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients must be in [1, FA_CLIP_MAX_CLIENTS (128)]");
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  return rownorm_workspace_bytes(n_clients, n_cols);
}

int fa_rownorm2_f32(const float* stack, int64_t row_stride, int32_t n_clients, const float* center, int64_t col_begin,
                    int64_t n_cols, void* workspace, int64_t workspace_bytes, double* norm2_out, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !workspace || !norm2_out) return fail(FA_ERR_ARG, "null stack, workspace or norm2_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_CLIP_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_CLIP_MAX_CLIENTS (128)");
  if (n_cols < 1) return fail(FA_ERR_ARG, "n_cols must be >= 1");
  if (bad_window(row_stride, col_begin, n_cols)) return fail(FA_ERR_ARG, "bad column window");
  const int64_t need = rownorm_workspace_bytes(n_clients, n_cols);
  if (workspace_bytes < need)
    return fail(FA_ERR_SIZE, ("workspace too small: fa_rownorm_workspace gives " + std::to_string(need) + " bytes").c_str());
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(center, 16) || !aligned_to(workspace, 16) || !aligned_to(norm2_out, 8))
    return fail(FA_ERR_ALIGN, "center and workspace must be 16-B aligned, norm2_out 8-B aligned");
  int forced = g_reduce_grid.load(std::memory_order_relaxed);
  if (forced > kRownormGridCap) forced = kRownormGridCap;
  const RownormPlan p = plan_rownorm_window(n_clients, n_cols, device_cus(), forced);
  return launch_rownorm(p, stack, row_stride, n_clients, center, col_begin, n_cols, static_cast<float*>(workspace),
                        norm2_out, static_cast<hipStream_t>(stream));
}

int fa_clip_sum_f32(const float* stack, int64_t row_stride, int32_t n_clients, const float* center, const float* scale,
                    float* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !center || !scale || !acc_out) return fail(FA_ERR_ARG, "null stack, center, scale or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_CLIP_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_CLIP_MAX_CLIENTS (128)");
  if (n_cols < 0 || bad_window(row_stride, col_begin, n_cols)) return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(scale, 4))
    return fail(FA_ERR_ALIGN, "center and acc_out must be 16-B aligned, scale 4-B aligned");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_fold_window(FA_ACC_F32, n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_clip_sum(p, stack, row_stride, n_clients, center, scale, acc_out, col_begin, n_cols,
                         static_cast<hipStream_t>(stream));
}

int fa_clip_fold_f32(const float* stack, int64_t row_stride, int32_t n_clients, const float* center,
                     const float* scale, const float* acc_in, float* acc_out, int64_t col_begin, int64_t n_cols,
                     void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !center || !scale || !acc_out) return fail(FA_ERR_ARG, "null stack, center, scale or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_CLIP_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_CLIP_MAX_CLIENTS (128)");
  if (n_cols < 0 || bad_window(row_stride, col_begin, n_cols)) return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16) || !aligned_to(scale, 4))
    return fail(FA_ERR_ALIGN, "center, acc_in and acc_out must be 16-B aligned, scale 4-B aligned");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_fold_window(FA_ACC_F32, n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_clip_fold(p, stack, row_stride, n_clients, center, scale, acc_in, acc_out, col_begin, n_cols,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
