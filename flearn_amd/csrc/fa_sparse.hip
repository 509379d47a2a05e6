// fa_sparse.hip — the sparse-upload entries of the C ABI (include/flearn_amd.h): fa_sparse_workspace
// and fa_sparse_fold_f32 (fa_sparse.hpp: the ordered fp32 sum of top-k client rows, opening or
// continuing an FA_ACC_F32 accumulator for fa_fold_finish).  Host side only, as fa_mx.hip; a unit of
// its own so that it compiles beside the others and no existing kernel shares a unit with it.
#include <string>

#include "fa_sparse.hpp"
#include "fa_sparse_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::sparse::bounds_kernel;
using fa::sparse::window_fold_kernel;

}  // namespace

extern "C" {

int64_t fa_sparse_workspace(int32_t n_clients, int64_t n_cols) {
  if (n_clients < 1 || n_clients > FA_SPARSE_MAX_CLIENTS)
    return fail(FA_ERR_ARG, "n_clients must be in [1, FA_SPARSE_MAX_CLIENTS (1024)]");
  if (n_cols < 0 || n_cols > kSparseMaxColumn) return fail(FA_ERR_ARG, "n_cols must be in [0, 2^32 - 1]");
  return sparse_workspace_bytes(n_clients, n_cols);
}

int fa_sparse_fold_f32(const uint32_t* pairs, int64_t row_stride_pairs, int32_t n_clients, const float* weights,
                       const float* center, float wsum, const float* acc_in, float* acc_out, int64_t col_begin,
                       int64_t n_cols, void* workspace, int64_t workspace_bytes, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!pairs || !weights || !acc_out || !workspace) return fail(FA_ERR_ARG, "null pairs, weights, acc_out or workspace");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_SPARSE_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_SPARSE_MAX_CLIENTS (1024)");
  if (n_cols < 0 || col_begin < 0 || row_stride_pairs < 0) return fail(FA_ERR_ARG, "bad column window or row stride");
  // columns are uint32 and 0xFFFFFFFF is the padding pair's: the window ends below it
  if (col_begin > kSparseMaxColumn || n_cols > kSparseMaxColumn - col_begin)
    return fail(FA_ERR_SIZE, "the column window does not fit uint32 columns (col_begin + n_cols <= 2^32 - 1)");
  if (row_stride_pairs > kSparseMaxRowPairs) return fail(FA_ERR_SIZE, "row_stride_pairs exceeds 2^27 pairs");
  const int64_t need = sparse_workspace_bytes(n_clients, n_cols);
  if (workspace_bytes < need)
    return fail(FA_ERR_SIZE, ("workspace too small: fa_sparse_workspace gives " + std::to_string(need) + " bytes").c_str());
  if (!aligned_to(pairs, 16) || row_stride_pairs % 2 != 0)
    return fail(FA_ERR_ALIGN, "pair rows not 16-B aligned (pairs, and row_stride_pairs in units of 2)");
  if (col_begin % 4 != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of 4");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16) || !aligned_to(workspace, 16))
    return fail(FA_ERR_ALIGN, "center, acc_in, acc_out and workspace must be 16-B aligned");
  if (!aligned_to(weights, 4)) return fail(FA_ERR_ALIGN, "weights must be 4-B aligned");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const SparsePlan p = plan_sparse_window(n_clients, n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* bounds = static_cast<int*>(workspace);
  hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)p.bounds_grid), dim3(256), 0, s, pairs, row_stride_pairs,
                     (int)row_stride_pairs, n_clients, col_begin, n_cols, kSparseWC, p.nwin, bounds);
  if (int rc = launch_check()) return rc;
  FA_LAUNCH_AS(TInst, window_fold_kernel, (kSparseWC, kSparseDepth, kSparseW), p.grid, 64 * kSparseW, s, pairs,
               row_stride_pairs, (int)row_stride_pairs, n_clients, weights, center, wsum, acc_in, acc_out, col_begin,
               n_cols, p.nwin, bounds);
  ++g_last_launch.launches;  // the bounds launch before it
  return launch_check();
}

}  // extern "C"
