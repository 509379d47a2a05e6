// fa_trimwide.hip — the wide trimmed-sum entry of the C ABI (include/flearn_amd.h): fa_trim_sum_wide
// (fa_trimwide.hpp: up to 1024 clients, a column's clients sorted by several lanes and merged through
// LDS).  Host side only, as fa_quant4.hip; a unit of its own so that it compiles beside the others
// and no existing kernel shares a unit with it.  It instantiates merge_trim_kernel alone: the depths
// fa_trim_sum serves go to fa_trim_sum, and the 8-byte kinds to fa_rows.hip's trim_kernel_elem
// launcher (fa::host::launch_trim_elem_kind).
#include "fa_trimwide.hpp"
#include "fa_trimwide_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::trimwide::merge_trim_kernel;

static_assert(kTrimWideRun == fa::trimwide::kRun && kTrimWideThreads == fa::trimwide::kThreads,
              "the plan's constants are the kernel's");

int launch_merge_trim(const TrimWidePlan& p, const float* stack, int64_t stride, int n, int trim, float* acc_out,
                      int64_t col0, int64_t ncols, hipStream_t s) {
#define FA_MERGE_TRIM(NP)                                                                                       \
  case NP:                                                                                                      \
    FA_LAUNCH_AS(TInst, merge_trim_kernel, (NP, kNT), p.grid, kTrimWideThreads, s, stack, stride, n, trim,      \
                 acc_out, col0, ncols);                                                                         \
    return launch_check()
  switch (p.np) {
    FA_MERGE_TRIM(256);
    FA_MERGE_TRIM(512);
    FA_MERGE_TRIM(1024);
  }
#undef FA_MERGE_TRIM
  return no_kernel("merge_trim_kernel");
}

}  // namespace

extern "C" {

int fa_trim_sum_wide(int32_t acc_kind, const void* stack, int64_t row_stride, int32_t n_clients, int32_t trim,
                     void* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (acc_kind != FA_ACC_F32 && acc_kind != FA_ACC_F64 && acc_kind != FA_ACC_I64)
    return fail(FA_ERR_ARG, "trimmed sums take FA_ACC_F32, FA_ACC_F64 or FA_ACC_I64");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_TRIM_WIDE_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_TRIM_WIDE_MAX_CLIENTS (1024)");
  if (trim < 0 || 2 * (int64_t)trim >= n_clients) return fail(FA_ERR_ARG, "trim must satisfy 0 <= 2 * trim < n_clients");
  if (n_cols < 0 || col_begin < 0 || row_stride < col_begin + n_cols) return fail(FA_ERR_ARG, "bad column window");
  if (!stack || !acc_out) return fail(FA_ERR_ARG, "null stack or accumulator");
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(acc_out, 16)) return fail(FA_ERR_ALIGN, "accumulator must be 16-B aligned");
  if (n_cols == 0) return FA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (acc_kind != FA_ACC_F32)  // O(n^2) per column: meant for small buckets such as BN counters
    return launch_trim_elem_kind(acc_kind, stack, row_stride, n_clients, trim, acc_out, col_begin, n_cols, s);
  if (n_clients <= FA_TRIM_MAX_CLIENTS)  // the register sort: the same plan, launch and record
    return fa_trim_sum(acc_kind, stack, row_stride, n_clients, trim, acc_out, col_begin, n_cols, stream);
  const int forced = g_reduce_grid.load(std::memory_order_relaxed);
  return launch_merge_trim(plan_trim_wide_window(n_clients, n_cols, device_cus(), forced),
                           static_cast<const float*>(stack), row_stride, n_clients, trim, static_cast<float*>(acc_out),
                           col_begin, n_cols, s);
}

}  // extern "C"
