// fa_bf16.hip — the bfloat16-upload entry of the C ABI (include/flearn_amd.h): fa_fold_bf16
// (fa_bf16.hpp: the weighted fp32 sum of bfloat16 client rows, widened in registers, opening or
// continuing an FA_ACC_F32 accumulator for fa_fold_finish).  Host side only, as fa_quant.hip; a unit
// of its own so that it compiles beside the others and no existing kernel shares a unit with it.
#include "fa_bf16.hpp"
#include "fa_bf16_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::bf16::widen_fold_kernel;

int launch_widen_fold(const Plan& p, const uint16_t* stack, int64_t stride, int n, const float* weights,
                      const float* acc_in, float* acc_out, int64_t col0, int64_t ncols, hipStream_t s) {
#define FA_WIDEN_FOLD(V)                                                                                       \
  case V:                                                                                                      \
    FA_LAUNCH_AS(TInst, widen_fold_kernel, (V, kBf16InFlight / (V * kBf16W), kBf16W, kNT), p.grid, 64 * kBf16W, s, \
                 stack, stride, n, weights, acc_in, acc_out, col0, ncols);                                     \
    return launch_check()
  if (p.W == kBf16W && p.V >= 1 && p.D == kBf16InFlight / (p.V * kBf16W)) {
    switch (p.V) {
      FA_WIDEN_FOLD(1);
      FA_WIDEN_FOLD(2);
      FA_WIDEN_FOLD(4);
    }
  }
#undef FA_WIDEN_FOLD
  return no_kernel("widen_fold_kernel");
}

}  // namespace

extern "C" {

int fa_fold_bf16(const uint16_t* stack, int64_t row_stride, int32_t n_clients, const float* weights,
                 const float* acc_in, float* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !weights || !acc_out) return fail(FA_ERR_ARG, "null stack, weights or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_cols < 0 || col_begin < 0 || col_begin > row_stride || n_cols > row_stride - col_begin)
    return fail(FA_ERR_ARG, "bad column window");
  // (n_cols <= row_stride, and a row of 2^62 columns is no address range: the byte count cannot wrap)
  if (acc_in && acc_in != acc_out && n_cols <= (INT64_MAX >> 2) && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (!aligned_to(stack, 16) || row_stride % 8 != 0)
    return fail(FA_ERR_ALIGN, "bfloat16 rows not 16-B aligned (stack, and row_stride in units of 8)");
  if (col_begin % 8 != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of 8 (one 16-B load)");
  if (!aligned_to(acc_out, 16) || !aligned_to(acc_in, 16))
    return fail(FA_ERR_ALIGN, "acc_in and acc_out must be 16-B aligned");
  if (!aligned_to(weights, 4)) return fail(FA_ERR_ALIGN, "weights must be 4-B aligned");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_bf16_window(n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_widen_fold(p, stack, row_stride, n_clients, weights, acc_in, acc_out, col_begin, n_cols,
                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
