// fa_quant.hip — the quantized-upload entry of the C ABI (include/flearn_amd.h): fa_deq_fold_q8
// (fa_quant.hpp: the weighted fp32 sum of int8 block-quantized client rows, dequantized in
// registers, opening or continuing an FA_ACC_F32 accumulator for fa_fold_finish).  Host side only,
// as fa_clip.hip; a unit of its own so that it compiles beside the others and no existing kernel
// shares a unit with it.
#include "fa_quant.hpp"
#include "fa_quant_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::quant::deq_fold_kernel;

int launch_deq_fold(const Plan& p, const int8_t* stack, int64_t stride, int n, const float* scales, int64_t sstride,
                    const float* weights, const float* center, const float* acc_in, float* acc_out, int64_t col0,
                    int64_t ncols, hipStream_t s) {
#define FA_DEQ_FOLD(V)                                                                                      \
  case V:                                                                                                   \
    FA_LAUNCH_AS(TInst, deq_fold_kernel, (V, kQ8InFlight / (V * kQ8W), kQ8W, kNT), p.grid, 64 * kQ8W, s,    \
                 stack, stride, n, scales, sstride, weights, center, acc_in, acc_out, col0, ncols);         \
    return launch_check()
  if (p.W == kQ8W && p.V >= 1 && p.D == kQ8InFlight / (p.V * kQ8W)) {
    switch (p.V) {
      FA_DEQ_FOLD(1);
      FA_DEQ_FOLD(2);
    }
  }
#undef FA_DEQ_FOLD
  return no_kernel("deq_fold_kernel");
}

}  // namespace

extern "C" {

int fa_deq_fold_q8(const int8_t* stack, int64_t row_stride, int32_t n_clients, const float* scales,
                   int64_t scale_stride, const float* weights, const float* center, const float* acc_in,
                   float* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !scales || !weights || !acc_out) return fail(FA_ERR_ARG, "null stack, scales, weights or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_cols < 0 || col_begin < 0 || col_begin > row_stride || n_cols > row_stride - col_begin)
    return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 16 != 0)
    return fail(FA_ERR_ALIGN, "code rows not 16-B aligned (stack, and row_stride in units of 16)");
  if (col_begin % FA_Q8_BLOCK != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of FA_Q8_BLOCK (1024)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16))
    return fail(FA_ERR_ALIGN, "center, acc_in and acc_out must be 16-B aligned");
  if (!aligned_to(scales, 4) || !aligned_to(weights, 4)) return fail(FA_ERR_ALIGN, "scales and weights must be 4-B aligned");
  if (n_cols > 0 && scale_stride < ceil_div(col_begin + n_cols, (int64_t)FA_Q8_BLOCK))
    return fail(FA_ERR_ARG, "bad column window: its last scale block is past scale_stride");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_q8_window(n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_deq_fold(p, stack, row_stride, n_clients, scales, scale_stride, weights, center, acc_in, acc_out,
                         col_begin, n_cols, static_cast<hipStream_t>(stream));
}

}  // extern "C"
