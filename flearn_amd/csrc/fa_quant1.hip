// fa_quant1.hip — the 1-bit sign-upload entry of the C ABI (include/flearn_amd.h): fa_deq_fold_q1
// (fa_quant1.hpp: the weighted fp32 sum of sign-and-scale client rows, dequantized in registers,
// opening or continuing an FA_ACC_F32 accumulator for fa_fold_finish).  Host side only, as
// fa_quant4.hip; a unit of its own so that it compiles beside the others and no existing kernel
// shares a unit with it.
#include "fa_quant1.hpp"
#include "fa_quant1_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::q1::sign_fold_kernel;

static_assert(FA_Q1_CHUNK == kQ1Chunk && FA_Q1_CHUNK == fa::q1::kChunk && FA_Q1_BLOCK == fa::q1::kBlock,
              "the header's constants are the kernel's");

int launch_sign_fold(const Plan& p, const uint8_t* stack, int64_t stride, int n, const float* scales, int64_t sstride,
                     const float* weights, const float* center, const float* acc_in, float* acc_out, int64_t col0,
                     int64_t ncols, hipStream_t s) {
  if (p.W == kQ1W && p.V == 1 && p.D == kQ1Depth) {
    FA_LAUNCH_AS(TInst, sign_fold_kernel, (1, kQ1Depth, kQ1W, kNT), p.grid, 64 * kQ1W, s, stack, stride, n, scales,
                 sstride, weights, center, acc_in, acc_out, col0, ncols);
    return launch_check();
  }
  return no_kernel("sign_fold_kernel");
}

}  // namespace

extern "C" {

int fa_deq_fold_q1(const uint8_t* stack, int64_t row_stride, int32_t n_clients, const float* scales,
                   int64_t scale_stride, const float* weights, const float* center, const float* acc_in,
                   float* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !scales || !weights || !acc_out) return fail(FA_ERR_ARG, "null stack, scales, weights or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  // a row holds 8 * row_stride columns; the window's bytes are counted without forming col_begin + n_cols
  if (n_cols < 0 || col_begin < 0 || row_stride < 0 || col_begin / 8 > row_stride ||
      n_cols / 8 + ((n_cols & 7) + (col_begin & 7) + 7) / 8 > row_stride - col_begin / 8)
    return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 16 != 0)
    return fail(FA_ERR_ALIGN, "code rows not 16-B aligned (stack, and row_stride in units of 16)");
  if (col_begin % FA_Q1_CHUNK != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of FA_Q1_CHUNK (2048)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16))
    return fail(FA_ERR_ALIGN, "center, acc_in and acc_out must be 16-B aligned");
  if (!aligned_to(scales, 4) || !aligned_to(weights, 4)) return fail(FA_ERR_ALIGN, "scales and weights must be 4-B aligned");
  if (n_cols > 0 && scale_stride < col_begin / FA_Q1_BLOCK + n_cols / FA_Q1_BLOCK + (n_cols % FA_Q1_BLOCK != 0))
    return fail(FA_ERR_ARG, "bad column window: its last scale block is past scale_stride");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_q1_window(n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_sign_fold(p, stack, row_stride, n_clients, scales, scale_stride, weights, center, acc_in, acc_out,
                          col_begin, n_cols, static_cast<hipStream_t>(stream));
}

}  // extern "C"
