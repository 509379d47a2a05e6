// fa_mx.hip — the Microscaling-upload entry of the C ABI (include/flearn_amd.h): fa_deq_fold_mx
// (fa_mx.hpp: the weighted fp32 sum of MXFP4 or MXFP8 client rows, decoded in registers by the
// scaled converts, opening or continuing an FA_ACC_F32 accumulator for fa_fold_finish).  Host side
// only, as fa_quant1.hip; a unit of its own so that it compiles beside the others and no existing
// kernel shares a unit with it.
#include "fa_mx.hpp"
#include "fa_mx_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::mx::mx_fold_kernel;

static_assert(FA_MX_CHUNK == kMxChunk && FA_MX_CHUNK == fa::mx::kChunk && FA_MX_BLOCK == fa::mx::kBlock,
              "the header's constants are the kernel's");

int launch_mx_fold(const Plan& p, int elem, const uint8_t* stack, int64_t stride, int n, const uint8_t* scales,
                   int64_t sstride, const float* weights, const float* center, const float* acc_in, float* acc_out,
                   int64_t col0, int64_t ncols, hipStream_t s) {
  if (p.W == kMxW && p.V == 1 && elem == FA_MX_FP4 && p.D == kMxDepth4) {
    FA_LAUNCH_AS(TInst, mx_fold_kernel, (FA_MX_FP4, 1, kMxDepth4, kMxW, kNT), p.grid, 64 * kMxW, s, stack, stride, n,
                 scales, sstride, weights, center, acc_in, acc_out, col0, ncols);
    return launch_check();
  }
  if (p.W == kMxW && p.V == 1 && elem == FA_MX_FP8 && p.D == kMxDepth8) {
    FA_LAUNCH_AS(TInst, mx_fold_kernel, (FA_MX_FP8, 1, kMxDepth8, kMxW, kNT), p.grid, 64 * kMxW, s, stack, stride, n,
                 scales, sstride, weights, center, acc_in, acc_out, col0, ncols);
    return launch_check();
  }
  return no_kernel("mx_fold_kernel");
}

}  // namespace

extern "C" {

int fa_deq_fold_mx(const uint8_t* stack, int64_t row_stride, int32_t n_clients, const uint8_t* scales,
                   int64_t scale_stride, const float* weights, const float* center, const float* acc_in,
                   float* acc_out, int64_t col_begin, int64_t n_cols, int32_t elem, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !scales || !weights || !acc_out) return fail(FA_ERR_ARG, "null stack, scales, weights or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (elem != FA_MX_FP4 && elem != FA_MX_FP8) return fail(FA_ERR_ARG, "elem must be FA_MX_FP4 or FA_MX_FP8");
  // a row holds row_stride (FP8) or 2 * row_stride (FP4) columns; the window's bytes are counted
  // without forming col_begin + n_cols
  const int64_t per = elem == FA_MX_FP4 ? 2 : 1;
  if (n_cols < 0 || col_begin < 0 || row_stride < 0 || col_begin / per > row_stride ||
      n_cols / per + (n_cols % per + col_begin % per + per - 1) / per > row_stride - col_begin / per)
    return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 16 != 0)
    return fail(FA_ERR_ALIGN, "code rows not 16-B aligned (stack, and row_stride in units of 16)");
  if (col_begin % FA_MX_CHUNK != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of FA_MX_CHUNK (2048)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16))
    return fail(FA_ERR_ALIGN, "center, acc_in and acc_out must be 16-B aligned");
  if (!aligned_to(scales, 4) || scale_stride % 4 != 0 || !aligned_to(weights, 4))
    return fail(FA_ERR_ALIGN, "scales (and scale_stride, in units of 4) and weights must be 4-B aligned");
  if (n_cols > 0 && (scale_stride < 0 ||
                     scale_stride < col_begin / FA_MX_BLOCK + n_cols / FA_MX_BLOCK + (n_cols % FA_MX_BLOCK != 0)))
    return fail(FA_ERR_ARG, "bad column window: its last scale block is past scale_stride");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_mx_window(n_cols, device_cus(), elem, g_reduce_grid.load(std::memory_order_relaxed));
  return launch_mx_fold(p, elem, stack, row_stride, n_clients, scales, scale_stride, weights, center, acc_in, acc_out,
                        col_begin, n_cols, static_cast<hipStream_t>(stream));
}

}  // extern "C"
