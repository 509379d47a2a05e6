// fa_quant4.hip — the 4-bit quantized-upload entry of the C ABI (include/flearn_amd.h):
// fa_deq_fold_q4 (fa_quant4.hpp: the weighted fp32 sum of int4 block-quantized client rows,
// dequantized in registers, opening or continuing an FA_ACC_F32 accumulator for fa_fold_finish).
// Host side only, as fa_quant.hip; a unit of its own so that it compiles beside the others and no
// existing kernel shares a unit with it.
#include "fa_quant4.hpp"
#include "fa_quant4_geometry.hpp"
#include "fa_host.hpp"

namespace {

using namespace fa;
using namespace fa::host;
using fa::q4::deq_fold4_kernel;

static_assert(FA_Q4_CHUNK == kQ4Chunk && FA_Q4_CHUNK == fa::q4::kChunk && FA_Q4_BLOCK == fa::q4::kBlock,
              "the header's constants are the kernel's");

int launch_deq_fold4(const Plan& p, const uint8_t* stack, int64_t stride, int n, const float* scales, int64_t sstride,
                     const float* weights, const float* center, const float* acc_in, float* acc_out, int64_t col0,
                     int64_t ncols, hipStream_t s) {
#define FA_DEQ_FOLD4(V)                                                                                     \
  case V:                                                                                                   \
    FA_LAUNCH_AS(TInst, deq_fold4_kernel, (V, kQ4InFlight / (V * kQ4W), kQ4W, kNT), p.grid, 64 * kQ4W, s,   \
                 stack, stride, n, scales, sstride, weights, center, acc_in, acc_out, col0, ncols);         \
    return launch_check()
  if (p.W == kQ4W && p.V >= 1 && p.V <= kQ4MaxV && p.D == kQ4InFlight / (p.V * kQ4W)) {
    switch (p.V) {
      FA_DEQ_FOLD4(1);
    }
  }
#undef FA_DEQ_FOLD4
  return no_kernel("deq_fold4_kernel");
}

}  // namespace

extern "C" {

int fa_deq_fold_q4(const uint8_t* stack, int64_t row_stride, int32_t n_clients, const float* scales,
                   int64_t scale_stride, const float* weights, const float* center, const float* acc_in,
                   float* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (!stack || !scales || !weights || !acc_out) return fail(FA_ERR_ARG, "null stack, scales, weights or acc_out");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  // a row holds 2 * row_stride columns; the window's bytes are counted without forming col_begin + n_cols
  if (n_cols < 0 || col_begin < 0 || row_stride < 0 || col_begin / 2 > row_stride ||
      n_cols / 2 + ((n_cols & 1) + (col_begin & 1) + 1) / 2 > row_stride - col_begin / 2)
    return fail(FA_ERR_ARG, "bad column window");
  if (!aligned_to(stack, 16) || row_stride % 16 != 0)
    return fail(FA_ERR_ALIGN, "code rows not 16-B aligned (stack, and row_stride in units of 16)");
  if (col_begin % FA_Q4_CHUNK != 0) return fail(FA_ERR_ALIGN, "col_begin must be a multiple of FA_Q4_CHUNK (2048)");
  if (!aligned_to(center, 16) || !aligned_to(acc_out, 16) || !aligned_to(acc_in, 16))
    return fail(FA_ERR_ALIGN, "center, acc_in and acc_out must be 16-B aligned");
  if (!aligned_to(scales, 4) || !aligned_to(weights, 4)) return fail(FA_ERR_ALIGN, "scales and weights must be 4-B aligned");
  if (n_cols > 0 && scale_stride < col_begin / FA_Q4_BLOCK + n_cols / FA_Q4_BLOCK + (n_cols % FA_Q4_BLOCK != 0))
    return fail(FA_ERR_ARG, "bad column window: its last scale block is past scale_stride");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * 4))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  const Plan p = plan_q4_window(n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  return launch_deq_fold4(p, stack, row_stride, n_clients, scales, scale_stride, weights, center, acc_in, acc_out,
                          col_begin, n_cols, static_cast<hipStream_t>(stream));
}

}  // extern "C"
