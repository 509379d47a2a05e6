// fa_reduce.hip — C ABI of the FedAVG-family aggregation engine (include/flearn_amd.h).
//
// Host side only: argument validation, dtype/mode dispatch and launches of the gfx950 kernels in
// fa_stack.hpp and fa_half.hpp on the caller's stream.  No allocation, no synchronisation, no host copies.
// Which kernel instantiation runs for a shape, and on what grid, is decided in fa_geometry.hpp
// (pure integer code, testable without a GPU; measured with tools/tune_reduce.hip on MI355X, see
// DESIGN.md §4); here one launcher per kernel family turns its Plan into the instantiation:
//   * fp32 client stacks (every configuration of the hot path): the row-pipelined kernel on
//     192 blocks (0.75 per CU) with equal interleaved pieces of the window; each block sweeps its
//     pieces (V KiB x W waves wide; W = 4 for the mean, 8 with a fused optimizer epilogue), rows
//     pipelined D = 64/(V*W) deep through per-row buffer descriptors (~64 KiB of client rows in
//     flight per block, whatever the window's width or depth);
//   * 8-byte kinds (f64 / i64 buckets, small): 4 quads per thread, one row at a time;
//   * float16 client stacks (fa_reduce_f16): the fp32 one-piece geometry for the same byte width
//     (plan_f16_window), octs of 8 halves per 16-B load.
// This unit holds the client-stack entries (fa_reduce_f32 / _splitn / _f64 / _i64 / _f16) and the
// readers of the state in fa_host.hpp (fa_last_error, fa_last_launch, fa_set_reduce_grid); the
// row-pointer, streamed and trimmed entries are in fa_rows.hip, and the copies, pushes and fences
// in fa_transport.hip.
#include "fa_geometry.hpp"
#include "fa_half.hpp"
#include "fa_host.hpp"
#include "fa_stack.hpp"

namespace {

using namespace fa;
using namespace fa::host;

// one piece per block: 4 waves for the mean; fused epilogues 4 waves up to 8 KiB and for the
// filled 16 / 32 KiB pieces, else 8 waves
template <int OP, class P, typename T>
int launch_rows(const Plan& p, const Window<P, T>& a, hipStream_t s) {
  constexpr bool kMean = OP == FA_OP_MEAN;
#define FA_ROWS(V, W, SHIPPED)                                                                                      \
  case V * 100 + W:                                                                                                 \
    if constexpr (SHIPPED) {                                                                                        \
      static_assert(V * W <= kPieceChunks, "piece wider than the in-flight budget");                                \
      FA_LAUNCH(reduce_kernel_rows, (P, T, OP, V, kPieceChunks / (V * W), W, kNT), p.grid, 64 * W, s, FA_WIN(a));   \
      return launch_check();                                                                                        \
    }                                                                                                               \
    break
  switch (p.V * 100 + p.W) {
    FA_ROWS(1, 4, true);
    FA_ROWS(2, 4, true);
    FA_ROWS(4, 4, true);
    FA_ROWS(8, 4, true);
    FA_ROWS(16, 4, kMean);
    FA_ROWS(2, 8, !kMean);
    FA_ROWS(4, 8, !kMean);
    FA_ROWS(8, 8, !kMean);
  }
#undef FA_ROWS
  return no_kernel("reduce_kernel_rows");
}

template <int OP, class P, typename T>
int launch_narrow(const Plan& p, const Window<P, T>& a, hipStream_t s) {
#define FA_NARROW(D)                                                                  \
  case D:                                                                             \
    FA_LAUNCH(reduce_kernel_narrow, (P, T, OP, D, 1, kNT), p.grid, 64, s, FA_WIN(a)); \
    return launch_check()
  switch (p.D) {
    FA_NARROW(16);
    FA_NARROW(32);
    FA_NARROW(40);
  }
#undef FA_NARROW
  return no_kernel("reduce_kernel_narrow");
}

template <int OP, int KG, class P, typename T>
int launch_rowmajor_kg(const Plan& p, const Window<P, T>& a, hipStream_t s) {
  constexpr bool XL = sizeof(T) == 8 && OP != FA_OP_MEAN && KG <= 3;  // the kernel's default, spelled out
  constexpr int EB = OP == FA_OP_MEAN ? 2 : 4;                        // EPIB of the 4 x 16 form
  if (!p.wide16 && p.EPIB == 2) {
    FA_LAUNCH(reduce_kernel_rowmajor, (P, T, OP, 8, 1, 8, KG, kNT, 2, false, XL), p.grid, 512, s, FA_WIN(a));
    return launch_check();
  }
  // Yogi's f64 epilogue has no 4 x 16 form at KG = 4 (fa_geometry.hpp rowmajor_plan)
  if constexpr (KG <= 3 || !(OP == FA_OP_YOGI && sizeof(T) == 8)) {
    if (p.wide16 && p.EPIB == EB) {
      FA_LAUNCH(reduce_kernel_rowmajor, (P, T, OP, 16, 1, 4, KG, kNT, EB, false, XL), p.grid, 256, s, FA_WIN(a));
      return launch_check();
    }
  }
  return no_kernel("reduce_kernel_rowmajor");
}

template <int OP, class P, typename T>
int launch_rowmajor(const Plan& p, const Window<P, T>& a, hipStream_t s) {
  if constexpr (sizeof(typename P::acc_t) == 4) {  // fp32 sums only
    switch (p.KG) {
      case 2: return launch_rowmajor_kg<OP, 2>(p, a, s);
      case 3: return launch_rowmajor_kg<OP, 3>(p, a, s);
      case 4: return launch_rowmajor_kg<OP, 4>(p, a, s);
    }
  }
  return no_kernel("reduce_kernel_rowmajor");
}

template <int OP, class P, typename T>
int launch_splitn(const Plan& p, const Window<P, T>& a, hipStream_t s) {
  if (p.W != kSplitW || p.D != kSplitD) return no_kernel("reduce_kernel_splitn");
  FA_LAUNCH(reduce_kernel_splitn, (P, T, OP, kSplitW, kSplitD, kNT), p.grid, 64 * kSplitW, s, FA_WIN(a));
  return launch_check();
}

// fa_reduce_f32 / fa_reduce_f32_splitn (reorder): the window split and each window's plan come
// from fa_geometry.hpp, the family's launcher instantiates it.
template <class P, int OP, typename T>
int launch_reduce(int mode, bool reorder, const float* stack, int64_t stride, int n, const void* w, int64_t col0,
                  int64_t ncols, const Epi<T>& e, hipStream_t s) {
  const int cus = device_cus();
  const int forced = g_reduce_grid.load(std::memory_order_relaxed);
  const int S = mode != FA_MODE_W64 && forced <= 0 ? window_count(OP, ncols) : 1;
  const int64_t width = window_width(ncols, S);
  for (int64_t c = 0; c < ncols; c += width) {
    const int64_t wc = ncols - c < width ? ncols - c : width;
    const Window<P, T> a{stack, stride, n, static_cast<const typename P::w_t*>(w), col0 + c, wc, epi_at(e, c)};
    const Plan p = plan_f32_window(mode, OP, n, wc, cus, forced, reorder && S == 1);
    int rc;
    switch (p.family) {
      case kFamRows: rc = launch_rows<OP>(p, a, s); break;
      case kFamNarrow: rc = launch_narrow<OP>(p, a, s); break;
      case kFamRowmajor: rc = launch_rowmajor<OP>(p, a, s); break;
      case kFamSplitn: rc = launch_splitn<OP>(p, a, s); break;
      default: rc = no_kernel("fp32 stack");
    }
    if (rc) return rc;
  }
  return FA_OK;
}

// fa_reduce_f64 / fa_reduce_i64: the occupancy query stays here, the grid rule is balanced_grid's
template <class P>
int launch_balanced(const Window<P, double>& a, hipStream_t s) {
  const auto kernel = reduce_kernel_balanced<P, double, FA_OP_MEAN, kBalancedV, kBalancedU, kNT>;
  const int64_t slots = (int64_t)device_cus() * resident_blocks_per_cu(kernel);
  FA_LAUNCH(reduce_kernel_balanced, (P, double, FA_OP_MEAN, kBalancedV, kBalancedU, kNT),
            balanced_grid(row_chunks(a.ncols), slots), kThreads, s, FA_WIN(a));
  return launch_check();
}

// fa_reduce_f16: VMAX bounds the instantiations (the sums' registers per oct, fa_geometry.hpp)
template <class HP, int DIV, int VMAX>
int launch_reduce_h16(const uint16_t* stack, int64_t stride, int n, const void* w, int64_t col0, int64_t ncols,
                      const EpiH16& e, hipStream_t s) {
  const Plan p = plan_f16_window(VMAX, ncols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  const typename HP::w_t* wt = static_cast<const typename HP::w_t*>(w);
#define FA_ROWS_H16(V, DEPTH, W)                                                                               \
  case V * 100 + W:                                                                                            \
    if constexpr (V <= VMAX) {                                                                                 \
      if (p.D != DEPTH) break;                                                                                 \
      FA_LAUNCH_AS(HInst, reduce_kernel_rows_h16, (HP, DIV, V, DEPTH, W, kNT), p.grid, 64 * W, s, stack,       \
                   stride, n, wt, col0, ncols, e);                                                             \
      return launch_check();                                                                                   \
    }                                                                                                          \
    break
  switch (p.V * 100 + p.W) {
    FA_ROWS_H16(1, 16, 1);
    FA_ROWS_H16(1, 16, 4);
    FA_ROWS_H16(2, 8, 4);
    FA_ROWS_H16(4, 4, 4);
    FA_ROWS_H16(8, 2, 4);
    FA_ROWS_H16(16, 1, 4);
  }
#undef FA_ROWS_H16
  return no_kernel("reduce_kernel_rows_h16");
}

// fa_reduce_f32 and fa_reduce_f32_splitn (reorder: the caller allows the split-N order)
int reduce_f32(bool reorder, const float* stack, int64_t row_stride, int32_t n_clients, int32_t mode,
               const void* weights, double denom, int64_t col_begin, int64_t n_cols, const fa_epilogue* epi,
               float* out32, double* out64, void* stream) {
  g_last_launch = LaunchRecord{};
  int rc = check_common(stack, row_stride, n_clients, weights, col_begin, n_cols, out32, out64);
  if (rc) return rc;
  if (n_cols == 0) return FA_OK;
  const int op = epi ? epi->op : FA_OP_MEAN;
  if ((rc = check_columns(out32, out64, epi ? epi->prev : nullptr, epi ? epi->v : nullptr,
                          mode == FA_MODE_W32_DIV32 ? sizeof(float) : sizeof(double),
                          epi ? epi->h : nullptr)))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_mode(mode, epi, denom, n_clients, out32, out64, n_cols, [&](auto p, const auto& e) {
    return with_op(op, [&](auto OP) {
      return launch_reduce<decltype(p), OP()>(mode, reorder, stack, row_stride, n_clients, weights, col_begin, n_cols,
                                              e, s);
    });
  });
}

// fa_reduce_f64 (P = AccF64) and fa_reduce_i64 (AccI64)
template <class P>
int reduce_8byte(const typename P::x_t* stack, int64_t row_stride, int32_t n_clients,
                 const typename P::w_t* weights, double denom, int64_t col_begin, int64_t n_cols, double* out64,
                 void* stream) {
  g_last_launch = LaunchRecord{};
  int rc = check_common(stack, row_stride, n_clients, weights, col_begin, n_cols, out64, nullptr);
  if (rc) return rc;
  if (n_cols == 0) return FA_OK;
  if ((rc = check_columns(nullptr, out64, nullptr, nullptr, 8))) return rc;
  Window<P, double> a{stack, row_stride, n_clients, weights, col_begin, n_cols, {}};
  make_epi<double>(nullptr, denom, n_clients, nullptr, out64, &a.e);
  return launch_balanced(a, static_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" {

int fa_abi_version(void) { return FA_ABI_VERSION; }

const char* fa_last_error(void) { return g_last_error.c_str(); }

int fa_reduce_f32(const float* stack, int64_t row_stride, int32_t n_clients, int32_t mode,
                  const void* weights, double denom, int64_t col_begin, int64_t n_cols,
                  const fa_epilogue* epi, float* out32, double* out64, void* stream) {
  return reduce_f32(false, stack, row_stride, n_clients, mode, weights, denom, col_begin, n_cols, epi, out32, out64,
                    stream);
}

int fa_reduce_f32_splitn(const float* stack, int64_t row_stride, int32_t n_clients, int32_t mode,
                         const void* weights, double denom, int64_t col_begin, int64_t n_cols,
                         const fa_epilogue* epi, float* out32, double* out64, void* stream) {
  return reduce_f32(true, stack, row_stride, n_clients, mode, weights, denom, col_begin, n_cols, epi, out32, out64,
                    stream);
}

int fa_reduce_f64(const double* stack, int64_t row_stride, int32_t n_clients,
                  const double* weights, double denom, int64_t col_begin, int64_t n_cols,
                  double* out64, void* stream) {
  return reduce_8byte<AccF64>(stack, row_stride, n_clients, weights, denom, col_begin, n_cols, out64, stream);
}

int fa_reduce_i64(const int64_t* stack, int64_t row_stride, int32_t n_clients,
                  const int64_t* weights, double denom, int64_t col_begin, int64_t n_cols,
                  double* out64, void* stream) {
  return reduce_8byte<AccI64>(stack, row_stride, n_clients, weights, denom, col_begin, n_cols, out64, stream);
}

int fa_reduce_f16(const void* stack, int64_t row_stride, int32_t n_clients, int32_t mode, const void* weights,
                  double denom, int64_t col_begin, int64_t n_cols, void* out16, float* out32, double* out64,
                  void* stream) {
  g_last_launch = LaunchRecord{};
  if (int rc = check_window(stack, row_stride, n_clients, weights, col_begin, n_cols, out16 || out32 || out64))
    return rc;
  if (mode < FA_MODE_H16_NUMPY || mode > FA_MODE_H16_W64) return fail(FA_ERR_ARG, "unknown float16 reduce mode");
  if (!aligned_to(stack, 16) || row_stride % 8 != 0 || col_begin % 8 != 0)
    return fail(FA_ERR_ALIGN, "float16 row window not 16-B aligned (stack, row_stride and col_begin in units of 8)");
  if (!aligned_to(out16, 16) || !aligned_to(out32, 16) || !aligned_to(out64, 32))
    return fail(FA_ERR_ALIGN, "output arrays must be 16-B (out16, out32) / 32-B (out64) aligned");
  if (n_cols == 0) return FA_OK;
  const EpiH16 e{denom, static_cast<uint16_t*>(out16), out32, out64};
  const uint16_t* st = static_cast<const uint16_t*>(stack);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (mode) {
    case FA_MODE_H16_NUMPY:
      return launch_reduce_h16<AccH16Pk, kDivF64, 16>(st, row_stride, n_clients, weights, col_begin, n_cols, e, s);
    case FA_MODE_H16_TORCH:
      return launch_reduce_h16<AccH16Torch, kDivF64, 16>(st, row_stride, n_clients, weights, col_begin, n_cols, e, s);
    case FA_MODE_H16_NP16:
      return launch_reduce_h16<AccH16Pk, kDivF16, 16>(st, row_stride, n_clients, weights, col_begin, n_cols, e, s);
    case FA_MODE_H16_W32:
      return launch_reduce_h16<AccH16W32, kDivF32, 8>(st, row_stride, n_clients, weights, col_begin, n_cols, e, s);
    default:
      return launch_reduce_h16<AccH16W64, kDivF64, 4>(st, row_stride, n_clients, weights, col_begin, n_cols, e, s);
  }
}

int fa_reduce_windows(int32_t op, int64_t n_cols) {
  if (n_cols < 0) return fail(FA_ERR_ARG, "negative n_cols");
  if (g_reduce_grid.load(std::memory_order_relaxed) > 0) return 1;
  if (op < FA_OP_MEAN || op > FA_OP_DYN) return fail(FA_ERR_ARG, "unknown epilogue op");
  return window_count(op, n_cols);
}

int fa_set_reduce_grid(int32_t grid) {
  if (grid < 0) return fail(FA_ERR_ARG, "grid must be >= 0");
  return g_reduce_grid.exchange(grid);
}

int fa_last_launch(fa_launch_record* out) {
  if (!out) return fail(FA_ERR_ARG, "null launch record");
  out->kernel = g_last_launch.kernel;
  out->grid = g_last_launch.grid;
  out->launches = g_last_launch.launches;
  out->reserved = 0;
  return FA_OK;
}

}  // extern "C"
