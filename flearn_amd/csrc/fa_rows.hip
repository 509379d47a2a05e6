// fa_rows.hip — the entries of the C ABI (include/flearn_amd.h) beside the one-launch stack reduce:
// the row-pointer path (fa_rows_plan cuts the segments into pieces, fa_reduce_f32_rows launches the
// segmented reduce of fa_segrows.hpp over them, fa_gather_rows* copy per-client tensors into a
// stack), the streamed rounds (fa_fold / fa_fold_finish, fa_fold.hpp), the trimmed sums
// (fa_trim_sum, fa_trim.hpp: one column per lane, the clients sorted in registers, one instantiation
// per padded depth, the 8-byte kinds by repeated selection) and the standalone update fa_opt_apply.
// Host side only, as fa_reduce.hip.  The fold entries share this unit with the segmented reduce on
// purpose: see the note at launch_fold_rows.
#include <algorithm>

#include "fa_fold.hpp"
#include "fa_geometry.hpp"
#include "fa_host.hpp"
#include "fa_segrows.hpp"
#include "fa_trim.hpp"

namespace {

using namespace fa;
using namespace fa::host;

// Segmented row-pointer reduce (fa_reduce_f32_rows): reduce_kernel_segrows_rm — blocks claim
// groups of kSegKG wide pieces (at most kSegPieceChunks KiB of a row each) and sweep them row by
// row, one 64-KiB step (8 waves x 8 KiB) in flight like the stack kernel's row-major groups; then
// the narrow pieces one by one through a 16-deep one-quad sweep.  192 blocks (tools/tune_rows.py,
// profiles/r02/tune_rows/: grouped 100 x ResNet-18 85.7% = the stack kernel's, against 81-84% for
// one claimed piece at a time).  Plain mean: 4 waves x 8 KiB, D = 2; fused epilogues: 8 waves
// x 4 KiB, D = 2.
constexpr int kSegPieceChunks = 64;
constexpr double kSegBlocksPerCU = 0.75;
constexpr int kSegW = 8, kSegV = 8, kSegKG = 2;                // row-major groups of 2 pieces, 8 x 8 KiB
constexpr int64_t kSegWideCols = (int64_t)64 * kSegW * 4;      // wider pieces go into groups

template <class P, int OP, typename T>
int launch_segrows(const float* const* rows, int n, const void* w, const fa_piece* pieces, int64_t npieces,
                   int grid, int32_t* work, const Epi<T>& e, hipStream_t s) {
  const typename P::w_t* wt = static_cast<const typename P::w_t*>(w);
  // f64 sums (np.float64 weights) need twice the accumulator registers: one piece per group
  constexpr int KG = sizeof(typename P::acc_t) == 8 ? 1 : kSegKG;
  // fused f64 state: whole-line stores (FedAVGM 100 x ResNet-50 uploads in place 1647.6 -> 1633.8 us,
  // bit-identical: tools/probe_rows_xl.py, profiles/r05/rows_xl/)
  constexpr bool XLS = sizeof(T) == 8 && OP != FA_OP_MEAN;
  FA_LAUNCH(reduce_kernel_segrows_rm, (P, T, OP, kSegV, kSegW, KG, 16, kNT, false, XLS), grid, 64 * kSegW, s, rows, n,
            wt, pieces, npieces, work, e);
  return launch_check();
}

// fa_gather_rows*: the shared argument checks (`bad`: the entry's own complaint, checked after
// them), then one launch(grid, i0) per tile of up to 65535 clients (the grid's y limit)
template <class F>
int gather_tiles(const void* stack, int64_t row_stride, int32_t n_clients, const void* rows, const int64_t* segs,
                 int32_t n_segments, const char* bad, F&& launch) {
  if (n_clients < 0 || n_segments < 0 || row_stride < 0) return fail(FA_ERR_ARG, "bad gather sizes");
  if (n_clients == 0 || n_segments == 0) return FA_OK;
  if (!stack || !rows || !segs) return fail(FA_ERR_ARG, "null gather pointer");
  if (bad) return fail(FA_ERR_ARG, bad);
  for (int32_t i0 = 0; i0 < n_clients; i0 += 65535) {
    launch(dim3((unsigned)n_segments, (unsigned)std::min<int32_t>(65535, n_clients - i0)), i0);
    if (int rc = launch_check()) return rc;
  }
  return FA_OK;
}

template <typename E>
int gather_rows(void* stack, int64_t row_stride, int32_t n_clients, const void* const* rows, const int64_t* segs,
                int32_t n_segments, void* stream, const char* bad = nullptr) {
  return gather_tiles(stack, row_stride, n_clients, rows, segs, n_segments, bad, [&](dim3 grid, int32_t i0) {
    hipLaunchKernelGGL(gather_rows_kernel<E>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<E*>(stack), row_stride, n_clients, reinterpret_cast<const E* const*>(rows), segs,
                       n_segments, i0);
  });
}

// Piece cut of one segment: `pc` chunks at most, equal pieces (the last one takes the remainder)
template <typename F>
void cut_segment(int64_t len, int64_t pc, F&& emit) {
  const int64_t chunks = (len + 255) / 256;
  if (chunks == 0) return;
  const int64_t np = (chunks + pc - 1) / pc;
  const int64_t per = (chunks + np - 1) / np * 256;  // columns per piece, whole 1-KiB chunks
  for (int64_t off = 0; off < len; off += per) emit(off, len - off < per ? len - off : per);
}

// Why fa_fold is compiled in this unit and not in one of its own: hipcc makes device helpers
// internal and specialises them for their callers in the unit.  fold_kernel_rows<AccF32> calls
// col_rsrc<const float> with a pointer known to be non-null; alone in a unit the helper's null test
// is folded away and the five AccF32 kernels come out with other registers and instruction counts
// (V = 16: 170 VGPRs and 982 instructions against 152 and 1041).  Beside a kernel whose epilogue
// (finish_piece) passes col_rsrc<const float> a pointer that may be null, as reduce_kernel_segrows_rm
// does here, they are instruction for instruction the code that was measured on MI355X
// (tools/kernel_code_diff.py).
//
// fa_fold: one chunk of a streamed round.  plan_fold_window chooses the piece width and the grid;
// FIRST (no acc_in) is a block-uniform branch of the kernel, so only the policy and V are
// template arguments.
template <class P>
int launch_fold_rows(const Plan& p, const float* stack, int64_t stride, int n, const void* w, const void* acc_in,
                     void* acc_out, int64_t col0, int64_t ncols, hipStream_t s) {
  typedef typename P::acc_t A;
  const typename P::w_t* wt = static_cast<const typename P::w_t*>(w);
  const A* ai = static_cast<const A*>(acc_in);
  A* ao = static_cast<A*>(acc_out);
#define FA_FOLD_ROWS(V)                                                                                          \
  case V:                                                                                                        \
    FA_LAUNCH_AS(HInst, fold_kernel_rows, (P, V, kPieceChunks / (V * kFoldW), kFoldW, kNT), p.grid, 64 * kFoldW, \
                 s, stack, stride, n, wt, ai, ao, col0, ncols);                                                  \
    return launch_check()
  if (p.W == kFoldW && p.D == kPieceChunks / (p.V * kFoldW)) {
    switch (p.V) {
      FA_FOLD_ROWS(1);
      FA_FOLD_ROWS(2);
      FA_FOLD_ROWS(4);
      FA_FOLD_ROWS(8);
      FA_FOLD_ROWS(16);
    }
  }
#undef FA_FOLD_ROWS
  return no_kernel("fold_kernel_rows");
}

template <class P>
int launch_fold_elem(const Plan& p, const void* stack, int64_t stride, int n, const void* w, const void* acc_in,
                     void* acc_out, int64_t col0, int64_t ncols, hipStream_t s) {
  typedef typename P::acc_t A;
  FA_LAUNCH_AS(HInst, fold_kernel_elem, (P), p.grid, kThreads, s, static_cast<const typename P::x_t*>(stack), stride,
               n, static_cast<const typename P::w_t*>(w), static_cast<const A*>(acc_in), static_cast<A*>(acc_out), col0,
               ncols);
  return launch_check();
}

// fa_fold_finish: one quad per lane over the accumulator (A), result precision T, op OP
template <typename A, int OP, typename T>
int launch_fold_finish(const A* acc, int64_t n, const Epi<T>& e, hipStream_t s) {
  const int64_t blocks = (n + kThreads * 4 - 1) / (kThreads * 4);
  FA_LAUNCH_AS(FInst, fold_finish_kernel, (A, T, OP), blocks, kThreads, s, acc, n, e);
  return launch_check();
}

// fa_trim_sum: the padded depth NP and the grid come from plan_trim_window
int launch_trim_rows(const TrimPlan& p, const float* stack, int64_t stride, int n, int trim, float* acc_out,
                     int64_t col0, int64_t ncols, hipStream_t s) {
#define FA_TRIM_ROWS(NP)                                                                                        \
  case NP:                                                                                                      \
    FA_LAUNCH_AS(TInst, trim_kernel_rows, (NP, kTrimW, kNT), p.grid, 64 * kTrimW, s, stack, stride, n, trim,    \
                 acc_out, col0, ncols);                                                                         \
    return launch_check()
  switch (p.np) {
    FA_TRIM_ROWS(4);
    FA_TRIM_ROWS(8);
    FA_TRIM_ROWS(16);
    FA_TRIM_ROWS(32);
    FA_TRIM_ROWS(64);
    FA_TRIM_ROWS(128);
  }
#undef FA_TRIM_ROWS
  return no_kernel("trim_kernel_rows");
}

template <typename T>
int launch_trim_elem(int64_t grid, const void* stack, int64_t stride, int n, int trim, void* acc_out, int64_t col0,
                     int64_t ncols, hipStream_t s) {
  FA_LAUNCH_AS(EInst, trim_kernel_elem, (T), grid, kThreads, s, static_cast<const T*>(stack), stride, n, trim,
               static_cast<T*>(acc_out), col0, ncols);
  return launch_check();
}
}  // namespace

extern "C" {

int fa_rows_plan(int32_t n_segments, const int64_t* seg_col, const int64_t* seg_len, int32_t op,
                 int32_t grid_hint, fa_piece* pieces, int64_t cap, int64_t* n_pieces, int32_t* grid) {
  if (n_segments < 0 || (n_segments > 0 && (!seg_col || !seg_len)) || !n_pieces || !grid)
    return fail(FA_ERR_ARG, "bad rows plan arguments");
  if (op < FA_OP_MEAN || op > FA_OP_DYN) return fail(FA_ERR_ARG, "unknown epilogue op");
  for (int32_t s = 0; s < n_segments; ++s)
    if (seg_len[s] < 0 || seg_col[s] < 0 || seg_col[s] % 4 != 0)
      return fail(FA_ERR_ARG, "segment columns must be >= 0 and 4-aligned");
  const int64_t target = grid_hint > 0 ? grid_hint : (int64_t)(device_cus() * kSegBlocksPerCU + 0.5);
  // Piece width and grid: the widest pieces (<= kSegPieceChunks) and a grid near the target
  // whose KG-piece groups fill whole rounds — a group is the unit a block claims, and every slot
  // of the last round left empty is a block idling through a whole group sweep (92% fill left
  // 15 of 192 blocks idle for half of a 100 x ResNet-18 launch: tools/tune_rows.py --trace).
  // A grid hint is taken as given.
  auto count = [&](int64_t pc, int64_t* nwide) {
    int64_t all = 0, wide = 0;
    for (int32_t s = 0; s < n_segments; ++s)
      cut_segment(seg_len[s], pc, [&](int64_t, int64_t cols) {
        ++all;
        wide += cols > kSegWideCols;
      });
    *nwide = wide;
    return all;
  };
  const int64_t glo = grid_hint > 0 ? target : target - target / 8, ghi = target;
  int64_t best_pc = kSegPieceChunks, g = target, best_fill = -1;
  for (int64_t pc = kSegPieceChunks; pc >= kSegPieceChunks * 5 / 8 && best_fill < 1000; --pc) {
    int64_t nwide = 0;
    count(pc, &nwide);
    const int64_t groups = (nwide + kSegKG - 1) / kSegKG;
    for (int64_t gg = ghi; gg >= glo && gg >= 1; --gg) {
      const int64_t rounds = (groups + gg - 1) / gg;
      const int64_t fill = groups == 0 ? 1000 : groups * 1000 / (rounds * gg);  // busy share of the slots
      if (fill > best_fill) {
        best_fill = fill;
        best_pc = pc;
        g = gg;
      }
      if (fill >= 1000) break;
    }
  }
  int64_t nwide = 0;
  const int64_t total = count(best_pc, &nwide);
  const int64_t claims = (nwide + kSegKG - 1) / kSegKG + (total - nwide);
  if (g > claims) g = claims;
  *grid = (int32_t)g;
  *n_pieces = total;
  if (!pieces) return FA_OK;
  if (cap < total) return fail(FA_ERR_SIZE, "piece array too small");
  int64_t k = 0;
  for (int32_t s = 0; s < n_segments; ++s)
    cut_segment(seg_len[s], best_pc, [&](int64_t off, int64_t cols) {
      fa_piece& p = pieces[k++];
      p.col = seg_col[s] + off;
      p.seg_off = off;
      p.seg = s;
      p.n_cols = (int32_t)cols;
      p.aux = 0;
    });
  // largest first (stable: equal pieces keep bucket order): the wide pieces lead and pair into
  // groups of similar size, the narrow ones are claimed last, one at a time
  std::stable_sort(pieces, pieces + k, [](const fa_piece& a, const fa_piece& b) { return a.n_cols > b.n_cols; });
  if (k > 0) pieces[0].aux = nwide;
  return FA_OK;
}

int fa_reduce_f32_rows(const float* const* rows, int32_t n_clients, int32_t mode, const void* weights,
                       double denom, const fa_piece* pieces, int64_t n_pieces, int32_t grid, int32_t* work,
                       const fa_epilogue* epi, float* out32, double* out64, void* stream) {
  g_last_launch = LaunchRecord{};
  if (n_clients <= 0) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_pieces < 0 || (n_pieces > 0 && (!rows || !pieces || !work))) return fail(FA_ERR_ARG, "null rows, pieces or work");
  if (n_pieces > 0 && (grid <= 0 || grid > n_pieces)) return fail(FA_ERR_ARG, "grid must be in [1, n_pieces]");
  if (!weights) return fail(FA_ERR_ARG, "null weights");
  if (!out32 && !out64) return fail(FA_ERR_ARG, "no output");
  if (n_pieces == 0) return FA_OK;
  const int op = epi ? epi->op : FA_OP_MEAN;
  int rc;
  if ((rc = check_columns(out32, out64, epi ? epi->prev : nullptr, epi ? epi->v : nullptr,
                          mode == FA_MODE_W32_DIV32 ? sizeof(float) : sizeof(double), epi ? epi->h : nullptr)))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(work, 0, sizeof(int32_t), s) != hipSuccess) return fail(FA_ERR_LAUNCH, "clearing the piece counter");
  // (no column count for make_epi: the pieces, not one window, say which columns are touched)
  return with_mode(mode, epi, denom, n_clients, out32, out64, 0, [&](auto p, const auto& e) {
    return with_op(op, [&](auto OP) {
      return launch_segrows<decltype(p), OP()>(rows, n_clients, weights, pieces, n_pieces, grid, work, e, s);
    });
  });
}

int fa_gather_rows(void* stack, int64_t row_stride, int32_t n_clients, int32_t elem_size,
                   const void* const* rows, const int64_t* segs, int32_t n_segments, void* stream) {
  const char* bad = elem_size != 4 && elem_size != 8 ? "elem_size must be 4 or 8" : nullptr;
  if (elem_size == 8) return gather_rows<uint64_t>(stack, row_stride, n_clients, rows, segs, n_segments, stream, bad);
  return gather_rows<uint32_t>(stack, row_stride, n_clients, rows, segs, n_segments, stream, bad);
}

int fa_gather_rows_f16(void* stack, int64_t row_stride, int32_t n_clients, const void* const* rows,
                       const int64_t* segs, int32_t n_segments, void* stream) {
  return gather_rows<uint16_t>(stack, row_stride, n_clients, rows, segs, n_segments, stream);
}

int fa_gather_rows_f64(double* stack, int64_t row_stride, int32_t n_clients, const void* const* rows,
                       const int64_t* segs, int32_t n_segments, void* stream) {
  return gather_tiles(stack, row_stride, n_clients, rows, segs, n_segments, nullptr, [&](dim3 grid, int32_t i0) {
    hipLaunchKernelGGL(gather_rows_f64_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), stack,
                       row_stride, n_clients, rows, segs, n_segments, i0);
  });
}

int fa_opt_apply(int32_t prec, const fa_epilogue* epi, const float* local, const void* glob,
                 int64_t n, float* out32, double* out64, void* stream) {
  if (!epi || !glob || n < 0) return fail(FA_ERR_ARG, "bad apply arguments");
  if (!local && epi->op != FA_OP_DYN) return fail(FA_ERR_ARG, "apply needs local");
  if (!out32 && !out64) return fail(FA_ERR_ARG, "no output");
  if (n == 0) return FA_OK;
  if (epi->op == FA_OP_MEAN) return fail(FA_ERR_ARG, "apply needs an optimizer op");
  if (epi->op == FA_OP_DYN && !(epi->n_clients >= 1))
    return fail(FA_ERR_ARG, "FedDyn apply needs n_clients >= 1");
  const size_t ve = prec == FA_PREC_F32 ? sizeof(float) : sizeof(double);
  int rc0 = check_columns(out32, out64, local, epi->v, ve, epi->h);
  if (rc0) return rc0;
  if (!epi->v) return fail(FA_ERR_ARG, "apply needs v");
  fa_epilogue local_epi = *epi;
  if (epi->op != FA_OP_DYN) local_epi.prev = local;
  const int64_t blocks = (n + kThreads * 4 - 1) / (kThreads * 4);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // make_epi has rejected every op but the optimizers' by the time the kernel is chosen
  auto apply = [&](auto t) {
    typedef decltype(t) T;
    Epi<T> e;
    if (int rc = make_epi(&local_epi, 1.0, 1, out32, out64, &e, n)) return rc;
    return with_op(epi->op, [&](auto OP) {
      if constexpr (OP() != FA_OP_MEAN)
        hipLaunchKernelGGL((apply_kernel<T, OP()>), dim3((unsigned)blocks), dim3(kThreads), 0, s,
                           static_cast<const T*>(glob), n, e);
      return launch_check();
    });
  };
  if (prec == FA_PREC_F64) return apply(double{});
  if (prec == FA_PREC_F32) return apply(float{});
  return fail(FA_ERR_ARG, "unknown precision");
}

int fa_fold(int32_t acc_kind, const void* stack, int64_t row_stride, int32_t n_clients, const void* weights,
            const void* acc_in, void* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (acc_kind < FA_ACC_F32 || acc_kind > FA_ACC_I64) return fail(FA_ERR_ARG, "unknown accumulator kind");
  if (int rc = check_window(stack, row_stride, n_clients, weights, col_begin, n_cols, acc_out != nullptr)) return rc;
  const bool wide = acc_kind == FA_ACC_F64 || acc_kind == FA_ACC_I64;
  const bool fp64sum = acc_kind != FA_ACC_F32;
  if (wide ? !aligned_window(static_cast<const double*>(stack), row_stride, col_begin)
           : !aligned_window(static_cast<const float*>(stack), row_stride, col_begin))
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned");
  if (!aligned_to(acc_in, 16) || !aligned_to(acc_out, 16)) return fail(FA_ERR_ALIGN, "accumulator must be 16-B aligned");
  if (acc_in && acc_in != acc_out && overlaps(acc_in, acc_out, (size_t)n_cols * (fp64sum ? 8 : 4)))
    return fail(FA_ERR_ARG, "acc_out must be acc_in or an array not overlapping it");
  if (n_cols == 0) return FA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Plan p = plan_fold_window(acc_kind, n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  switch (acc_kind) {
    case FA_ACC_F32:
      return launch_fold_rows<AccF32>(p, static_cast<const float*>(stack), row_stride, n_clients, weights, acc_in,
                                      acc_out, col_begin, n_cols, s);
    case FA_ACC_F32_W64:
      return launch_fold_rows<AccF32W64>(p, static_cast<const float*>(stack), row_stride, n_clients, weights, acc_in,
                                         acc_out, col_begin, n_cols, s);
    case FA_ACC_F64:
      return launch_fold_elem<AccF64>(p, stack, row_stride, n_clients, weights, acc_in, acc_out, col_begin, n_cols, s);
    default:
      return launch_fold_elem<AccI64>(p, stack, row_stride, n_clients, weights, acc_in, acc_out, col_begin, n_cols, s);
  }
}

int fa_fold_finish(int32_t acc_kind, int32_t mode, const void* acc, double denom, int64_t n_cols,
                   const fa_epilogue* epi, float* out32, double* out64, void* stream) {
  g_last_launch = LaunchRecord{};
  if (acc_kind < FA_ACC_F32 || acc_kind > FA_ACC_I64) return fail(FA_ERR_ARG, "unknown accumulator kind");
  if (n_cols < 0 || !acc) return fail(FA_ERR_ARG, "bad accumulator");
  if (!out32 && !out64) return fail(FA_ERR_ARG, "no output");
  const int op = epi ? epi->op : FA_OP_MEAN;
  const bool fp32rows = acc_kind == FA_ACC_F32 || acc_kind == FA_ACC_F32_W64;
  if (!fp32rows && op != FA_OP_MEAN) return fail(FA_ERR_ARG, "an epilogue needs an fp32 accumulator kind");
  if (acc_kind == FA_ACC_F32 && mode != FA_MODE_W32_DIV64 && mode != FA_MODE_W32_DIV32)
    return fail(FA_ERR_ARG, "FA_ACC_F32 needs mode FA_MODE_W32_DIV64 or FA_MODE_W32_DIV32");
  if (acc_kind == FA_ACC_F32_W64 && mode != FA_MODE_W64) return fail(FA_ERR_ARG, "FA_ACC_F32_W64 needs mode FA_MODE_W64");
  // there is no reduce to take N from
  if (op == FA_OP_DYN && !(epi->n_clients > 0)) return fail(FA_ERR_ARG, "FedDyn finish needs n_clients > 0");
  if (!aligned_to(acc, 16)) return fail(FA_ERR_ALIGN, "accumulator must be 16-B aligned");
  const bool f32res = acc_kind == FA_ACC_F32 && mode == FA_MODE_W32_DIV32;
  if (int rc = check_columns(out32, out64, epi ? epi->prev : nullptr, epi ? epi->v : nullptr,
                             f32res ? sizeof(float) : sizeof(double), epi ? epi->h : nullptr))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto go = [&](auto a, auto t) {
    typedef decltype(a) A;
    typedef decltype(t) T;
    Epi<T> e;
    if (int rc = make_epi(epi, denom, 0, out32, out64, &e, n_cols)) return rc;
    if (n_cols == 0) return (int)FA_OK;
    if constexpr (std::is_same<A, int64_t>::value) {
      return launch_fold_finish<A, FA_OP_MEAN>(static_cast<const A*>(acc), n_cols, e, s);
    } else {
      return with_op(op, [&](auto OP) { return launch_fold_finish<A, OP()>(static_cast<const A*>(acc), n_cols, e, s); });
    }
  };
  switch (acc_kind) {
    case FA_ACC_F32: return f32res ? go(float{}, float{}) : go(float{}, double{});
    case FA_ACC_I64: return go(int64_t{}, double{});
    default: return go(double{}, double{});  // FA_ACC_F32_W64 / FA_ACC_F64 (plain mean only, checked above)
  }
}

int fa_trim_sum(int32_t acc_kind, const void* stack, int64_t row_stride, int32_t n_clients, int32_t trim,
                void* acc_out, int64_t col_begin, int64_t n_cols, void* stream) {
  g_last_launch = LaunchRecord{};
  if (acc_kind != FA_ACC_F32 && acc_kind != FA_ACC_F64 && acc_kind != FA_ACC_I64)
    return fail(FA_ERR_ARG, "trimmed sums take FA_ACC_F32, FA_ACC_F64 or FA_ACC_I64");
  if (n_clients < 1) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (n_clients > FA_TRIM_MAX_CLIENTS) return fail(FA_ERR_ARG, "n_clients exceeds FA_TRIM_MAX_CLIENTS (128)");
  if (trim < 0 || 2 * (int64_t)trim >= n_clients) return fail(FA_ERR_ARG, "trim must satisfy 0 <= 2 * trim < n_clients");
  if (n_cols < 0 || col_begin < 0 || row_stride < col_begin + n_cols) return fail(FA_ERR_ARG, "bad column window");
  if (!stack || !acc_out) return fail(FA_ERR_ARG, "null stack or accumulator");
  if (!aligned_to(stack, 16) || row_stride % 4 != 0 || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "row window not 16-B aligned (stack, and row_stride / col_begin in units of 4)");
  if (!aligned_to(acc_out, 16)) return fail(FA_ERR_ALIGN, "accumulator must be 16-B aligned");
  if (n_cols == 0) return FA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int forced = g_reduce_grid.load(std::memory_order_relaxed);
  if (acc_kind == FA_ACC_F32)
    return launch_trim_rows(plan_trim_window(n_clients, n_cols, device_cus(), forced), static_cast<const float*>(stack),
                            row_stride, n_clients, trim, static_cast<float*>(acc_out), col_begin, n_cols, s);
  const int64_t grid = trim_elem_grid(n_cols, device_cus(), forced);
  if (acc_kind == FA_ACC_F64)
    return launch_trim_elem<double>(grid, stack, row_stride, n_clients, trim, acc_out, col_begin, n_cols, s);
  return launch_trim_elem<int64_t>(grid, stack, row_stride, n_clients, trim, acc_out, col_begin, n_cols, s);
}

}  // extern "C"
