// fa_reduce.hip — C ABI of the FedAVG-family aggregation engine (include/flearn_amd.h).
//
// Host side only: argument validation, dtype/mode dispatch and launches of the gfx950 kernels in
// fa_device.hpp on the caller's stream.  No allocation, no synchronisation, no host copies.
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
//   * trimmed sums (fa_trim_sum): one column per lane, the clients sorted in registers, one
//     instantiation per padded depth (plan_trim_window); 8-byte kinds by repeated selection.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <atomic>
#include <string>
#include <type_traits>
#include <vector>

#include "fa_device.hpp"
#include "fa_geometry.hpp"
#include "flearn_amd.h"

namespace {

using namespace fa;

thread_local std::string g_last_error;

int fail(int code, const char* what) {
  g_last_error = what;
  return code;
}

// fa_last_launch (ABI 16): what the calling thread's last fa_reduce_* / fa_fold* / fa_trim_sum call launched.  A launch
// stores a pointer and two integers; the name is built once per instantiation (a static of its
// launch site, as resident_blocks_per_cu keeps its occupancy).
struct LaunchRecord {
  const char* kernel = nullptr;
  int64_t grid = 0;
  int32_t launches = 0;
};
thread_local LaunchRecord g_last_launch;

template <class P, typename T, auto... A>
struct Inst {};
template <class HP, auto... A>
struct HInst {};  // the float16 family has no T

// "family<P,T,args...>": the kernel's demangled symbol name without `fa::`, whitespace and the
// argument list.  FA_LAUNCH instantiates the kernel from the same argument list, every defaulted
// template argument spelled out, so the name cannot drift from what is launched.
std::string make_kernel_name(const char* family, const std::string& f) {
  // f: pretty_of<Inst<...>>(), "... [I = (anonymous namespace)::Inst<fa::AccF32, float, 0, ...>]"
  std::string out = family;
  const size_t b = f.find("Inst<"), e = f.rfind('>');
  if (b == std::string::npos || e == std::string::npos) return out;
  for (size_t i = b + 4; i <= e; ++i) {
    if (f.compare(i, 4, "fa::") == 0) i += 4;
    if (f[i] != ' ') out += f[i];
  }
  return out;
}

template <class I>
const char* pretty_of() {
  return __PRETTY_FUNCTION__;
}

inline void note_launch(const std::string& kernel, int64_t grid) {
  g_last_launch.kernel = kernel.c_str();
  g_last_launch.grid = grid;
  ++g_last_launch.launches;
}

#define FA_TARGS(...) __VA_ARGS__
// FA_LAUNCH(kernel family, (all of its template arguments), grid, block, stream, kernel arguments...)
// The name is a static of the launch site, built at the first launch of each instantiation.
// FA_LAUNCH_AS names the tag template first: HInst for the float16 family.
#define FA_LAUNCH_AS(Tag, family, targs, grid, block, stream, ...)                                              \
  do {                                                                                                          \
    hipLaunchKernelGGL((family<FA_TARGS targs>), dim3((unsigned)(grid)), dim3(block), 0, stream, __VA_ARGS__);  \
    static const std::string name_ = make_kernel_name(#family, pretty_of<Tag<FA_TARGS targs>>());               \
    note_launch(name_, (int64_t)(grid));                                                                        \
  } while (0)
#define FA_LAUNCH(...) FA_LAUNCH_AS(Inst, __VA_ARGS__)

// The runtime epilogue op as a compile-time constant: f(std::integral_constant<int, OP>{}).
template <class F>
int with_op(int op, F&& f) {
  switch (op) {
    case FA_OP_MEAN: return f(std::integral_constant<int, FA_OP_MEAN>{});
    case FA_OP_AVGM: return f(std::integral_constant<int, FA_OP_AVGM>{});
    case FA_OP_ADAGRAD: return f(std::integral_constant<int, FA_OP_ADAGRAD>{});
    case FA_OP_YOGI: return f(std::integral_constant<int, FA_OP_YOGI>{});
    case FA_OP_ADAM: return f(std::integral_constant<int, FA_OP_ADAM>{});
    case FA_OP_DYN: return f(std::integral_constant<int, FA_OP_DYN>{});
    default: return fail(FA_ERR_ARG, "unknown epilogue op");
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr bool kNT = true;  // client bytes are read once: non-temporal

int device_cus() {
  static thread_local int dev = -1, cus = 0;
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return 256;
  if (d != dev) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || cus <= 0)
      cus = 256;
    dev = d;
  }
  return cus;
}

template <typename K>
int resident_blocks_per_cu(K kernel) {
  static int occ = 0;  // per kernel instantiation
  if (occ == 0) {
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kernel, kThreads, 0) != hipSuccess || o <= 0) o = 1;
    occ = o;
  }
  return occ;
}

template <typename X>
bool aligned_window(const X* stack, int64_t stride, int64_t col0) {
  const uintptr_t a = (uintptr_t)(stack + col0);
  return (a % (4 * sizeof(X))) == 0 && ((stride * (int64_t)sizeof(X)) % (4 * sizeof(X))) == 0;
}

int launch_check() {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(err));
  return FA_OK;
}

// fa_set_reduce_grid: 0 = the geometry (fa_geometry.hpp) chooses the grid
std::atomic<int> g_reduce_grid{0};

// One column window of a client stack: the arguments every stack kernel takes, in their order.
template <class P, typename T>
struct Window {
  const typename P::x_t* stack;
  int64_t stride;
  int n;
  const typename P::w_t* w;
  int64_t col0, ncols;
  Epi<T> e;
};
#define FA_WIN(a) a.stack, a.stride, a.n, a.w, a.col0, a.ncols, a.e

// The launchers below turn a Plan (fa_geometry.hpp) into the template instantiation it names, one
// switch per kernel family.  They choose nothing: a plan value with no shipped instantiation is an
// error, never another kernel.
int no_kernel(const char* family) {
  return fail(FA_ERR_ARG, (std::string("no shipped ") + family + " instantiation for the plan").c_str());
}

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

template <typename T>
Epi<T> epi_at(const Epi<T>& e, int64_t c) {  // the epilogue's per-column arrays from column c on
  Epi<T> o = e;
  if (o.prev) o.prev += c;
  if (o.v) o.v += c;
  if (o.v_out) o.v_out += c;
  if (o.h) o.h += c;
  if (o.out32) o.out32 += c;
  if (o.out64) o.out64 += c;
  return o;
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
  const Plan p = plan_f16_window(VMAX, ncols, device_cus());
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

bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// [a, a + bytes) and [b, b + bytes) share a byte
bool overlaps(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// ncols: the columns the launch touches (0: unknown — only the exact-alias check applies)
template <typename T>
int make_epi(const fa_epilogue* in, double denom, int n_reduced, float* out32, double* out64, Epi<T>* e,
             int64_t ncols = 0) {
  e->denom = (T)denom;
  e->prev = nullptr;
  e->v = nullptr;
  e->h = nullptr;
  e->trace = nullptr;
  e->v_out = nullptr;
  e->beta = e->eta = e->tau = e->beta2 = e->c = e->n = T(0);
  e->alpha32 = 0.f;
  e->out32 = out32;
  e->out64 = out64;
  if (!in || in->op == FA_OP_MEAN) return FA_OK;
  if (in->op < FA_OP_AVGM || in->op > FA_OP_DYN) return fail(FA_ERR_ARG, "unknown epilogue op");
  if (!in->v) return fail(FA_ERR_ARG, "epilogue needs v");
  e->v = static_cast<T*>(in->v);
  if (in->v_out) {
    if (!aligned_to(in->v_out, 4 * sizeof(T))) return fail(FA_ERR_ALIGN, "v_out must be 4-element aligned");
    if (in->v_out == in->v || (ncols > 0 && overlaps(in->v_out, in->v, (size_t)ncols * sizeof(T))))
      return fail(FA_ERR_ARG, "v_out must be NULL (in place) or an array not overlapping v");
    e->v_out = static_cast<T*>(in->v_out);
  }
  if (in->op == FA_OP_DYN) {
    if (!in->h) return fail(FA_ERR_ARG, "FedDyn epilogue needs h");
    const double nc = in->n_clients > 0 ? in->n_clients : (double)n_reduced;
    if (!(nc >= 1)) return fail(FA_ERR_ARG, "FedDyn epilogue needs n_clients >= 1");
    e->h = in->h;
    e->n = (T)nc;
    e->c = (T)(in->alpha / nc);  // self.alpha / len(w_local_lst): a Python float   dyn.py:26
    e->alpha32 = (float)in->alpha;
    return FA_OK;
  }
  if (!in->prev) return fail(FA_ERR_ARG, "epilogue needs prev and v");
  e->prev = in->prev;
  e->beta = (T)in->beta;
  e->eta = (T)in->eta;
  e->tau = (T)in->tau;
  e->beta2 = (T)in->beta2;
  e->c = (T)(1.0 - in->beta2);  // Python evaluates (1 - self.beta2) in double
  return FA_OK;
}

// The fp32 reduce mode as its accumulation policy P and epilogue precision T: builds the Epi<T>
// (make_epi; ncols as there) and calls f(P{}, e).
template <class F>
int with_mode(int mode, const fa_epilogue* epi, double denom, int n_clients, float* out32, double* out64,
              int64_t ncols, F&& f) {
  auto go = [&](auto p, auto t) {
    Epi<decltype(t)> e;
    if (int rc = make_epi(epi, denom, n_clients, out32, out64, &e, ncols)) return rc;
    return f(p, e);
  };
  switch (mode) {
    case FA_MODE_W32_DIV64: return go(AccF32{}, double{});
    case FA_MODE_W32_DIV32: return go(AccF32{}, float{});
    case FA_MODE_W64: return go(AccF32W64{}, double{});
    default: return fail(FA_ERR_ARG, "unknown reduce mode");
  }
}

// per-column arrays are accessed with 4-element vector loads/stores
int check_columns(const float* out32, const double* out64, const void* prev, const void* v,
                  size_t v_elem, const float* h = nullptr) {
  if (!aligned_to(out32, 16) || !aligned_to(out64, 32) || !aligned_to(prev, 16) ||
      !aligned_to(v, 4 * v_elem) || !aligned_to(h, 16))
    return fail(FA_ERR_ALIGN, "output / prev / v / h arrays must be 4-element aligned");
  return FA_OK;
}

// What every fa_reduce_* entry checks first, in this order
int check_window(const void* stack, int64_t stride, int n, const void* w, int64_t col0, int64_t ncols,
                 bool has_output) {
  if (n <= 0) return fail(FA_ERR_ARG, "n_clients must be >= 1");
  if (ncols < 0 || col0 < 0 || stride < col0 + ncols) return fail(FA_ERR_ARG, "bad column window");
  if (!stack || !w) return fail(FA_ERR_ARG, "null stack or weights");
  if (!has_output) return fail(FA_ERR_ARG, "no output");
  return FA_OK;
}

template <typename X>
int check_common(const X* stack, int64_t stride, int n, const void* w, int64_t col0,
                 int64_t ncols, const void* o1, const void* o2) {
  if (int rc = check_window(stack, stride, n, w, col0, ncols, o1 || o2)) return rc;
  if (!aligned_window(stack, stride, col0)) return fail(FA_ERR_ALIGN, "row window not 16-B aligned");
  return FA_OK;
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
template <class AT, typename T, auto... X>
struct FInst {};  // the naming tag: fold_finish_kernel<A,T,OP>
template <typename A, int OP, typename T>
int launch_fold_finish(const A* acc, int64_t n, const Epi<T>& e, hipStream_t s) {
  const int64_t blocks = (n + kThreads * 4 - 1) / (kThreads * 4);
  FA_LAUNCH_AS(FInst, fold_finish_kernel, (A, T, OP), blocks, kThreads, s, acc, n, e);
  return launch_check();
}

// fa_trim_sum: the padded depth NP and the grid come from plan_trim_window
template <auto... A>
struct TInst {};  // the naming tags: trim_kernel_rows<NP,W,NT>, trim_kernel_elem<T>
template <class T>
struct EInst {};
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

int fa_copy(void* dst, const void* src, int64_t nbytes, void* stream) {
  if ((!dst || !src) && nbytes > 0) return fail(FA_ERR_ARG, "null copy pointer");
  if (nbytes < 0) return fail(FA_ERR_ARG, "negative copy size");
  if (nbytes == 0) return FA_OK;
  if (((uintptr_t)dst | (uintptr_t)src) & 15) return fail(FA_ERR_ALIGN, "copy pointers must be 16-byte aligned");
  // 512 blocks of 256 lanes, grid-stride: enough 16-B stores in flight for PCIe (tools/probe_zc.cpp)
  const int64_t quads = nbytes / 16;
  int64_t blocks = (quads + kThreads - 1) / kThreads;
  if (blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(copy_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), nbytes);
  return launch_check();
}

// fa_push's default grid.  The kernel is paced (each wave drains its stores per round): a block
// keeps 4 waves x 4 quads x 1 KiB = 16 KiB in flight per destination link, so 16 blocks keep
// ~256 KiB per link — about an xGMI link's bandwidth-delay product (64-153 GB/s x 1-2 us), more
// only queues in the fabric and slows a reduce beside the push.  Provisional:
// no multi-GPU run has measured it against seven xGMI links; bench.py's calibration picks the grid
// on the node and records every grid's push-beside-reduce pair, 16 included
constexpr int64_t kPushGrid = 16;

int fa_ipc_handle(const void* ptr, void* handle, int64_t* offset) {
  if (!ptr || !handle || !offset) return fail(FA_ERR_ARG, "null ipc argument");
  static_assert(sizeof(hipIpcMemHandle_t) == FA_IPC_HANDLE_BYTES, "IPC handle size");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  hipError_t e = hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(ptr)));
  if (e != hipSuccess) return fail(FA_ERR_ARG, hipGetErrorString(e));
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, reinterpret_cast<void*>(base));
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  memcpy(handle, &h, sizeof h);
  *offset = (int64_t)((const char*)ptr - (const char*)base);
  return FA_OK;
}

int fa_ipc_open(const void* handle, void** base) {
  if (!handle || !base) return fail(FA_ERR_ARG, "null ipc argument");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof h);
  const hipError_t e = hipIpcOpenMemHandle(base, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

int fa_ipc_close(void* base) {
  if (!base) return fail(FA_ERR_ARG, "null ipc base");
  const hipError_t e = hipIpcCloseMemHandle(base);
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

int fa_dev_alloc(int64_t nbytes, void** ptr) {
  if (!ptr || nbytes <= 0) return fail(FA_ERR_ARG, "bad device allocation request");
  *ptr = nullptr;
  const hipError_t e = hipMalloc(ptr, (size_t)nbytes);
  if (e != hipSuccess) {
    *ptr = nullptr;
    return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  }
  return FA_OK;
}

int fa_dev_free(void* ptr) {
  if (!ptr) return FA_OK;
  const hipError_t e = hipFree(ptr);
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

int fa_mem_range(const void* ptr, void** base, int64_t* size) {
  if (!ptr || !base || !size) return fail(FA_ERR_ARG, "null range argument");
  hipDeviceptr_t b = nullptr;
  size_t n = 0;
  const hipError_t e = hipMemGetAddressRange(&b, &n, reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(ptr)));
  if (e != hipSuccess) return fail(FA_ERR_ARG, hipGetErrorString(e));
  *base = reinterpret_cast<void*>(b);
  *size = (int64_t)n;
  return FA_OK;
}

int fa_push(const void* src, int64_t nbytes, void* const* dsts, int32_t n_dsts, int32_t grid, void* stream) {
  if (nbytes < 0 || n_dsts < 0 || n_dsts > 8 || grid < 0) return fail(FA_ERR_ARG, "bad push size, destination count or grid");
  if (nbytes == 0 || n_dsts == 0) return FA_OK;
  if (!src || !dsts) return fail(FA_ERR_ARG, "null push pointer");
  PushDsts d{};
  uintptr_t any = (uintptr_t)src;
  for (int i = 0; i < n_dsts; ++i) {
    if (!dsts[i]) return fail(FA_ERR_ARG, "null push destination");
    d.p[i] = static_cast<uint8_t*>(dsts[i]);
    any |= (uintptr_t)dsts[i];
  }
  if ((any & 15) || (nbytes & 15)) return fail(FA_ERR_ALIGN, "push pointers and size must be 16-byte multiples");
  const int64_t quads = nbytes / 16;
  int64_t blocks = (quads + kThreads - 1) / kThreads;
  const int64_t cap = grid > 0 ? grid : kPushGrid;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(push_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(src), quads, d, n_dsts);
  return launch_check();
}

constexpr hipMemcpyKind kCopyEngine = hipMemcpyDeviceToDeviceNoCU;

int fa_copy_dma(void* dst, const void* src, int64_t nbytes, void* stream) {
  if (nbytes < 0) return fail(FA_ERR_ARG, "negative copy size");
  if (nbytes == 0) return FA_OK;
  if (!dst || !src) return fail(FA_ERR_ARG, "null copy pointer");
  // NoCU: a copy engine, not the runtime's blit kernel.  With hipMemcpyDeviceToDevice the runtime
  // ran every leg as __amd_rocclr_copyBuffer kernels on the compute queues (rocprofv3, round 5:
  // profiles/r05/push_dma_trace/) — the CUs and memory pipelines the "copy-engine" push was meant
  // to leave to the reduce
  const hipError_t e = hipMemcpyAsync(dst, src, (size_t)nbytes, kCopyEngine, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

// one event recorded on `from`, waited for by `to` (destroyed at once: HIP releases it when done)
static int stream_after(hipStream_t to, hipStream_t from) {
  hipEvent_t ev;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ev, from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
  (void)hipEventDestroy(ev);
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

int fa_push_dma(const void* src, int64_t nbytes, void* const* dsts, int32_t n_dsts, void* const* streams,
                void* stream) {
  if (nbytes < 0 || n_dsts < 0 || n_dsts > 8) return fail(FA_ERR_ARG, "bad push size or destination count");
  if (nbytes == 0 || n_dsts == 0) return FA_OK;
  if (!src || !dsts || !streams) return fail(FA_ERR_ARG, "null push pointer");
  for (int i = 0; i < n_dsts; ++i)
    if (!dsts[i] || !streams[i]) return fail(FA_ERR_ARG, "null push destination or stream");
  hipEvent_t ev;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ev, static_cast<hipStream_t>(stream));
  for (int i = 0; i < n_dsts && e == hipSuccess; ++i) {
    hipStream_t s = static_cast<hipStream_t>(streams[i]);
    e = hipStreamWaitEvent(s, ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(dsts[i], src, (size_t)nbytes, kCopyEngine, s);
  }
  (void)hipEventDestroy(ev);
  if (e != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(e));
  return FA_OK;
}

int fa_cache_fence(int32_t kind, void* stream) {
  // 64 one-wave blocks: workgroups are dealt round-robin over the 8 XCDs, so every XCD's L2 gets
  // the fence from several waves
  if (kind == FA_FENCE_RELEASE)
    hipLaunchKernelGGL(cache_fence_kernel<0>, dim3(64), dim3(64), 0, static_cast<hipStream_t>(stream));
  else if (kind == FA_FENCE_ACQUIRE)
    hipLaunchKernelGGL(cache_fence_kernel<1>, dim3(64), dim3(64), 0, static_cast<hipStream_t>(stream));
  else
    return fail(FA_ERR_ARG, "unknown cache fence kind");
  return launch_check();
}

int fa_stream_join(void* stream, void* const* streams, int32_t n) {
  if (n < 0 || n > 16 || (n > 0 && !streams)) return fail(FA_ERR_ARG, "bad stream list");
  for (int i = 0; i < n; ++i) {
    const int rc = stream_after(static_cast<hipStream_t>(stream), static_cast<hipStream_t>(streams[i]));
    if (rc) return rc;
  }
  return FA_OK;
}

int fa_fill_uniform_f32(float* dst, int64_t row_stride, int32_t n_rows, int64_t n_cols,
                        uint64_t seed, int64_t row_begin, int64_t col_global_begin, void* stream) {
  if (!dst || n_rows < 0 || n_cols < 0 || row_stride < n_cols) return fail(FA_ERR_ARG, "bad fill");
  if (n_rows == 0 || n_cols == 0) return FA_OK;
  if (n_rows > 65535) return fail(FA_ERR_ARG, "too many rows for one fill");
  int64_t bx = (n_cols + kThreads - 1) / kThreads;
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)bx, (unsigned)n_rows), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), dst, row_stride, n_cols, seed, row_begin,
                     col_global_begin);
  return launch_check();
}

}  // extern "C"

