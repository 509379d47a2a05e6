// fa_host.hpp — what the host units of the C ABI (fa_reduce.hip, fa_rows.hip, fa_gram.hip, fa_clip.hip, fa_noise.hip, fa_quant.hip, fa_transport.hip)
// share: the per-thread error and launch-record state, the launch macros that name an
// instantiation as they launch it, the op / mode dispatch, and the argument checks.  Internal:
// inline functions and variables in namespace fa::host, nothing with a C name.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <atomic>
#include <string>
#include <type_traits>

#include "fa_geometry.hpp"
#include "fa_numerics.hpp"
#include "flearn_amd.h"

namespace fa {
namespace host {

// One object per thread (the error text, the launch record) or per process (the forced grid) for
// the whole library: inline variables, so that every unit's entries write what fa_last_error,
// fa_last_launch and fa_set_reduce_grid (fa_reduce.hip) read.
inline thread_local std::string g_last_error;

inline int fail(int code, const char* what) {
  g_last_error = what;
  return code;
}

// fa_last_launch (ABI 16): what the calling thread's last fa_reduce_* / fa_fold* / fa_trim_sum / fa_gram_f32 / fa_rownorm2_f32 / fa_clip_sum_f32 / fa_clip_fold_f32 / fa_gauss_add_f32 / fa_deq_fold_q8 call launched.  A launch
// stores a pointer and two integers; the name is built once per instantiation (a static of its
// launch site, as resident_blocks_per_cu keeps its occupancy).
struct LaunchRecord {
  const char* kernel = nullptr;
  int64_t grid = 0;
  int32_t launches = 0;
};
inline thread_local LaunchRecord g_last_launch;

template <class P, typename T, auto... A>
struct Inst {};
template <class HP, auto... A>
struct HInst {};  // the float16 family has no T
template <class AT, typename T, auto... X>
struct FInst {};  // the naming tag: fold_finish_kernel<A,T,OP>
template <auto... A>
struct TInst {};  // the naming tags: trim_kernel_rows<NP,W,NT>, gram_kernel_tile<NP,CEN,NT>, rownorm_kernel / clip_sum_kernel / clip_fold_kernel / deq_fold_kernel<V,D,W,NT>, trim_kernel_elem<T>
template <class T>
struct EInst {};

// "family<P,T,args...>": the kernel's demangled symbol name without `fa::`, whitespace and the
// argument list.  FA_LAUNCH instantiates the kernel from the same argument list, every defaulted
// template argument spelled out, so the name cannot drift from what is launched.
inline std::string make_kernel_name(const char* family, const std::string& f) {
  // f: pretty_of<Inst<...>>(), "... [I = fa::host::Inst<fa::AccF32, float, 0, ...>]"
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

constexpr bool kNT = true;  // client bytes are read once: non-temporal

inline int device_cus() {
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

inline int launch_check() {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(FA_ERR_LAUNCH, hipGetErrorString(err));
  return FA_OK;
}

// fa_set_reduce_grid: 0 = the geometry (fa_geometry.hpp) chooses the grid
inline std::atomic<int> g_reduce_grid{0};

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

// The units' launchers turn a Plan (fa_geometry.hpp) into the template instantiation it names, one
// switch per kernel family.  They choose nothing: a plan value with no shipped instantiation is an
// error, never another kernel.
inline int no_kernel(const char* family) {
  return fail(FA_ERR_ARG, (std::string("no shipped ") + family + " instantiation for the plan").c_str());
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

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// [a, a + bytes) and [b, b + bytes) share a byte
inline bool overlaps(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// ncols: the columns the launch touches (0: unknown — only the exact-alias check applies)
template <typename T>
int make_epi(const fa_epilogue* in, double denom, int n_reduced, float* out32, double* out64, Epi<T>* e,
             int64_t ncols = 0) {
  e->denom = (T)denom;
  // the reciprocal quotient: double epilogues only (fp32 sums: kHasRecipQuot), and only where it is
  // the IEEE quotient bit for bit
  e->rq = sizeof(T) == 8 && recip_quot_exact(denom) ? 1 : 0;
  e->rdenom = e->rq ? 1.0 / denom : 0.0;
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
inline int check_columns(const float* out32, const double* out64, const void* prev, const void* v,
                  size_t v_elem, const float* h = nullptr) {
  if (!aligned_to(out32, 16) || !aligned_to(out64, 32) || !aligned_to(prev, 16) ||
      !aligned_to(v, 4 * v_elem) || !aligned_to(h, 16))
    return fail(FA_ERR_ALIGN, "output / prev / v / h arrays must be 4-element aligned");
  return FA_OK;
}

// What every fa_reduce_* entry checks first, in this order
inline int check_window(const void* stack, int64_t stride, int n, const void* w, int64_t col0, int64_t ncols,
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

}  // namespace host
}  // namespace fa
