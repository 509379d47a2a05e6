// tune_rows.hip — geometry sweep of the row-pointer (device-upload) reduce; TOOL, not product.
//
// Built as tools/libtune_rows.so (hipcc --offload-arch=gfx950 -O3 -fPIC -shared tools/tune_rows.hip -o tools/libtune_rows.so) and driven from Python
// (tools/tune_rows.py) with piece tables built there: the one-piece-per-claim kernel the product
// used before (fa_tune_device.hpp reduce_kernel_segrows, dynamic piece claiming) at several
// V / D / W, and the product kernel (fa_device.hpp reduce_kernel_segrows_rm, claimed row-major
// groups) at several V / W / KG.
// Earlier sweeps of this file (profiles/r02/tune_rows/) also held a column-major kernel with
// the row pointers prefetched one refill ahead (no gain).
#include <hip/hip_runtime.h>

#include "fa_tune_device.hpp"

namespace {
using namespace fa;

template <int V, int D, int W>
int launch(const float* const* rows, int n, const float* w, const fa_piece* pieces, int64_t npieces, int grid,
           int* work, const Epi<double>& e, hipStream_t s) {
  if (hipMemsetAsync(work, 0, sizeof(int), s) != hipSuccess) return -3;
  hipLaunchKernelGGL((reduce_kernel_segrows<AccF32, double, 0, V, D, W, true>), dim3((unsigned)grid), dim3(64 * W), 0, s,
                     rows, n, w, pieces, npieces, work, e);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

// variant -> (V, D, W) of reduce_kernel_segrows; the piece width is chosen by the caller
extern "C" int tune_rows_launch(int variant, const float* const* rows, int n, const float* w, const fa_piece* pieces,
                                int64_t npieces, int grid, int* work, double denom, float* out32, void* stream) {
  Epi<double> e{};
  e.denom = denom;
  e.out32 = out32;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (variant) {
    case 0: return launch<8, 2, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 1: return launch<16, 1, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 2: return launch<8, 1, 8>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 3: return launch<8, 2, 8>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 4: return launch<8, 4, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 5: return launch<4, 4, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 6: return launch<4, 2, 8>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 7: return launch<16, 2, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    default: return -1;
  }
}

// split-N variants (fa_device.hpp reduce_kernel_splitn<W, D>) on a [n, stride] stack
namespace {
template <int W, int D>
int launch_sn(const float* stack, int64_t stride, int n, const float* w, int64_t ncols, const Epi<double>& e,
              hipStream_t s) {
  const int64_t chunks = ((ncols + 3) / 4 + 63) / 64;
  hipLaunchKernelGGL((reduce_kernel_splitn<AccF32, double, 0, W, D, true>), dim3((unsigned)chunks), dim3(64 * W), 0,
                     s, stack, stride, n, w, (int64_t)0, ncols, e);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
}  // namespace

extern "C" int tune_splitn_launch(int variant, const float* stack, int64_t stride, int n, const float* w, int64_t ncols,
                                  double denom, float* out32, void* stream) {
  Epi<double> e{};
  e.denom = denom;
  e.out32 = out32;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (variant) {
    case 0: return launch_sn<4, 8>(stack, stride, n, w, ncols, e, s);
    case 1: return launch_sn<4, 16>(stack, stride, n, w, ncols, e, s);
    case 2: return launch_sn<8, 8>(stack, stride, n, w, ncols, e, s);
    case 3: return launch_sn<8, 16>(stack, stride, n, w, ncols, e, s);
    case 4: return launch_sn<16, 8>(stack, stride, n, w, ncols, e, s);
    case 5: return launch_sn<16, 4>(stack, stride, n, w, ncols, e, s);
    case 6: return launch_sn<2, 16>(stack, stride, n, w, ncols, e, s);
    case 7: return launch_sn<16, 16>(stack, stride, n, w, ncols, e, s);
    default: return -1;
  }
}

// probe: does a 16-B raw buffer load whose range covers only `bytes` (< 16) return the in-range
// dwords (per-dword range check) or nothing?  out[0..3] = the load at offset `off`
namespace {
__global__ void oob_probe_kernel(const float* src, uint32_t bytes, int off, float* out) {
  if (threadIdx.x == 0) {
    const vec4<float>::type v = buf_load_quad<true>(row_rsrc(src, bytes), off, 0);
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    out[3] = v[3];
  }
}
}  // namespace

extern "C" int tune_oob_probe(const float* src, uint32_t bytes, int off, float* out, void* stream) {
  hipLaunchKernelGGL(oob_probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), src, bytes, off, out);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// row-major grouped row-pointer kernel (fa_device.hpp reduce_kernel_segrows_rm<V, W, KG, DN>)
namespace {
template <int V, int W, int KG>
int launch_rm(const float* const* rows, int n, const float* w, const fa_piece* pieces, int64_t npieces, int grid,
              int* work, const Epi<double>& e, hipStream_t s) {
  if (hipMemsetAsync(work, 0, sizeof(int), s) != hipSuccess) return -3;
  hipLaunchKernelGGL((reduce_kernel_segrows_rm<AccF32, double, 0, V, W, KG, 16, true>), dim3((unsigned)grid),
                     dim3(64 * W), 0, s, rows, n, w, pieces, npieces, work, e);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
}  // namespace

extern "C" int tune_rows_rm_launch(int variant, const float* const* rows, int n, const float* w,
                                   const fa_piece* pieces, int64_t npieces, int grid, int* work, double denom,
                                   float* out32, void* stream) {
  Epi<double> e{};
  e.denom = denom;
  e.out32 = out32;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (variant) {
    case 0: return launch_rm<8, 8, 2>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 1: return launch_rm<8, 8, 3>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 2: return launch_rm<8, 8, 4>(rows, n, w, pieces, npieces, grid, work, e, s);
    case 3: return launch_rm<16, 4, 2>(rows, n, w, pieces, npieces, grid, work, e, s);
    default: return -1;
  }
}

// the product geometry (V8 W8 KG2, DN16) with per-claim wall-clock stamps (TR): trace[block*32+...]
extern "C" int tune_rows_rm_trace(const float* const* rows, int n, const float* w, const fa_piece* pieces,
                                  int64_t npieces, int grid, int* work, double denom, float* out32,
                                  unsigned long long* trace, void* stream) {
  Epi<double> e{};
  e.denom = denom;
  e.out32 = out32;
  e.trace = trace;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(work, 0, sizeof(int), s) != hipSuccess) return -3;
  hipLaunchKernelGGL((reduce_kernel_segrows_rm<AccF32, double, 0, 8, 8, 2, 16, true, true>), dim3((unsigned)grid),
                     dim3(512), 0, s, rows, n, w, pieces, npieces, work, e);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// fused FedAVGM through the product's row-pointer geometry (V8 W8 KG2, DN16), f64 state, with
// (xl = 1) or without whole-line f64 stores (round 5: tools/probe_rows_xl.py)
extern "C" int tune_rows_rm_avgm(int xl, const float* const* rows, int n, const float* w, const fa_piece* pieces,
                                 int64_t npieces, int grid, int* work, double denom, const float* prev, double* v,
                                 double* v_out, float* out32, void* stream) {
  Epi<double> e{};
  e.denom = denom;
  e.prev = prev;
  e.v = v;
  e.v_out = v_out;
  e.out32 = out32;
  e.beta = 0.9;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(work, 0, sizeof(int), s) != hipSuccess) return -3;
  if (xl)
    hipLaunchKernelGGL((reduce_kernel_segrows_rm<AccF32, double, FA_OP_AVGM, 8, 8, 2, 16, true, false, true>),
                       dim3((unsigned)grid), dim3(512), 0, s, rows, n, w, pieces, npieces, work, e);
  else
    hipLaunchKernelGGL((reduce_kernel_segrows_rm<AccF32, double, FA_OP_AVGM, 8, 8, 2, 16, true, false, false>),
                       dim3((unsigned)grid), dim3(512), 0, s, rows, n, w, pieces, npieces, work, e);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
