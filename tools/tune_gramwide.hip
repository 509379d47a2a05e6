// tune_gramwide.hip — the wide Gram kernel's unit orders against each other (measurement tool, not a
// gate): panel_pair_kernel<false> launched directly with each order of fa_gramwide.hpp on one stack.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Iflearn_amd/csrc
//         tools/tune_gramwide.hip -o tools/tune_gramwide
//   tools/tune_gramwide [n_clients = 1000] [n_cols = 4194304] [reps = 10]
// Prints one line per order: the median and minimum time of `reps` launches after 2 warm-up ones, and
// the rate of the MFMA flop issued (active tiles only).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fa_gramwide.hpp"

#define CHECK(x)                                                                  \
  do {                                                                            \
    const hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

__global__ void fill_kernel(float* x, size_t count) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (float)((i * 2654435761u >> 8) & 0xffff) * (1.f / 65536.f) - 0.5f;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 1000, reps = argc > 3 ? std::atoi(argv[3]) : 10;
  const int64_t ncols = argc > 2 ? std::atoll(argv[2]) : 4194304;
  if (n <= fa::kGramMaxClients || n > fa::kGramWideMaxClients || ncols < 1 || ncols % 4 != 0 || reps < 1) return 2;
  int cus = 0;
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const fa::GramWidePlan p = fa::plan_gram_wide(n, ncols, cus, 0);
  float *stack = nullptr, *work = nullptr;
  CHECK(hipMalloc(&stack, (size_t)n * ncols * 4));
  CHECK(hipMalloc(&work, (size_t)p.workspace_bytes));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, stack, (size_t)n * ncols);
  CHECK(hipDeviceSynchronize());
  double tiles = 0;  // active 32 x 32 tiles over all pairs
  for (int I = 0; I < p.panels; ++I)
    for (int J = I; J < p.panels; ++J) {
      const int a = std::min(4, p.tiles - 4 * I), b = std::min(4, p.tiles - 4 * J);
      tiles += I == J ? a * (a + 1) / 2 : a * b;
    }
  const double flop = tiles * 32 * 32 * 2 * (double)(p.chunks * p.kc);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const char* names[] = {"slice-major, XCD-grouped", "slice-major", "pair-major"};
  for (int order = 0; order < 3; ++order) {
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; ++r) {
      CHECK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(fa::gramwide::panel_pair_kernel<false>, dim3((unsigned)(p.slices * p.pairs)), dim3(256), 0, 0,
                         stack, ncols, n, (const float*)nullptr, (int64_t)0, ncols, p.chunks, (int)p.slices, p.panels, order,
                         work);
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      float t = 0;
      CHECK(hipEventElapsedTime(&t, e0, e1));
      if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    std::printf("n=%d cols=%lld slices=%lld pairs=%d %-26s median %.3f ms min %.3f ms  %.1f TF/s issued\n", n,
                (long long)ncols, (long long)p.slices, p.pairs, names[order], ms[ms.size() / 2], ms[0],
                flop / (ms[ms.size() / 2] * 1e-3) / 1e12);
  }
  CHECK(hipFree(stack));
  CHECK(hipFree(work));
  return 0;
}
