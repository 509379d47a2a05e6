// fa_noise.hip — the Gaussian-noise entry of the C ABI (include/flearn_amd.h): fa_gauss_add_f32
// (fa_noise.hpp: counter-based normals added to an FA_ACC_F32 accumulator, the noise step of a
// DP-FedAvg round).  Host side only, as fa_clip.hip; a unit of its own so that it compiles beside
// the others and no existing kernel shares a unit with it.
#include <cmath>
#include <string>

#include "fa_geometry.hpp"
#include "fa_host.hpp"
#include "fa_noise.hpp"

static_assert(fa::kNoiseBlock == fa::noise::kNoiseThreads, "the plan's block is the kernel's");

extern "C" {

int fa_gauss_add_f32(float* acc, int64_t col_begin, int64_t n_cols, float sigma, uint64_t seed, uint64_t sequence,
                     void* stream) {
  using namespace fa;
  using namespace fa::host;
  g_last_launch = LaunchRecord{};
  if (n_cols < 0 || col_begin < 0) return fail(FA_ERR_ARG, "bad column window (col_begin and n_cols must be >= 0)");
  if (!acc && n_cols > 0) return fail(FA_ERR_ARG, "null acc");
  if (!(sigma >= 0.f) || std::isinf(sigma)) return fail(FA_ERR_ARG, "sigma must be finite and >= 0");
  if (!aligned_to(acc, 16) || col_begin % 4 != 0)
    return fail(FA_ERR_ALIGN, "acc must be 16-B aligned and col_begin a multiple of 4");
  if (n_cols == 0 || sigma == 0.f) return FA_OK;  // nothing launched: the accumulator's bits stay
  const NoisePlan p = plan_gauss_add(n_cols, device_cus(), g_reduce_grid.load(std::memory_order_relaxed));
  hipLaunchKernelGGL(noise::gauss_add_kernel, dim3((unsigned)p.grid), dim3(noise::kNoiseThreads), 0,
                     static_cast<hipStream_t>(stream), acc, col_begin / 4, n_cols, sigma, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)sequence, (uint32_t)(sequence >> 32));
  static const std::string name_ = "gauss_add_kernel";
  note_launch(name_, p.grid);
  return launch_check();
}

}  // extern "C"
