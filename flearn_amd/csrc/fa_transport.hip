// fa_transport.hip — the entries of the C ABI (include/flearn_amd.h) that launch no reduce: copies
// and pushes by kernel (fa_transport.hpp) or copy engine, cache fences, stream joins, IPC handles,
// device allocations and the benchmark's fill.  Host side only; of fa_host.hpp it needs the error
// state and launch_check.
#include <cstring>

#include "fa_host.hpp"
#include "fa_transport.hpp"

using namespace fa;
using namespace fa::host;

extern "C" {

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
