// MI355X (gfx950 / CDNA4) kernels of the GPU-share stack.  See gsx_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace {
thread_local std::string g_err;  // the library's one error text: every translation unit sets it through gsx::set_error
}  // namespace

namespace gsx __attribute__((visibility("hidden"))) {

void set_error(const char* what) { g_err = what; }

int fail(hipError_t e, const char* what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), static_cast<int>(e));
  set_error(buf);
  return static_cast<int>(e);
}

int fail_arg(const char* what) {
  set_error(what);
  return static_cast<int>(hipErrorInvalidValue);
}

int current_device(const char* who, int* dev) {
  GSX_CHECK(hipGetDevice(dev));
  if (*dev < 0 || *dev >= kMaxDevices) return fail_arg((std::string(who) + ": device index").c_str());
  return 0;
}

}  // namespace gsx

using namespace gsx;

namespace {

// ------------------------------------------------------------------ CU probe

__global__ __launch_bounds__(64) void cuprobe_kernel(uint32_t* out, int spin) {
  uint32_t hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  // keep the workgroup resident for a while so the dispatcher spreads the
  // grid over every CU the queue's mask allows
  float x = static_cast<float>(threadIdx.x);
  for (int i = 0; i < spin; ++i) x = __builtin_fmaf(x, 1.0000001f, 0.5f);
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = hw;
    out[2 * blockIdx.x + 1] = xcc | (x == -1.0f ? 0x80000000u : 0u);
  }
}

}  // namespace

extern "C" {

const char* gsx_last_error(void) { return g_err.c_str(); }

int gsx_device_count(int* n) {
  GSX_CHECK(hipGetDeviceCount(n));
  return 0;
}

int gsx_device_info(int dev, gsx_devinfo* out) {
  hipDeviceProp_t p;
  GSX_CHECK(hipGetDeviceProperties(&p, dev));
  std::memset(out, 0, sizeof(*out));
  std::snprintf(out->name, sizeof(out->name), "%s", p.name);
  std::snprintf(out->arch, sizeof(out->arch), "%s", p.gcnArchName);
  GSX_CHECK(hipDeviceGetPCIBusId(out->pci_bus_id, sizeof(out->pci_bus_id), dev));
  out->total_mem = p.totalGlobalMem;
  out->cu_count = p.multiProcessorCount;
  out->clock_khz = p.clockRate;
  out->wave_size = p.warpSize;
  out->lds_per_block = p.sharedMemPerBlock;
  return 0;
}

int gsx_mem_info(int dev, uint64_t* free_b, uint64_t* total_b) {
  GSX_CHECK(hipSetDevice(dev));
  size_t f = 0, t = 0;
  GSX_CHECK(hipMemGetInfo(&f, &t));
  *free_b = f;
  *total_b = t;
  return 0;
}

int gsx_set_device(int dev) {
  GSX_CHECK(hipSetDevice(dev));
  return 0;
}

int gsx_synchronize(int dev) {
  GSX_CHECK(hipSetDevice(dev));
  GSX_CHECK(hipDeviceSynchronize());
  return 0;
}

int gsx_stream_create(int dev, const uint32_t* cu_mask, int mask_words, void** stream) {
  GSX_CHECK(hipSetDevice(dev));
  hipStream_t s;
  if (mask_words > 0) {
    GSX_CHECK(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask_words), cu_mask));
  } else {
    GSX_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  *stream = s;
  return 0;
}

int gsx_stream_get_mask(void* stream, uint32_t* cu_mask, int mask_words) {
  GSX_CHECK(hipExtStreamGetCUMask(S(stream), static_cast<uint32_t>(mask_words), cu_mask));
  return 0;
}

int gsx_stream_destroy(void* stream) {
  GSX_CHECK(hipStreamDestroy(S(stream)));
  return 0;
}

int gsx_stream_sync(void* stream) {
  GSX_CHECK(hipStreamSynchronize(S(stream)));
  return 0;
}

int gsx_malloc(int dev, uint64_t bytes, void** ptr) {
  GSX_CHECK(hipSetDevice(dev));
  GSX_CHECK(hipMalloc(ptr, bytes));
  return 0;
}

int gsx_free(void* ptr) {
  GSX_CHECK(hipFree(ptr));
  return 0;
}

int gsx_memcpy_d2h(void* dst, const void* src, uint64_t bytes) {
  GSX_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int gsx_memcpy_h2d(void* dst, const void* src, uint64_t bytes) {
  GSX_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

int gsx_cuprobe(void* stream, int blocks, int spin, uint32_t* out_host) {
  if (blocks <= 0 || blocks > (1 << 20) || spin < 0) return fail_arg("gsx_cuprobe: bad blocks/spin");
  uint32_t* d = nullptr;
  GSX_CHECK(hipMallocAsync(reinterpret_cast<void**>(&d), sizeof(uint32_t) * 2 * blocks, S(stream)));
  hipLaunchKernelGGL(cuprobe_kernel, dim3(blocks), dim3(64), 0, S(stream), d, spin);
  GSX_CHECK(hipGetLastError());
  GSX_CHECK(hipMemcpyAsync(out_host, d, sizeof(uint32_t) * 2 * blocks, hipMemcpyDeviceToHost, S(stream)));
  GSX_CHECK(hipFreeAsync(d, S(stream)));
  GSX_CHECK(hipStreamSynchronize(S(stream)));
  return 0;
}

}  // extern "C"
