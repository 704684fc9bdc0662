// Host-side helpers shared by the translation units of libgsx_kernels.so.  Internal: not part of the C ABI
// (gsx_kernels.h), and hidden, so none of it shows among the library's exported symbols.
#pragma once

#include <hip/hip_runtime.h>

namespace gsx __attribute__((visibility("hidden"))) {

constexpr int kMaxDevices = 64;  // per-device state is indexed by the HIP device index

// The text gsx_last_error() returns on this thread; the string itself lives in gsx_kernels.hip.
void set_error(const char* what);
int fail(hipError_t e, const char* what);  // "<what>: <hip error string> (<code>)"; returns e
int fail_arg(const char* what);            // returns hipErrorInvalidValue

// The calling thread's current device, checked against kMaxDevices; a failure's text begins with `who`.
int current_device(const char* who, int* dev);

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace gsx

#define GSX_CHECK(call)                                  \
  do {                                                   \
    hipError_t _e = (call);                              \
    if (_e != hipSuccess) return ::gsx::fail(_e, #call); \
  } while (0)
