// Host-side helpers shared by the translation units of libgsx_kernels.so and by the tools that link the same
// objects.  Internal: not part of the C ABI (gsx_kernels.h), and hidden, so none of it shows among the library's
// exported symbols.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>

#include "gsx_kernels.h"

namespace gsx __attribute__((visibility("hidden"))) {

constexpr int kMaxDevices = 64;  // per-device state is indexed by the HIP device index

// The text gsx_last_error() returns on this thread; the string itself lives in gsx_kernels.hip.
void set_error(const char* what);
int fail(hipError_t e, const char* what);  // "<what>: <hip error string> (<code>)"; returns e
int fail_arg(const char* what);            // returns hipErrorInvalidValue

// The calling thread's current device, checked against kMaxDevices; a failure's text begins with `who`.
int current_device(const char* who, int* dev);

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The run loops of the two pre-flight tests.  gsx_cutest_run and gsx_memtest_run are these with no option set; the
// operator tools (tool_cutest.hip, tool_memtest.hip), which link the library's objects, set them.

struct CutestOpts {
  const gsx_cutest_inject* inject = nullptr;  // passed on to every launch
  double max_seconds = 0;  // > 0: a budget from the start of the run, looked at before every launch
};
// As gsx_cutest_run.  A run that its budget ends sets *truncated and is no error; report->launches counts completed
// launches, and cus_expected and covered are set however the run ends.
int cutest_run(void* stream, int level, uint32_t expect_cus, const CutestOpts& opts, gsx_cutest_report* report,
               double* seconds, bool* truncated);

struct MemtestOpts {
  const std::chrono::steady_clock::time_point* deadline = nullptr;  // looked at before every pass
  // flip_mask != 0: after the first write pass the dword at base + flip_offset is XORed with it, through a host copy
  uint64_t flip_offset = 0;
  uint32_t flip_mask = 0;
};
// As gsx_memtest_run, for one range.  *passes and *bytes_moved ACCUMULATE, as *report does: completed passes and
// what they read and wrote.  A run that its deadline ends sets *truncated and is no error.
int memtest_run(void* stream, void* base, uint64_t bytes, uint64_t origin, int level, const MemtestOpts& opts,
                gsx_memtest_report* report, uint32_t* passes, uint64_t* bytes_moved, bool* truncated);

}  // namespace gsx

#define GSX_CHECK(call)                                  \
  do {                                                   \
    hipError_t _e = (call);                              \
    if (_e != hipSuccess) return ::gsx::fail(_e, #call); \
  } while (0)
