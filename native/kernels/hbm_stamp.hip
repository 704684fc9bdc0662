// HBM stamps for MI355X (gfx950): a pod's slice is stamped with {tag, offset} every `stride` bytes when it is
// admitted, and every resident slice is verified by counting its bad stamps.  C ABI in gsx_kernels.h.
//
// Two device helpers (stamp an extent, count an extent's bad stamps), two kernels over a table of extents
// (grid.y = extent), one host launcher; a single range is a table of one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "gsx_internal.h"
#include "gsx_kernels.h"

using namespace gsx;

namespace {

// 16-B aligned: one dwordx4 load / store per stamp.  With 8-B alignment the compiler split each access into two
// dwordx2, and both halves of a stamp missed L2 together: two DRAM reads per stamp (rocprofv3 PMC,
// profiles/r02_pmc_admit/)
struct alignas(16) Stamp {
  uint64_t tag;
  uint64_t off;
};
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));  // a stamp read as one 16-B vector

typedef const __attribute__((address_space(1))) u64x2* global_stamp_ptr;  // slice addresses are device memory

typedef __attribute__((address_space(1))) u64x2* global_stamp_wptr;

__device__ __forceinline__ u64x2 load_stamp(const char* p) { return *(global_stamp_ptr)(p); }
__device__ __forceinline__ void store_stamp(char* p, uint64_t tag, uint64_t off) {
  u64x2 v;
  v.x = tag;
  v.y = off;
  *(global_stamp_wptr)(p) = v;  // one global_store_dwordx4
}

// The blocks of one grid row (gridDim.x of 256 lanes) stride over the stamp positions of one extent.
__device__ __forceinline__ void stamp_extent(const gsx_slice sl, uint64_t stride) {
  const uint64_t n = sl.bytes / stride;
  char* base = reinterpret_cast<char*>(sl.addr);
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    store_stamp(base + i * stride, sl.tag, i * stride);
  }
}

// Adds the extent's bad stamps to *bad (pinned host memory): wave64 reduction, then one system-scope atomic per
// wave that saw a mismatch.
__device__ __forceinline__ void count_bad_stamps(const gsx_slice sl, uint64_t stride, unsigned long long* bad) {
  const uint64_t n = sl.bytes / stride;
  const char* base = reinterpret_cast<const char*>(sl.addr);
  uint32_t mine = 0;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const u64x2 st = load_stamp(base + i * stride);
    mine += (st.x != sl.tag || st.y != i * stride) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd_system(bad, static_cast<unsigned long long>(mine));
}

constexpr int kMaxSlices = 32;
struct SliceTable {
  gsx_slice s[kMaxSlices];
  int n;
};

__global__ __launch_bounds__(256) void stamp_slices_kernel(SliceTable t, uint64_t stride) {
  stamp_extent(t.s[blockIdx.y], stride);
}

__global__ __launch_bounds__(256) void verify_slices_kernel(SliceTable t, uint64_t stride, unsigned long long* bad) {
  count_bad_stamps(t.s[blockIdx.y], stride, bad);
}

// Stamp and verify stay two launches.  One fused launch (stamp rows and verify rows in one grid) was measured: it
// was not faster in the wall-clock of an admission, and it cannot verify the stamps it has just written, because the
// rows of one launch are unordered (profiles/r02_fused_admit/).

// One bad-stamp counter per device, in pinned host memory the kernels add to directly: no memset, no copy, and one
// stream sync per count.  Its reset -> kernel launch -> readback sequence is held under the device's mutex, so
// concurrent callers on one device (e.g. two Python threads) never mix their counts.
std::mutex g_mu;
unsigned long long* g_host_counter[kMaxDevices] = {nullptr};
std::mutex g_dev_mu[kMaxDevices];

int pinned_counter(const char* who, int* dev, unsigned long long** hc) {
  if (int rc = current_device(who, dev)) return rc;
  std::lock_guard<std::mutex> g(g_mu);
  if (!g_host_counter[*dev]) {
    GSX_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g_host_counter[*dev]), 64, hipHostMallocCoherent));
  }
  *hc = g_host_counter[*dev];
  return 0;
}

// Grid caps, in blocks of 256 lanes per extent.  A table row gets one stamp per lane up to 1024 blocks.  Measured
// on MI355X: verifying 4 x 64 GiB at a 1 MiB stride takes ~12 us with 64 or with 1024 blocks per slice -- every read
// opens its own DRAM page and TLB entry, so translation, not per-lane latency, bounds it
// (profiles/r01_session7_gpu.md).  A single range (gsx_hbm_stamp / gsx_hbm_verify) gets up to 8192.
constexpr int kTableBlocks = 1024, kRangeBlocks = 8192;

// The one launcher: stamps slices[0, n_stamp), then counts the bad stamps of slices[0, n_verify) into *bad.
// Extents go out in tables of kMaxSlices, each launch's grid.x sized from the largest extent of its table.
// n_verify == 0 launches the stamps only, and synchronises only where `sync` asks; otherwise reset -> launches ->
// one sync -> read of the device's counter run under the device's mutex.
int launch(const char* who, hipStream_t st, const gsx_slice* slices, int n_stamp, int n_verify, uint64_t stride,
           int max_blocks, bool sync, uint64_t* bad) {
  auto tables = [&](int count, auto&& kernel) {
    for (int from = 0; from < count; from += kMaxSlices) {
      SliceTable t;
      t.n = std::min(kMaxSlices, count - from);
      uint64_t maxn = 0;
      for (int i = 0; i < t.n; ++i) {
        t.s[i] = slices[from + i];
        maxn = std::max<uint64_t>(maxn, t.s[i].bytes / stride);
      }
      const uint64_t gx = std::clamp<uint64_t>((maxn + 255) / 256, 1, max_blocks);
      kernel(dim3(static_cast<uint32_t>(gx), t.n), t);
      GSX_CHECK(hipGetLastError());
    }
    return 0;
  };
  if (int rc = tables(n_stamp, [&](dim3 grid, const SliceTable& t) {
        hipLaunchKernelGGL(stamp_slices_kernel, grid, dim3(256), 0, st, t, stride);
      }))
    return rc;
  if (!n_verify) {
    if (sync) GSX_CHECK(hipStreamSynchronize(st));
    return 0;
  }
  int dev = 0;
  unsigned long long* hc = nullptr;
  if (int rc = pinned_counter(who, &dev, &hc)) return rc;
  std::lock_guard<std::mutex> dl(g_dev_mu[dev]);
  __atomic_store_n(hc, 0ull, __ATOMIC_SEQ_CST);
  if (int rc = tables(n_verify, [&](dim3 grid, const SliceTable& t) {
        hipLaunchKernelGGL(verify_slices_kernel, grid, dim3(256), 0, st, t, stride, hc);
      }))
    return rc;
  GSX_CHECK(hipStreamSynchronize(st));
  *bad = __atomic_load_n(hc, __ATOMIC_SEQ_CST);
  return 0;
}

}  // namespace

extern "C" {

int gsx_hbm_stamp(void* stream, void* base, uint64_t bytes, uint64_t stride, uint64_t tag) {
  if (!base || stride < sizeof(Stamp) || stride % 16) return fail_arg("gsx_hbm_stamp: stride must be >=16, %16");
  if (reinterpret_cast<uintptr_t>(base) % 16) return fail_arg("gsx_hbm_stamp: base not 16-B aligned");
  if (bytes < stride) return 0;
  const gsx_slice sl = {reinterpret_cast<uintptr_t>(base), bytes, tag};
  return launch("gsx_hbm_stamp", S(stream), &sl, 1, 0, stride, kRangeBlocks, false, nullptr);
}

int gsx_hbm_verify(void* stream, const void* base, uint64_t bytes, uint64_t stride, uint64_t tag, uint64_t* bad) {
  if (!base || stride < sizeof(Stamp) || stride % 16) return fail_arg("gsx_hbm_verify: stride must be >=16, %16");
  if (reinterpret_cast<uintptr_t>(base) % 16) return fail_arg("gsx_hbm_verify: base not 16-B aligned");
  *bad = 0;
  if (bytes < stride) return 0;
  const gsx_slice sl = {reinterpret_cast<uintptr_t>(base), bytes, tag};
  return launch("gsx_hbm_verify", S(stream), &sl, 0, 1, stride, kRangeBlocks, true, bad);
}

int gsx_hbm_admit_n(void* stream, const gsx_slice* slices, int n, int n_stamp, int verify, uint64_t stride,
                    uint64_t* bad) {
  *bad = 0;
  if (n < 0 || n_stamp < 0 || n_stamp > n || stride < sizeof(Stamp) || stride % 16)
    return fail_arg("gsx_hbm_admit_n: bad n/n_stamp/stride");
  for (int i = 0; i < n; ++i) {
    if (!slices[i].addr || slices[i].addr % 16) return fail_arg("gsx_hbm_admit_n: slice base not 16-B aligned");
  }
  return launch("gsx_hbm_admit_n", S(stream), slices, n_stamp, verify ? n : 0, stride, kTableBlocks, true, bad);
}

}  // extern "C"
