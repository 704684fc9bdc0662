// HBM pre-flight memory test for MI355X (gfx950): pattern write, check and moving-inversions passes at HBM
// bandwidth, and the scrub (gsx_hbm_fill), which is the SOLID write pass.  C ABI at the end of gsx_kernels.h; NumPy
// twin of the generator in ops/memtest.py.
//
// Every pass is one grid-stride launch: 16 B per lane (global_load / global_store_dwordx4), four independent
// accesses in flight per lane, grid sized from the CU count, 64-bit index math, no LDS, no scratch, no atomics.
// The expected data is never stored: a check regenerates it from (pattern, seed, invert, W), W = origin/16 + word
// index.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <mutex>

#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "mix64.h"

using namespace gsx;

namespace {

constexpr int kWrite = 0, kCheck = 1, kCheckRewrite = 2;
constexpr uint32_t kMaxErrs = GSX_MEMTEST_MAX_ERRS;

// What one launch reports, in pinned host memory.  Every wave of the grid has a header and kMaxErrs record slots
// of its own and writes them with plain stores: no wave waits for the host, and none contends with another.  (With
// one shared counter and shared slots, updated by system-scope atomics, a range that was bad throughout ran a
// 4 GiB check at 0.40 TB/s against 4.7 TB/s clean on MI355X: some 8000 waves' atomics on one host address
// serialise.)  The host zeroes the headers before the launch and merges headers and records after the sync.
struct alignas(16) WaveHead {
  unsigned long long bad;  // mismatching dwords this wave saw
  uint32_t flipped;        // OR of expected ^ actual over them
  uint32_t nrec;           // records it wrote: min(bad, kMaxErrs)
};
struct LaunchReport {
  WaveHead* heads;        // [waves]
  gsx_memtest_err* recs;  // [waves][kMaxErrs]
};
static_assert(sizeof(gsx_memtest_err) == 16 && sizeof(WaveHead) == 16, "a record or a header is one 16-B store");
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int PAT>
__device__ __forceinline__ uint4 gen_word(uint64_t W, uint32_t seed, uint64_t key, uint32_t inv) {
  uint4 v;
  const uint32_t lo = static_cast<uint32_t>(W), hi = static_cast<uint32_t>(W >> 32);
  if (PAT == GSX_MEMTEST_ADDR) {
    v = make_uint4(lo, hi, ~lo, ~hi);
  } else if (PAT == GSX_MEMTEST_SOLID) {
    v = make_uint4(seed, seed, seed, seed);
  } else if (PAT == GSX_MEMTEST_WALK) {
    const uint32_t b = 4u * lo + seed;  // only its low five bits matter
    v = make_uint4(1u << (b & 31u), 1u << ((b + 1u) & 31u), 1u << ((b + 2u) & 31u), 1u << ((b + 3u) & 31u));
  } else {
    const uint64_t a = random_half(W, 0, key), c = random_half(W, 1, key);
    v = make_uint4(static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(c),
                   static_cast<uint32_t>(c >> 32));
  }
  return make_uint4(v.x ^ inv, v.y ^ inv, v.z ^ inv, v.w ^ inv);
}

// A check reads every word once: the nontemporal hint keeps the sweep from displacing itself in the caches.  Measured
// on MI355X over 4 GiB, interleaved with the plain form: check 5.4 against 4.9 TB/s (RANDOM), 5.6 against 5.2 (ADDR).
// The same hint on the stores cost the write pass 6 % (4.8 against 5.1 TB/s), so stores stay plain.
__device__ __forceinline__ uint4 ld16(const uint4* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t bad_dwords(uint4 e, uint4 a) {
  return (e.x != a.x) + (e.y != a.y) + (e.z != a.z) + (e.w != a.w);
}

__device__ __forceinline__ uint32_t flipped_bits(uint4 e, uint4 a) {
  return (e.x ^ a.x) | (e.y ^ a.y) | (e.z ^ a.z) | (e.w ^ a.w);
}

__device__ __forceinline__ void put_err(gsx_memtest_err* recs, uint32_t slot, uint64_t off, uint32_t e, uint32_t a) {
  if (slot < kMaxErrs) {
    u32x4 r = {static_cast<uint32_t>(off), static_cast<uint32_t>(off >> 32), e, a};
    *reinterpret_cast<u32x4*>(&recs[slot]) = r;
  }
}

// the bad dwords of one word go to slots slot, slot+1, ...
__device__ __forceinline__ uint32_t put_word(gsx_memtest_err* recs, uint32_t slot, uint64_t off, uint4 e, uint4 a) {
  if (e.x != a.x) put_err(recs, slot++, off, e.x, a.x);
  if (e.y != a.y) put_err(recs, slot++, off + 4, e.y, a.y);
  if (e.z != a.z) put_err(recs, slot++, off + 8, e.z, a.z);
  if (e.w != a.w) put_err(recs, slot++, off + 12, e.w, a.w);
  return slot;
}

// what a wave has found so far in its sweep
struct Tally {
  uint32_t mine = 0;  // this lane's bad dwords
  uint32_t flip = 0;  // OR of expected ^ actual over them
  uint32_t nrec = 0;  // records the wave has written, the same in every lane
};

// One step of the sweep, called by a whole wave (every lane active: both loops of the kernel keep a wave together):
// the N words i, i + step, ... of a lane that is `live`; a lane that is not stays in with a count of zero.
// e[] and a[] are indexed by unrolled constants only, so they stay in registers.
template <int PAT, int MODE, int N>
__device__ __forceinline__ void sweep_step(uint4* __restrict__ p, uint64_t i, uint64_t step, bool live, uint64_t W0,
                                           uint32_t seed, uint64_t key, uint32_t inv, gsx_memtest_err* recs,
                                           Tally& t) {
  if (MODE == kWrite) {
    if (live) {
#pragma unroll
      for (int k = 0; k < N; ++k) p[i + k * step] = gen_word<PAT>(W0 + i + k * step, seed, key, inv);
    }
    return;
  }
  uint4 e[N], a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) e[k] = a[k] = make_uint4(0, 0, 0, 0);
  if (live) {
    // N independent 16-B loads in flight per lane, all issued before any expected word is generated
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = ld16(p + i + k * step);
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = gen_word<PAT>(W0 + i + k * step, seed, key, inv);
    if (MODE == kCheckRewrite) {  // the complement goes out whether or not the word was bad
#pragma unroll
      for (int k = 0; k < N; ++k) p[i + k * step] = make_uint4(~e[k].x, ~e[k].y, ~e[k].z, ~e[k].w);
    }
  }
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    c += bad_dwords(e[k], a[k]);
    t.flip |= flipped_bits(e[k], a[k]);
  }
  t.mine += c;
  if (t.nrec >= kMaxErrs || __ballot(c != 0) == 0) return;
  // The rare path: a lane of the wave saw a mismatch in this step and the wave's slots are not used up.  The lanes'
  // bad dwords take the wave's next slots in lane order.  A wave in a range that is bad throughout comes here once,
  // for 32 stores.
  const int lane = threadIdx.x & 63;
  uint32_t incl = c;  // inclusive prefix sum of the lanes' counts
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const uint32_t total = __shfl(incl, 63, 64);
  uint32_t slot = t.nrec + incl - c;
  if (c != 0 && slot < kMaxErrs) {
#pragma unroll
    for (int k = 0; k < N; ++k) slot = put_word(recs, slot, 16 * (W0 + i + k * step), e[k], a[k]);
  }
  t.nrec = t.nrec + total < kMaxErrs ? t.nrec + total : kMaxErrs;
}

// p[0, n16): the words W0 .. W0 + n16 - 1.  MODE kWrite stores the pattern; kCheck compares; kCheckRewrite
// compares and stores the complement of the expected word in the same pass (moving inversions).
template <int PAT, int MODE>
__global__ __launch_bounds__(256) void memtest_kernel(uint4* __restrict__ p, uint64_t n16, uint64_t W0, uint32_t seed,
                                                      uint32_t inv, LaunchReport rep) {
  const uint64_t key = seed_key(seed);
  uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t step = gridDim.x * 256ull;
  Tally t;
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  gsx_memtest_err* recs = MODE == kWrite ? nullptr : rep.recs + static_cast<uint64_t>(wave) * kMaxErrs;
  // a wave's 64 lanes hold consecutive words: the unrolled loop runs while the wave's last lane has four words left,
  // so the whole wave leaves it together
  for (uint64_t last = i + (63u - (threadIdx.x & 63u)); last + 3 * step < n16; last += 4 * step, i += 4 * step) {
    sweep_step<PAT, MODE, 4>(p, i, step, true, W0, seed, key, inv, recs, t);
  }
  // tail: the words left (four per lane in a wave that straddles the end of the unrolled range).  Lanes run out
  // at different trip counts, so those that are done stay in with a count of zero until the whole wave is
  for (;;) {
    const bool live = i < n16;
    if (__ballot(live) == 0) break;
    sweep_step<PAT, MODE, 1>(p, i, step, live, W0, seed, key, inv, recs, t);
    i += step;
  }
  if (MODE != kWrite) {
    // wave64 reduction over the whole grid-stride loop: one counter update per wave and launch, and none from a
    // wave that saw no mismatch (a lane's own count fits 32 bits: it reads a 1/2^19th of the range on MI355X)
    unsigned long long bad = t.mine;
    uint32_t flip = t.flip;
    for (int o = 32; o > 0; o >>= 1) {
      bad += __shfl_xor(bad, o, 64);
      flip |= __shfl_xor(flip, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && bad) {
      u32x4 h = {static_cast<uint32_t>(bad), static_cast<uint32_t>(bad >> 32), flip, t.nrec};
      *reinterpret_cast<u32x4*>(&rep.heads[wave]) = h;
    }
  }
}

std::mutex g_mu;
LaunchReport g_rep[kMaxDevices] = {};  // pinned, device-visible; one per device, for the largest grid (8 blocks / CU)
int g_cus[kMaxDevices] = {0};
std::mutex g_dev_mu[kMaxDevices];  // its own, not the stamp counter's: a memory test never waits for an admission

// the current device, its CU count and its pinned launch report
int device_state(int* dev, int* cus, LaunchReport* rep) {
  if (int rc = current_device("gsx_memtest", dev)) return rc;
  std::lock_guard<std::mutex> g(g_mu);
  if (!g_cus[*dev]) {
    int n = 0;
    GSX_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, *dev));
    g_cus[*dev] = n > 0 ? n : 1;
  }
  if (rep && !g_rep[*dev].recs) {
    const size_t waves = static_cast<size_t>(g_cus[*dev]) * 8 * 4;
    GSX_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g_rep[*dev].heads), waves * sizeof(WaveHead),
                            hipHostMallocCoherent));
    GSX_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g_rep[*dev].recs), waves * kMaxErrs * sizeof(gsx_memtest_err),
                            hipHostMallocCoherent));
  }
  *cus = g_cus[*dev];
  if (rep) *rep = g_rep[*dev];
  return 0;
}

// 1024 words per block until the grid reaches 8 blocks per CU (four words per lane: the unrolled loop runs from
// 16 KiB up), the grid-stride loop from there
int grid_for(uint64_t n16, int cus) {
  const uint64_t cap = static_cast<uint64_t>(cus) * 8;
  const uint64_t g = (n16 + 1023) / 1024;
  return static_cast<int>(g > cap ? cap : (g < 1 ? 1 : g));
}

// the kernels, kKernels[pattern][mode]: one row per GSX_MEMTEST_* pattern, its columns kWrite, kCheck, kCheckRewrite
using Kernel = void (*)(uint4*, uint64_t, uint64_t, uint32_t, uint32_t, LaunchReport);
template <int PAT>
constexpr Kernel kRow[] = {memtest_kernel<PAT, kWrite>, memtest_kernel<PAT, kCheck>, memtest_kernel<PAT, kCheckRewrite>};
constexpr const Kernel* kKernels[] = {kRow<GSX_MEMTEST_ADDR>, kRow<GSX_MEMTEST_SOLID>, kRow<GSX_MEMTEST_WALK>,
                                      kRow<GSX_MEMTEST_RANDOM>};
constexpr int kPatterns = sizeof(kKernels) / sizeof(kKernels[0]);
static_assert(GSX_MEMTEST_ADDR == 0 && GSX_MEMTEST_SOLID == 1 && GSX_MEMTEST_WALK == 2 && GSX_MEMTEST_RANDOM == 3,
              "kKernels is indexed by the pattern's value");

int launch(int mode, hipStream_t st, int grid, int pattern, uint4* p, uint64_t n16, uint64_t W0, uint32_t seed,
           uint32_t inv, LaunchReport rep) {
  if (pattern < 0 || pattern >= kPatterns) return fail_arg("gsx_memtest: unknown pattern");
  hipLaunchKernelGGL(kKernels[pattern][mode], dim3(grid), dim3(256), 0, st, p, n16, W0, seed, inv, rep);
  GSX_CHECK(hipGetLastError());
  return 0;
}

const char* check_range(const void* base, uint64_t bytes, uint64_t origin) {
  if (!base || reinterpret_cast<uintptr_t>(base) % 16) return "gsx_memtest: base not 16-B aligned";
  if (bytes % 16 || origin % 16) return "gsx_memtest: bytes and origin must be multiples of 16";
  if (origin + bytes < origin) return "gsx_memtest: origin + bytes wraps";
  return nullptr;
}

}  // namespace

extern "C" {

int gsx_memtest_write(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert) {
  if (const char* why = check_range(base, bytes, origin)) return fail_arg(why);
  if (!bytes) return 0;
  int dev = 0, cus = 0;
  if (int rc = device_state(&dev, &cus, nullptr)) return rc;
  return launch(kWrite, S(stream), grid_for(bytes / 16, cus), pattern, static_cast<uint4*>(base), bytes / 16,
                origin / 16, seed, invert ? 0xFFFFFFFFu : 0u, LaunchReport{});
}

// the scrub: the SOLID write pass with the pattern as its seed; no report, so neither pinned memory nor a mutex
int gsx_hbm_fill(void* stream, void* base, uint64_t bytes, uint32_t pattern) {
  if (!base || bytes % 16 || reinterpret_cast<uintptr_t>(base) % 16) return fail_arg("gsx_hbm_fill: need 16-B multiple");
  if (!bytes) return 0;
  int dev = 0, cus = 0;
  if (int rc = device_state(&dev, &cus, nullptr)) return rc;
  return launch(kWrite, S(stream), grid_for(bytes / 16, cus), GSX_MEMTEST_SOLID, static_cast<uint4*>(base), bytes / 16,
                0, pattern, 0, LaunchReport{});
}

int gsx_memtest_check(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert, int rewrite, gsx_memtest_report* report) {
  if (!report) return fail_arg("gsx_memtest_check: no report");
  if (const char* why = check_range(base, bytes, origin)) return fail_arg(why);
  if (!bytes) return 0;
  int dev = 0, cus = 0;
  LaunchReport rep{};
  if (int rc = device_state(&dev, &cus, &rep)) return rc;
  hipStream_t st = S(stream);
  // reset -> launch -> read back under the device's mutex: concurrent callers never mix their reports
  std::lock_guard<std::mutex> dl(g_dev_mu[dev]);
  const int grid = grid_for(bytes / 16, cus);
  const size_t waves = static_cast<size_t>(grid) * 4;
  std::memset(rep.heads, 0, waves * sizeof(WaveHead));
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  const uint32_t inv = invert ? 0xFFFFFFFFu : 0u;
  if (int rc = launch(rewrite ? kCheckRewrite : kCheck, st, grid, pattern, static_cast<uint4*>(base), bytes / 16,
                      origin / 16, seed, inv, rep))
    return rc;
  GSX_CHECK(hipStreamSynchronize(st));
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  for (size_t w = 0; w < waves; ++w) {
    const WaveHead h = rep.heads[w];
    if (!h.bad) continue;
    report->bad_dwords += h.bad;
    report->flipped_or |= h.flipped;
    const uint32_t got = h.nrec < kMaxErrs ? h.nrec : kMaxErrs;
    for (uint32_t k = 0; k < got && report->n_errs < kMaxErrs; ++k)
      report->errs[report->n_errs++] = rep.recs[w * kMaxErrs + k];
  }
  return 0;
}

int gsx_memtest_pass(int level, uint32_t idx, gsx_memtest_pass_t* out) {
  if (level != GSX_MEMTEST_QUICK && level != GSX_MEMTEST_FULL) return -1;
  // triples {write, check + rewrite (the complement is now in memory), check the complement} of (pattern, seed)
  static const uint32_t solid[] = {0u, 0xFFFFFFFFu, 0x55555555u, 0xAAAAAAAAu};
  const uint32_t triple = idx / 3, step = idx % 3;
  const uint32_t triples = level == GSX_MEMTEST_FULL ? 2 + 4 + 32 : 2;
  if (triple >= triples) return 1;
  if (triple == 0) {
    out->pattern = GSX_MEMTEST_ADDR, out->seed = 0;
  } else if (triple == 1) {
    out->pattern = GSX_MEMTEST_RANDOM, out->seed = 0;
  } else if (triple < 6) {
    out->pattern = GSX_MEMTEST_SOLID, out->seed = solid[triple - 2];
  } else {
    out->pattern = GSX_MEMTEST_WALK, out->seed = triple - 6;
  }
  out->write = step == 0;
  out->rewrite = step == 1;
  out->invert = step == 2;
  return 0;
}

int gsx_memtest_run(void* stream, void* base, uint64_t bytes, uint64_t origin, int level, gsx_memtest_report* report,
                    uint32_t* passes_out, double* seconds_out) {
  uint32_t passes = 0;
  uint64_t moved = 0;
  bool truncated = false;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = memtest_run(stream, base, bytes, origin, level, MemtestOpts{}, report, &passes, &moved, &truncated);
  if (passes_out) *passes_out = passes;
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

}  // extern "C"

namespace gsx __attribute__((visibility("hidden"))) {

int memtest_run(void* stream, void* base, uint64_t bytes, uint64_t origin, int level, const MemtestOpts& opts,
                gsx_memtest_report* report, uint32_t* passes, uint64_t* bytes_moved, bool* truncated) {
  if (level != GSX_MEMTEST_QUICK && level != GSX_MEMTEST_FULL) return fail_arg("gsx_memtest_run: unknown level");
  if (!report) return fail_arg("gsx_memtest_run: no report");
  if (opts.flip_mask && (opts.flip_offset % 4 || opts.flip_offset >= bytes))
    return fail_arg("gsx_memtest_run: the dword to flip is outside the range");
  uint32_t flip = opts.flip_mask;
  gsx_memtest_pass_t ps;
  for (uint32_t k = 0; gsx_memtest_pass(level, k, &ps) == 0; ++k) {
    if (opts.deadline && std::chrono::steady_clock::now() >= *opts.deadline) {
      *truncated = true;
      break;
    }
    int rc;
    if (ps.write) {
      rc = gsx_memtest_write(stream, base, bytes, origin, ps.pattern, ps.seed, ps.invert);
      if (!rc && flip) {
        // one dword of the caller's own buffer, flipped through the host: a data mismatch for the check to find
        uint32_t w = 0;
        char* at = static_cast<char*>(base) + opts.flip_offset;
        if (hipStreamSynchronize(S(stream)) != hipSuccess || hipMemcpy(&w, at, 4, hipMemcpyDeviceToHost) != hipSuccess)
          return fail_arg("--inject: reading the dword failed");
        w ^= flip;
        flip = 0;
        if (hipMemcpy(at, &w, 4, hipMemcpyHostToDevice) != hipSuccess)
          return fail_arg("--inject: writing the dword failed");
      }
    } else {
      rc = gsx_memtest_check(stream, base, bytes, origin, ps.pattern, ps.seed, ps.invert, ps.rewrite, report);
    }
    if (rc) return rc;
    ++*passes;
    *bytes_moved += bytes * (ps.rewrite ? 2 : 1);
  }
  return 0;
}

}  // namespace gsx
