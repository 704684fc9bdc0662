// C ABI of libgsx_kernels.so: the MI355X (gfx950) device-side pieces of the
// GPU-share stack.  The reference has no GPU code at all;
// these are new capabilities that make the shares verifiable on hardware:
//
//  * CU probe            — every workgroup records the hardware XCC / SE / CU /
//                          SIMD it ran on (s_getreg HW_ID, XCC_ID), so a CU
//                          mask (the MPS stand-in of BASELINE.json) can be
//                          checked against what the hardware actually used;
//  * HBM stamp / verify  — a pod's gpu-mem slice is stamped with its tag and
//                          verified later: proves co-resident pods placed by
//                          the binpack allocator really fit and never overlap
//                          (hbm_stamp.hip);
//  * HBM scrub           — the memory test's SOLID write pass, used to wipe a slice
//                          when a pod leaves (and as the HBM roofline probe);
//  * HBM memory test     — pattern write / check / moving-inversions passes at HBM
//                          bandwidth: the device plugin's pre-flight (memtest.hip);
//  * bf16 MFMA GEMM      — the pod workload used to measure isolation
//                          (throughput under per-pod CU partitions);
//  * CU-masked streams   — hipExtStreamCreateWithCUMask.
//
// All functions return 0 or a hipError_t value; gsx_last_error() has text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  char name[64];
  char arch[32];
  char pci_bus_id[32];
  uint64_t total_mem;
  int32_t cu_count;
  int32_t xcc_count;  // not reported by HIP; filled from the probe by callers
  int32_t clock_khz;
  int32_t wave_size;
  uint64_t lds_per_block;
} gsx_devinfo;

const char* gsx_last_error(void);
int gsx_device_count(int* n);
int gsx_device_info(int dev, gsx_devinfo* out);
int gsx_mem_info(int dev, uint64_t* free_b, uint64_t* total_b);
int gsx_synchronize(int dev);
// Make `dev` current on the calling thread (native runtime threads launch admission kernels).
int gsx_set_device(int dev);

// streams (mask_words == 0: plain stream)
int gsx_stream_create(int dev, const uint32_t* cu_mask, int mask_words, void** stream);
int gsx_stream_get_mask(void* stream, uint32_t* cu_mask, int mask_words);
int gsx_stream_destroy(void* stream);
int gsx_stream_sync(void* stream);

// memory
int gsx_malloc(int dev, uint64_t bytes, void** ptr);
int gsx_free(void* ptr);
int gsx_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int gsx_memcpy_h2d(void* dst, const void* src, uint64_t bytes);

// CU probe: `blocks` workgroups of 64 threads each spin `spin` iterations and
// record (HW_ID, XCC_ID) into out[2*b] / out[2*b+1].  Runs on `stream`
// (may be a CU-masked stream) and synchronises it.
int gsx_cuprobe(void* stream, int blocks, int spin, uint32_t* out_host);

// HBM stamp/verify (hbm_stamp.hip): 16-byte stamps {tag, offset} every `stride` bytes of
// [base, base+bytes).  stamp launches and returns without synchronising; verify returns the
// number of bad stamps in *bad after one stream sync.
int gsx_hbm_stamp(void* stream, void* base, uint64_t bytes, uint64_t stride, uint64_t tag);
int gsx_hbm_verify(void* stream, const void* base, uint64_t bytes, uint64_t stride, uint64_t tag, uint64_t* bad);
// Batched pod admission.  A pod is made of one or several extents (its slice is not contiguous when the arena
// is fragmented): stamp slices[0, n_stamp), then (verify != 0) verify all n slices, each in one launch per 32
// extents; *bad = total bad stamps.  The bad-stamp counter lives in pinned host memory, so there is no memset /
// copy kernel and exactly one stream sync per call.
typedef struct {
  uint64_t addr;
  uint64_t bytes;
  uint64_t tag;
} gsx_slice;
int gsx_hbm_admit_n(void* stream, const gsx_slice* slices, int n, int n_stamp, int verify, uint64_t stride,
                    uint64_t* bad);

// Fill [base, base+bytes) with a 32-bit pattern (bytes % 16 == 0): gsx_memtest_write's SOLID pass (memtest.hip).
int gsx_hbm_fill(void* stream, void* base, uint64_t bytes, uint32_t pattern);

// bf16 GEMM (gemm.hip): C[M][N] (bf16) = A[M][K] (bf16, row-major) * B[N][K]^T (bf16, row-major), fp32 accumulate.
// A, B and C are 16-B aligned.  Launches on `stream` and returns without synchronising.
// gsx_gemm_bf16_nt requires M % 128 == 0, N % 128 == 0, K % 64 == 0 and dispatches to one of the configurations
// below: the phased 256x256 kernel when M and N are multiples of 256, the grouped 128x128 tile otherwise.
int gsx_gemm_bf16_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K);
// The configurations, one table in gemm.hip: index 0 .. 10, each a kernel with a BM x BN block tile and a name
// ("256x256/8w-phased-g4"); most are ablations kept for benchmarking.  _cfg_name returns NULL and _cfg_tile
// nonzero outside the table.  _launch_cfg launches configuration `cfg`, which requires M % BM == 0, N % BN == 0,
// K % 64 == 0.
const char* gsx_gemm_cfg_name(int cfg);
int gsx_gemm_cfg_tile(int cfg, int* bm, int* bn);
int gsx_gemm_bf16_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int cfg);

// elapsed milliseconds of `iters` back-to-back gsx_gemm_bf16_nt on `stream`, by hip events (for benches)
int gsx_event_time_gemm(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int iters,
                        float* ms);

// HBM pre-flight memory test (memtest.hip).  The expected content of 16-byte word W = origin/16 + word index is
// generated from (pattern, seed, invert, W) and never stored; `origin` is the byte offset of `base` in the whole
// tested range, so a range tested chunk by chunk keeps globally unique content.
//   ADDR    dwords {lo32(W), hi32(W), ~lo32(W), ~hi32(W)}
//   SOLID   every dword = seed
//   WALK    dword j = 1u << ((4*W + j + seed) & 31)
//   RANDOM  two 64-bit outputs of a counter-based mixer (splitmix64's output function) of 2*W + half and seed
// invert != 0 complements all four dwords.  bytes and origin are multiples of 16; base is 16-B aligned.
enum { GSX_MEMTEST_ADDR = 0, GSX_MEMTEST_SOLID = 1, GSX_MEMTEST_WALK = 2, GSX_MEMTEST_RANDOM = 3 };
enum { GSX_MEMTEST_QUICK = 0, GSX_MEMTEST_FULL = 1 };
typedef struct {
  uint64_t offset;  // origin + byte offset of the dword
  uint32_t expected, actual;
} gsx_memtest_err;
#define GSX_MEMTEST_MAX_ERRS 32
typedef struct {
  uint64_t bad_dwords;  // exact count
  uint32_t flipped_or;  // OR of expected ^ actual over all bad dwords
  uint32_t n_errs;      // min(bad_dwords, MAX_ERRS)
  gsx_memtest_err errs[GSX_MEMTEST_MAX_ERRS];
} gsx_memtest_report;
// One launch on `stream`, not synchronised.
int gsx_memtest_write(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert);
// Compares every dword and ACCUMULATES into *report (the caller zeroes it); one stream sync.  rewrite != 0 also
// stores the complement of the expected word in the same pass (moving inversions: a bad word is overwritten
// with correct data).  The per-launch counters live in pinned host memory, as gsx_hbm_admit_n's do.
int gsx_memtest_check(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert, int rewrite, gsx_memtest_report* report);
// The fixed pass sequence of a level, each a triple {write, check + rewrite, check inverted}: QUICK runs ADDR and
// RANDOM (8 x bytes of traffic); FULL adds SOLID with seeds 0, ~0, 0x55555555, 0xAAAAAAAA and WALK with seeds 0..31.
int gsx_memtest_run(void* stream, void* base, uint64_t bytes, uint64_t origin, int level, gsx_memtest_report* report,
                    uint32_t* passes_out, double* seconds_out);
// Pass `idx` of a level's sequence (what gsx_memtest_run and gsx-memtest execute): 0, or 1 past the last pass.
typedef struct {
  int pattern;
  uint32_t seed;
  int invert, rewrite, write;  // write != 0: a write pass; otherwise a check, with or without rewrite
} gsx_memtest_pass_t;
int gsx_memtest_pass(int level, uint32_t idx, gsx_memtest_pass_t* out);

#ifdef __cplusplus
}
#endif
