// bf16 MFMA GEMM family for the pod workload: C[M][N] = A[M][K] * B[N][K]^T (bf16 in/out, fp32 accumulate).
// C ABI in gsx_kernels.h.
//
// Three kernels share one tile map, one LDS swizzle and one epilogue; they differ in the schedule of their K loop:
// gemm_kernel (several tile shapes, one __syncthreads per K-tile), gemm_phased_kernel (256x256, prefetch in flight
// across barriers; the dispatched one) and gemm_w4_kernel (256x256, one wave per SIMD; ablation).  Common structure
// (BM x BN block tile, BK = 64):
//   * global -> LDS with global_load_lds (16 B/lane), lane-linear LDS image,
//     XOR swizzle folded into the per-lane *global* source address;
//   * two LDS buffers: tile k+1 in flight while the MFMAs consume tile k;
//   * v_mfma_f32_16x16x32_bf16, each wave owns a (BM/WM) x (BN/WN) C tile;
//   * s_setprio around the MFMA burst so the partner wave's loads issue;
//   * grouped, XCD-aware tile order (GROUP_M tile-rows per group; workgroup
//     ids remapped bijectively so one XCD's blocks share A/B panels in L2);
//   * epilogue through LDS: 16-B coalesced row stores.
// The tile map, the swizzle, the epilogue, the first two schedules and the host launcher are in gemm_tile.h, which
// the fp8 family (gemm_fp8.hip) instantiates too; the table of the eleven configurations follows the kernels.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int BK = Bf16::BK;

// ---------------------------------------------------------------------------
// 4-wave 256x256 kernel: one wave per SIMD, 128x128 C per wave.
//
// rocprofv3 on the 8-wave kernels showed 1.57x the LDS instructions of
// hipBLASLt's 256x256 kernel: a 128x64 wave tile re-reads A once per 64
// columns.  A 128x128 wave tile halves that (LDS bytes per FLOP 0.75x), at
// the price of 256 fp32 accumulators per lane — AGPRs, which gfx950 has when
// a wave owns its SIMD (waves_per_eu = 1, 512 registers per lane).
//
// With no partner wave on the SIMD, latency is hidden inside the wave: the
// K loop runs in k32 sub-steps, and the fragments of sub-step s+1 (16
// ds_read_b128) are issued before the 64 MFMAs of sub-step s (register
// double buffer).  LDS holds two K-tiles (2 x 64 KiB); tile t+2 is staged
// into tile t's buffer as soon as every wave has read it, and waited for
// with a counted vmcnt(16) (one tile of loads stays in flight) one sub-step
// before it is read.  Past-the-end tiles are clamped (dead buffers).
//
// Measured (MI355X, random bf16, profiles/r01_rocprof_bench_gemm.md): LDS
// instructions drop to hipBLASLt's level (18.0M vs 16.8M at 8192^3; the
// 8-wave kernels issue 26.4M), but the kernel runs at 1.04-1.18 PFLOP/s, below
// the phased 8-wave kernel (1.41-1.47): hipcc (ROCm 7.2) keeps 256
// accumulators in AGPRs only with v_accvgpr_mov copies and s_nops between the
// MFMAs of the inner loop.  With the MFMAs in inline asm ("+a" pins the
// accumulators, ASM=true) the loop is clean — 8 MFMAs, 16 prefetch ds_reads,
// 56 MFMAs per sub-step, no copies — and reaches 1.11-1.22 PFLOP/s: with one
// wave per SIMD nothing fills the MFMA pipe across the two barriers per
// K-tile, which the staggered 8-wave kernel hides.  Kept as ablations; not
// dispatched by default.
// ---------------------------------------------------------------------------
template <int GROUP_M, bool ASM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_w4_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, uint16_t* __restrict__ C, int M, int N, int K) {
  constexpr int BM = 256, BN = 256, WT = 128;
  constexpr int TILE = 256 * BK * 2;  // 32 KiB per operand per K-tile
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  int tm, tn;
  tile_of<BM, BN, GROUP_M>(blockIdx.x, gridDim.x, M, N, tm, tn);
  const uint16_t* Ab = A + static_cast<size_t>(tm * BM) * K;
  const uint16_t* Bb = B + static_cast<size_t>(tn * BN) * K;

  int off[8];  // 8 rounds of 4 KiB (256 lanes x 16 B) cover one 256-row operand tile
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = (i * 4 + wid) * 64 + lane;
    off[i] = (p >> 3) * K + glds_col<uint16_t>(p);
  }
  const int nk = K / BK;
  auto stage = [&](int tile) {
    const int kt = tile < nk ? tile : nk - 1;
    char* la = lds + (tile & 1) * 2 * TILE;
    char* lb = la + TILE;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Ab + off[i] + kt * BK), (lptr_t)(la + (i * 4 + wid) * 1024), 16, 0,
                                       0);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * BK), (lptr_t)(lb + (i * 4 + wid) * 1024), 16, 0,
                                       0);
  };

  f32x4 acc[8][8];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  bf16x8 af[2][8], bfr[2][8];
  auto read = [&](int set, int tile, int kk) {
    const char* la = lds + (tile & 1) * 2 * TILE;
    const char* lb = la + TILE;
#pragma unroll
    for (int m = 0; m < 8; ++m)
      af[set][m] = *reinterpret_cast<const bf16x8*>(la + swz(wr * WT + m * 16 + fr, kk * 4 + fq));
#pragma unroll
    for (int n = 0; n < 8; ++n)
      bfr[set][n] = *reinterpret_cast<const bf16x8*>(lb + swz(wc * WT + n * 16 + fr, kk * 4 + fq));
  };
  // 64 MFMAs of one k32 sub-step; `prefetch` (the next sub-step's ds_reads) is issued after the
  // first row of 8, so the wait for this sub-step's fragments never covers the prefetch
  auto mma = [&](int set, int pf_tile, int pf_kk) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        if (m == 1 && n == 0) {
          __builtin_amdgcn_sched_barrier(0);
          read(set ^ 1, pf_tile, pf_kk);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ASM) {
          // accumulator pinned to AGPRs ("+a"): no accumulator copies between the MFMAs
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[m][n]) : "v"(af[set][m]), "v"(bfr[set][n]));
        } else {
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[set][m], bfr[set][n], acc[m][n], 0, 0, 0);
        }
      }
  };

  stage(0);
  stage(1);
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  ph_barrier();
  read(0, 0, 0);
  for (int t = 0; t < nk; ++t) {
    // sub-step (t, k 0..31): fragments of (t, k 32..63) in flight under the MFMAs
    mma(0, t, 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ph_barrier();  // every wave is done with tile t's buffer
    stage(t + 2);
    // sub-step (t, k 32..63): tile t+1 must have landed (tile t+2's 16 loads stay in flight)
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    ph_barrier();
    // unconditional (no phi copies); the last one reads a dead buffer, never used
    mma(1, t + 1, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (ASM) {
    // the compiler cannot see the asm MFMAs: cover the MFMA-write -> VALU-read (v_accvgpr_read) hazard
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  }
  ph_barrier();

  // wave-private 128x128 bf16 staging (32 KiB per wave)
  uint16_t* ct = reinterpret_cast<uint16_t*>(lds + wid * (WT * WT * 2));
  scatter16<WT>(ct, acc, fr, fq);
  store_wave_tile<WT, WT>(ct, C, N, tm * BM + wr * WT, tn * BN + wc * WT, 0, lane);
}

// ---------------------------------------------------------------------------
// Host side: one table (the launcher is gemm_tile.h's).
// ---------------------------------------------------------------------------

struct Cfg {
  const char* name;  // profiles/ key on the index and on this string
  int bm, bn;
  int (*launch)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K);
};
template <int BM, int BN, int WM, int WN, int GM>
constexpr Cfg plain(const char* name) {
  return {name, BM, BN,
          &launch<&gemm_kernel<Bf16, BM, BN, WM, WN, GM>, uint16_t, WM * WN * 64, 2 * (BM + BN) * BK * 2, BM, BN>};
}
template <int GM, bool M32>
constexpr Cfg phased(const char* name) {
  return {name, 256, 256, &launch<&gemm_phased_kernel<Bf16, GM, M32>, uint16_t, 512, 8 * PH_HALF, 256, 256>};
}
template <int GM, bool ASM>
constexpr Cfg w4(const char* name) {
  return {name, 256, 256, &launch<&gemm_w4_kernel<GM, ASM>, uint16_t, 256, 4 * 256 * BK * 2, 256, 256>};
}

constexpr Cfg kCfgs[] = {
    plain<128, 128, 2, 2, 8>("128x128/4w"),
    plain<256, 128, 4, 2, 4>("256x128/8w"),
    plain<128, 256, 2, 4, 8>("128x256/8w"),
    plain<256, 256, 2, 4, 4>("256x256/8w"),
    plain<128, 128, 2, 2, 1>("128x128/4w-nogroup"),
    phased<4, false>("256x256/8w-phased-g4"),
    phased<8, false>("256x256/8w-phased-g8"),
    w4<4, false>("256x256/4w-agpr-g4"),
    w4<8, false>("256x256/4w-agpr-g8"),
    w4<4, true>("256x256/4w-asm-agpr-g4"),
    phased<4, true>("256x256/8w-phased-g4-mfma32"),
};
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
// the two rows gsx_gemm_bf16_nt dispatches to
constexpr int kCfgGrouped128 = 0, kCfgPhased = 5;

static const Cfg* cfg_row(int cfg) { return cfg >= 0 && cfg < kNumCfgs ? &kCfgs[cfg] : nullptr; }

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_gemm_cfg_name(int cfg) { return cfg_row(cfg) ? cfg_row(cfg)->name : nullptr; }

int gsx_gemm_cfg_tile(int cfg, int* bm, int* bn) {
  const Cfg* c = cfg_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  return 0;
}

int gsx_gemm_bf16_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int cfg) {
  const Cfg* c = cfg_row(cfg);
  if (!c) return fail_arg("gsx_gemm_bf16_nt_launch_cfg: unknown config");
  return c->launch("gsx_gemm_bf16_nt_launch_cfg", S(stream), A, B, C, M, N, K);
}

int gsx_gemm_bf16_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % 64)
    return fail_arg("gsx_gemm_bf16_nt: need M%128==0, N%128==0, K%64==0");
  // phased 256x256 / 8 waves (prefetch in flight across barriers): 1.39-1.46 PFLOP/s on MI355X at
  // 4k-16k (the __syncthreads 256x256 tile: 1.12-1.21); 128x128 grouped otherwise (profiles/r01_kernels.json)
  const Cfg& c = kCfgs[(M % 256 == 0 && N % 256 == 0) ? kCfgPhased : kCfgGrouped128];
  return c.launch("gsx_gemm_bf16_nt", S(stream), A, B, C, M, N, K);
}

int gsx_event_time_gemm(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int iters,
                        float* ms) {
  return event_time(stream, iters, ms, [&] { return gsx_gemm_bf16_nt(stream, A, B, C, M, N, K); });
}

}  // extern "C"
