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
// One host launcher and one table of the eleven configurations follow the kernels.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

using namespace gsx;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;

constexpr int BK = 64;

// The LDS swizzle, both halves.  A K-tile row is 128 B = 8 chunks of 16 B, and the LDS image of a tile is
// lane-linear: load slot p (lane p of a round of global_load_lds) lands at byte 16 p, i.e. row p >> 3, chunk
// position p & 7.  Invariant: chunk c of row r sits at position c ^ ((r >> 1) & 7).  glds_col() is the writer's half
// (slot p fetches, from whichever global row its LDS row holds, the chunk that belongs at its position), swz() the
// reader's.  The XOR is its own inverse, so both apply the same term; change one and the other must follow.
__device__ __forceinline__ int glds_col(int p) {  // in elements, from the first element of the slot's global row
  const int row = p >> 3, slot = p & 7;
  return (slot ^ ((row >> 1) & 7)) * 8;
}
__device__ __forceinline__ uint32_t swz(int row, int chunk) {  // in bytes, from the tile's LDS base
  return static_cast<uint32_t>(row * (BK * 2) + ((chunk ^ ((row >> 1) & 7)) << 4));
}

__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return static_cast<uint16_t>((u >> 16) | ((u & 0xffff) ? 0x40 : 0));
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

// XCD-aware bijective remap of the workgroup id (ids are dealt round-robin to the 8 XCDs), then grouped tile order:
// GROUP_M tile-rows per group, the last group ragged.
template <int BM, int BN, int GROUP_M>
__device__ __forceinline__ void tile_of(int orig, int nwg, int M, int N, int& tm, int& tn) {
  const int xcd = orig & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  const int ntm = M / BM, ntn = N / BN;
  const int per_group = GROUP_M * ntn;
  const int g = wg / per_group;
  const int first_m = g * GROUP_M;
  const int gm = (ntm - first_m) < GROUP_M ? (ntm - first_m) : GROUP_M;
  tm = first_m + (wg % per_group) % gm;
  tn = (wg % per_group) / gm;
}

// Epilogue through LDS, in a region private to the wave: the accumulator fragments are scattered as bf16 into a
// row-major WTM x WTN tile `ct`, which then leaves in 16-B row stores.
// 16x16 C map: column fr = lane & 15, row 4 fq + reg, fq = lane >> 4
template <int WTN, int MR, int NR>
__device__ __forceinline__ void scatter16(uint16_t* ct, const f32x4 (&acc)[MR][NR], int fr, int fq) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) ct[(m * 16 + fq * 4 + j) * WTN + n * 16 + fr] = f2bf(acc[m][n][j]);
}
// 32x32 C map: column r32 = lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 h32, h32 = lane >> 5
template <int WTN, int MR, int NR>
__device__ __forceinline__ void scatter32(uint16_t* ct, const f32x16 (&acc)[MR][NR], int r32, int h32) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        ct[(m * 32 + (j & 3) + 8 * (j >> 2) + 4 * h32) * WTN + n * 32 + r32] = f2bf(acc[m][n][j]);
}
// The wave tile's origin in C is (row0, col0 + wcol).  The column comes in two parts that are added to the pointer one
// after the other: gemm_kernel keeps its block and wave columns apart, the 256x256 kernels pass their sum and 0.
// Summing them first is the same address but another instruction stream for gemm_kernel (0.4 % slower on MI355X).
template <int WTM, int WTN>
__device__ __forceinline__ void store_wave_tile(const uint16_t* ct, uint16_t* C, int N, int row0, int col0, int wcol,
                                                int lane) {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  constexpr int LPR = WTN / 8;   // lanes per row (16 B each)
  constexpr int RPI = 64 / LPR;  // rows per store instruction
#pragma unroll
  for (int i = 0; i < WTM / RPI; ++i) {
    const int rr = i * RPI + lane / LPR, cc = (lane % LPR) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(ct + rr * WTN + cc);
    *reinterpret_cast<uint4*>(C + static_cast<size_t>(row0 + rr) * N + col0 + wcol + cc) = v;
  }
}

template <int BM, int BN, int WM, int WN, int GROUP_M>
__global__ __launch_bounds__(WM * WN * 64) void gemm_kernel(const uint16_t* __restrict__ A,
                                                           const uint16_t* __restrict__ B,
                                                           uint16_t* __restrict__ C, int M, int N, int K) {
  constexpr int NW = WM * WN;
  constexpr int TA = BM * BK * 2, TB = BN * BK * 2;  // bytes per operand tile
  constexpr int MR = BM / WM / 16, NR = BN / WN / 16;
  constexpr int RA = TA / 1024 / NW, RB = TB / 1024 / NW;  // glds rounds per wave (1 KiB each)
  static_assert(RA >= 1 && RB >= 1 && TA % (1024 * NW) == 0 && TB % (1024 * NW) == 0, "tile/wave mismatch");
  constexpr int WTM = BM / WM, WTN = BN / WN;  // wave tile
  static_assert(NW * WTM * WTN * 2 <= 2 * (TA + TB), "epilogue staging must fit in LDS");
  extern __shared__ __attribute__((aligned(16))) char lds[];  // [buf][A|B], reused by the epilogue

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WN, wc = wid % WN;

  int tm, tn;
  tile_of<BM, BN, GROUP_M>(blockIdx.x, gridDim.x, M, N, tm, tn);
  const int row0 = tm * BM, col0 = tn * BN;

  int off[RA > RB ? RA : RB];  // round i loads the same rows and slots of an A tile and of a B tile
#pragma unroll
  for (int i = 0; i < (RA > RB ? RA : RB); ++i) {
    const int p = (i * NW + wid) * 64 + lane;
    off[i] = (p >> 3) * K + glds_col(p);
  }
  const uint16_t* Ab = A + static_cast<size_t>(row0) * K;
  const uint16_t* Bb = B + static_cast<size_t>(col0) * K;

  auto stage = [&](int kt, int buf) {
    char* la = lds + buf * (TA + TB);
    char* lb = la + TA;
#pragma unroll
    for (int i = 0; i < RA; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Ab + off[i] + kt * BK), (lptr_t)(la + (i * NW + wid) * 1024), 16,
                                       0, 0);
#pragma unroll
    for (int i = 0; i < RB; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * BK), (lptr_t)(lb + (i * NW + wid) * 1024), 16,
                                       0, 0);
  };

  f32x4 acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  stage(0, 0);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
    const char* la = lds + buf * (TA + TB);
    const char* lb = la + TA;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int ch = kk * 4 + fq;
      bf16x8 bfr[NR];
#pragma unroll
      for (int n = 0; n < NR; ++n) bfr[n] = *reinterpret_cast<const bf16x8*>(lb + swz(wc * WTN + n * 16 + fr, ch));
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(la + swz(wr * WTM + m * 16 + fr, ch));
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < NR; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[n], acc[m][n], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
  }
  uint16_t* ct = reinterpret_cast<uint16_t*>(lds + wid * (WTM * WTN * 2));
  scatter16<WTN>(ct, acc, fr, fq);
  store_wave_tile<WTM, WTN>(ct, C, N, row0 + wr * WTM, col0, wc * WTN, lane);
}

// ---------------------------------------------------------------------------
// Phased 256x256 kernel: the prefetch stays in flight across barriers.
//
// The kernel above ends every K-tile with __syncthreads(), which hipcc lowers
// to `s_waitcnt vmcnt(0); s_barrier`: the next tile's loads are drained every
// 64 K, and at one 512-thread block per CU nothing hides that.  Here a K-tile
// is four phases; each phase MFMAs one quadrant of the wave's 128x64 C tile
// (16 MFMAs) and issues one *half-tile* (16 KiB: 128 rows x 64 k of A or B)
// two K-tiles ahead.  Waits are counted (`vmcnt(8)` = four half-tiles may stay
// in flight), barriers are raw s_barrier, and the two wave groups (wr = 0/1,
// one of each per SIMD) run one barrier apart so that one wave's ds_reads
// overlap the other's MFMAs.
//
// Half-tiles (LDS regions of 16 KiB, [buffer = tile & 1][half]):
//   0: A rows {0-63, 128-191}  1: A rows {64-127, 192-255}   (m-half of each wave row)
//   2: B cols {wc*64 + 0..31}  3: B cols {wc*64 + 32..63}     (n-half of each wave col)
// Per K-tile phases (reads -> MFMA quadrant, and what is staged):
//   p0: read A0,B2 -> (m0,n0)   stage tile t+1 half 3
//   p1: read B3    -> (m0,n1)   stage tile t+1 half 1
//   p2: read A1    -> (m1,n1)   stage tile t+2 half 0
//   p3: -          -> (m1,n0)   stage tile t+2 half 2
// Every half is restaged >= 2 phases after its last read (WAR across the
// staggered groups) and waited for (vmcnt(8) before the first barrier of the
// phase) one phase before it is read (RAW).  Tiles past the end are clamped to
// the last tile so the counts stay uniform; those loads land in dead buffers.
// ---------------------------------------------------------------------------
constexpr int PH_HALF = 128 * BK * 2;  // 16 KiB

__device__ __forceinline__ void ph_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// M32: the same schedule on v_mfma_f32_32x32x16_bf16 (per quadrant 2 x 1 blocks of 32x32 over 4 k-steps: 8 MFMAs
// of twice the work instead of 16), for the A/B the MFMA-shape rule asks for (the chip may hold a different clock
// on the other shape; same LDS bytes, same registers).
template <int GROUP_M, bool M32 = false>
__global__ __launch_bounds__(512) void gemm_phased_kernel(const uint16_t* __restrict__ A,
                                                         const uint16_t* __restrict__ B, uint16_t* __restrict__ C,
                                                         int M, int N, int K) {
  constexpr int BM = 256, BN = 256, WTM = 128, WTN = 64;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;

  int tm, tn;
  tile_of<BM, BN, GROUP_M>(blockIdx.x, gridDim.x, M, N, tm, tn);
  const uint16_t* Ab = A + static_cast<size_t>(tm * BM) * K;
  const uint16_t* Bb = B + static_cast<size_t>(tn * BN) * K;

  // per-lane source offsets of the two 8-KiB rounds of each half
  int off[4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = (i * 8 + wid) * 64 + lane;
    const int lr = p >> 3;
    const int sw = glds_col(p);
    off[0][i] = ((lr >> 6) * 128 + (lr & 63)) * K + sw;
    off[1][i] = ((lr >> 6) * 128 + 64 + (lr & 63)) * K + sw;
    off[2][i] = ((lr >> 5) * 64 + (lr & 31)) * K + sw;
    off[3][i] = ((lr >> 5) * 64 + 32 + (lr & 31)) * K + sw;
  }
  const int nk = K / BK;
  auto stage = [&](int tile, int half) {
    const int kt = tile < nk ? tile : nk - 1;
    const uint16_t* src = (half < 2 ? Ab : Bb) + kt * BK;
    char* dst = lds + ((tile & 1) * 4 + half) * PH_HALF + wid * 1024;
    __builtin_amdgcn_global_load_lds((gptr_t)(src + off[half][0]), (lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(src + off[half][1]), (lptr_t)(dst + 8 * 1024), 16, 0, 0);
  };

  // the wave's 128x64 tile as [8][4] 16x16 fragments, or (M32) as [32-row block][32-col block]
  constexpr int AM = M32 ? 4 : 8, AN = M32 ? 2 : 4;
  std::conditional_t<M32, f32x16, f32x4> acc[AM][AN];
#pragma unroll
  for (int m = 0; m < AM; ++m)
#pragma unroll
    for (int n = 0; n < AN; ++n)
#pragma unroll
      for (int j = 0; j < (M32 ? 16 : 4); ++j) acc[m][n][j] = 0.f;

  const int fr = lane & 15, fq = lane >> 4;
  const int r32 = lane & 31, h32 = lane >> 5;  // M32 operand maps: row / column lane & 31, k = 8 (lane >> 5) + j
  bf16x8 af[4][2], bf[2][2][2];  // A: [m][kk]; B: [nh][n][kk]  (M32: A [b][kk], B [nh][kk], k-steps of 16)

  auto read_a = [&](const char* base, int mh) {
    const char* h = base + mh * PH_HALF;
    if constexpr (M32) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          af[b * 2 + (kk >> 1)][kk & 1] =
              *reinterpret_cast<const bf16x8*>(h + swz(wr * 64 + b * 32 + r32, kk * 2 + h32));
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          af[m][kk] = *reinterpret_cast<const bf16x8*>(h + swz(wr * 64 + m * 16 + fr, kk * 4 + fq));
    }
  };
  auto read_b = [&](const char* base, int nh) {
    const char* h = base + (2 + nh) * PH_HALF;
    if constexpr (M32) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        bf[nh][kk >> 1][kk & 1] = *reinterpret_cast<const bf16x8*>(h + swz(wc * 32 + r32, kk * 2 + h32));
    } else {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          bf[nh][n][kk] = *reinterpret_cast<const bf16x8*>(h + swz(wc * 32 + n * 16 + fr, kk * 4 + fq));
    }
  };
  auto mma = [&](int mh, int nh) {
    __builtin_amdgcn_s_setprio(1);
    if constexpr (M32) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[mh * 2 + b][nh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af[b * 2 + (kk >> 1)][kk & 1], bf[nh][kk >> 1][kk & 1], acc[mh * 2 + b][nh], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[mh * 4 + m][nh * 2 + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][kk], bf[nh][n][kk],
                                                                                 acc[mh * 4 + m][nh * 2 + n], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: what the steady state has issued before tile 0, phase 0
  stage(0, 0);
  stage(0, 2);
  stage(0, 3);
  stage(0, 1);
  stage(1, 0);
  stage(1, 2);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  ph_barrier();
  if (wr == 1) ph_barrier();  // stagger the groups by one barrier

  for (int t = 0; t < nk; ++t) {
    const char* base = lds + (t & 1) * 4 * PH_HALF;
    // p0
    read_a(base, 0);
    read_b(base, 0);
    stage(t + 1, 3);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    ph_barrier();
    mma(0, 0);
    ph_barrier();
    // p1
    read_b(base, 1);
    stage(t + 1, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    ph_barrier();
    mma(0, 1);
    ph_barrier();
    // p2
    read_a(base, 1);
    stage(t + 2, 0);
    ph_barrier();
    mma(1, 1);
    ph_barrier();
    // p3
    stage(t + 2, 2);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    ph_barrier();
    mma(1, 0);
    ph_barrier();
  }
  if (wr == 0) ph_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ph_barrier();

  uint16_t* ct = reinterpret_cast<uint16_t*>(lds + wid * (WTM * WTN * 2));
  if constexpr (M32) {
    scatter32<WTN>(ct, acc, r32, h32);
  } else {
    scatter16<WTN>(ct, acc, fr, fq);
  }
  store_wave_tile<WTM, WTN>(ct, C, N, tm * BM + wr * WTM, tn * BN + wc * WTN, 0, lane);
}

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
    off[i] = (p >> 3) * K + glds_col(p);
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
// Host side: one launcher, one table.
// ---------------------------------------------------------------------------

// Validates once for every kernel, then launches; a failure's text begins with `who`, the C entry point.
template <auto KERNEL, int THREADS, int LDS, int BM, int BN>
int launch(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K) {
  char msg[160];
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK) {
    std::snprintf(msg, sizeof(msg), "%s: need M%%%d==0, N%%%d==0, K%%%d==0", who, BM, BN, BK);
    return fail_arg(msg);
  }
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) % 16) {
    std::snprintf(msg, sizeof(msg), "%s: operands must be 16-B aligned", who);
    return fail_arg(msg);
  }
  // The kernels keep a lane's source offset inside an operand tile in an int: row * K + column, with
  // row < max(BM, BN) and column <= BK - 8 (off[] of the three kernels).  Everything else that grows with the
  // problem is added to the pointer in 64 bits.
  constexpr int SIDE = BM > BN ? BM : BN;
  if (static_cast<int64_t>(SIDE - 1) * K + (BK - 8) > INT32_MAX) {
    std::snprintf(msg, sizeof(msg), "%s: K too large: %d rows of K elements must stay below 2^31", who, SIDE);
    return fail_arg(msg);
  }
  // More dynamic LDS than the default limit has to be asked for.  The flag is per device because
  // hipFuncSetAttribute is documented per function and device, not because a failure without it was observed
  // (that has not been measured).  Two threads that race here both set the same value.
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (int rc = current_device(who, &dev)) return rc;
  if (!attr[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) return fail(e, who);
    attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(KERNEL, dim3((M / BM) * (N / BN)), dim3(THREADS), LDS, s, static_cast<const uint16_t*>(A),
                     static_cast<const uint16_t*>(B), static_cast<uint16_t*>(C), M, N, K);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct Cfg {
  const char* name;  // profiles/ key on the index and on this string
  int bm, bn;
  int (*launch)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K);
};
template <int BM, int BN, int WM, int WN, int GM>
constexpr Cfg plain(const char* name) {
  return {name, BM, BN, &launch<&gemm_kernel<BM, BN, WM, WN, GM>, WM * WN * 64, 2 * (BM + BN) * BK * 2, BM, BN>};
}
template <int GM, bool M32>
constexpr Cfg phased(const char* name) {
  return {name, 256, 256, &launch<&gemm_phased_kernel<GM, M32>, 512, 8 * PH_HALF, 256, 256>};
}
template <int GM, bool ASM>
constexpr Cfg w4(const char* name) {
  return {name, 256, 256, &launch<&gemm_w4_kernel<GM, ASM>, 256, 4 * 256 * BK * 2, 256, 256>};
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
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto timed = [&]() -> int {
    GSX_CHECK(hipEventCreate(&e0));
    GSX_CHECK(hipEventCreate(&e1));
    GSX_CHECK(hipEventRecord(e0, S(stream)));
    for (int i = 0; i < iters; ++i) {
      if (int rc = gsx_gemm_bf16_nt(stream, A, B, C, M, N, K)) return rc;
    }
    GSX_CHECK(hipEventRecord(e1, S(stream)));
    GSX_CHECK(hipEventSynchronize(e1));
    GSX_CHECK(hipEventElapsedTime(ms, e0, e1));
    return 0;
  };
  const int rc = timed();
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

}  // extern "C"
