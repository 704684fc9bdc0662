// Block-scaled fp8 grouped GEMM for MoE prefill: for every pair p of a tile plan of gsx_moe_prefill_plan, with e its
// tile's expert, C[p][0..N) (bf16) = A[p / a_div][0..K) * B[e][N][K]^T on OCP e4m3 operands with one fp32 scale per
// 1 x 128 group of a row of A and one per 128 x 128 block of an expert's matrix: gsx_moe_prefill_gemm_nt on the operands
// of gsx_gemm_fp8_block_nt.  C ABI and the numeric contract in gsx_kernels.h.
//
// One configuration, "128x128/4w-gather".  A plan tile is 128 pairs of one expert, so a workgroup's 128 x 128 block
// tile has one expert's B, and what neither parent has: 128 rows of A that lie anywhere in A, and with them 128 rows
// of scale_a that lie anywhere in scale_a.
//
// * Arithmetic.  gemm_fp8_block.hip's, instruction for instruction: per K-tile g (one scale block) and 16x16 fragment
//     p   = v_mfma_f32_16x16x128_f8f6f4(fragment of g, from a zero accumulator)
//     acc = fma(p, s_g, acc),  s_g = fl(scale_a[row][g] * scale_b[e][nb][g])
//   with B the MFMA's first operand, so lane (fr, fq) holds row fr of the fragment against columns 4 fq .. 4 fq + 3 and
//   needs one scale_a value per 16-row fragment; the fold of fragment f is issued behind the MFMA of fragment f + 2, the
//   last two folds of a K-tile behind the first MFMAs of the next, and the kernel is held at two waves per SIMD so that
//   the MFMA results stay in VGPRs.  The reasons are in that file's head comment.  4 waves as 2 x 2: a wave tile of 64
//   columns never straddles a 128-column scale block, and scale_b is one scalar load per wave and K-tile, issued one
//   K-tile ahead, through the expert's block row: scale_b + (e (N / 128) + nb) (K / 128), a 64-bit offset.
// * Gathering A.  LDS row r of the A tile holds A row rows[r] / a_div.  A lane stages 4 rows (one per round of 16-B
//   global_load_lds); it reads their 4 plan entries once, makes 4 64-bit addresses (row, and the chunk its LDS slot
//   holds under the swizzle) before the K loop and adds 128 B per K-tile.  An entry outside [0, P), the -1 of the
//   padding included, points at row 0 of A: valid memory whose product is never stored.  B's rows are dense: one 64-bit
//   base per workgroup, (e N + col0) K, and gemm_tile.h's 32-bit lane offsets.
// * Gathering scale_a.  The scale image of the tile is [row][4 K-tiles] fp32, 2 KiB, double-buffered behind the operand
//   stages, written by 4-B global_load_lds: lane l of a round fetches K-tile 4 q + l % 4 of tile row 16 round + l / 4,
//   from that pair's own scale row, scale_a + (rows[r] / a_div) sa_stride (row 0 for padding).  A lane whose K-tile
//   is past the last fetches the last again: nothing beyond a row's K / 128 entries is read, whatever sa_stride is.
//   Image q is staged with the operands of K-tile 4 q, one K-tile before its first use; the buffer it replaces was
//   last read four barriers earlier.
// * Epilogue.  Each wave transposes its 64 x 64 result through its 8 KiB of the (now idle) operand buffers: a lane's
//   four values are four columns of one row, one 8-B LDS store; rows then leave as 16-B stores to C + pair * N (64-bit),
//   8 lanes per row.  The 8 plan entries a lane stores by are read before the K loop; a padding row stores nothing, so
//   a pair that no tile lists keeps what C held.
// * LDS 2 x (16 + 16) KiB + 2 x 2 KiB = 68 KiB: two workgroups per CU, which with 4 waves each is the two waves per
//   SIMD the fold wants.  No scratch.
// * Untrusted plan.  n_tiles is clamped to T_max, a tile whose expert is outside [0, E) is skipped; both tests come
//   before the first barrier and the first load of A or B.  The grid is (N / 128) T_max, fixed by the host.
// * Workgroup order.  tile_of<128, 128, 8> over T_max row tiles by N / 128 column strips: after the XCD remap an XCD
//   runs a contiguous range of ids, and within it groups of 8 consecutive plan tiles sweep the column strips, the tile
//   fastest.  Tiles of an expert are consecutive in the plan, so the 8 workgroups that are neighbours on an XCD read one
//   128 x K strip of one expert's B at the same time (where experts have fewer tiles, strips of the few experts the 8
//   tiles belong to), and the 64 workgroups an XCD holds (two per CU) cover 8 strips of the same 8 tiles: a K-tile of a
//   B strip and of a gathered A panel is asked for by 8 workgroups of one L2 within a short time, and only the first
//   goes to HBM.  With the strip fastest a B strip would be re-read once per tile of its expert, far apart in time;
//   with whole columns of tiles fastest the gathered A panels would be.  That is reasoning, not a measurement: the
//   group size is the bf16 grouped kernel's and was not swept.  Unused tiles are the highest and leave at once.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "moe_prefill_plan.h"

namespace gsxgemm {

constexpr int PFB_SQ = 4;              // K-tiles per scale image
constexpr int PFB_SROW = PFB_SQ * 4;   // bytes of a row of a scale image
constexpr int PFB_LAG = 2;             // fragments between an MFMA and its fold
constexpr int PFB_GROUP_M = 8;
constexpr int PFB_TILE = PF_BM * ROW_BYTES;                     // bytes per operand tile (BM == BN)
constexpr int PFB_SIMG = PF_BM * PFB_SROW;                      // bytes of a scale image
constexpr int PFB_LDS = 2 * 2 * PFB_TILE + 2 * PFB_SIMG;        // [buf][A|B], [buf] scale images

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pfb_gemm_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, uint16_t* __restrict__ C,
    const int32_t* __restrict__ plan, int T_max, int P, int E, int a_div, int N, int K, const float* __restrict__ sa,
    int64_t sa_stride, const float* __restrict__ sb) {
  using OP = Fp8K128;
  using frag = OP::frag;
  constexpr int NW = 4, WN = 2, WT = 64, MR = 4, NR = 4, F = MR * NR;
  constexpr int R = PFB_TILE / 1024 / NW;  // glds rounds per wave and operand (1 KiB each)
  constexpr int RS = PF_BM / 16 / NW;      // and of a scale image (16 rows each)
  static_assert(PFB_LAG >= 1 && PFB_LAG <= NR, "the carried fragments share the last m");
  static_assert(NW * WT * WT * 2 <= 2 * 2 * PFB_TILE, "epilogue staging must fit in the operand buffers");
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / WN, wc = wid % WN;
  const int fr = lane & 15, fq = lane >> 4;

  int tm, tn;
  tile_of<PF_BM, PF_BN, PFB_GROUP_M>(blockIdx.x, gridDim.x, T_max * PF_BM, N, tm, tn);
  const int n_tiles = plan[0];
  if (tm >= (n_tiles < T_max ? n_tiles : T_max)) return;  // a negative n_tiles: every tile
  const int e = plan[4 + tm];
  if (static_cast<uint32_t>(e) >= static_cast<uint32_t>(E)) return;
  const int32_t* const rows = plan + 4 + T_max + static_cast<size_t>(tm) * PF_BM;
  const int col0 = tn * PF_BN;
  const int nk = K / ROW_BYTES;

  // the A row behind a plan entry; padding and anything else outside [0, P) reads row 0
  const auto src_row = [&](int pair) -> int64_t {
    return static_cast<uint32_t>(pair) < static_cast<uint32_t>(P) ? pair / a_div : 0;
  };
  int off[R];            // B: as the dense kernel
  const uint8_t* ar[R];  // A: the lane's row of round i, at the chunk its LDS slot holds
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int p = (i * NW + wid) * 64 + lane;
    off[i] = (p >> 3) * K + glds_col<uint8_t>(p);
    ar[i] = A + src_row(rows[p >> 3]) * K + glds_col<uint8_t>(p);
  }
  const uint8_t* Bb = B + (static_cast<size_t>(e) * N + col0) * K;
  auto stage = [&](int kt, int buf) {
    char* la = lds + buf * 2 * PFB_TILE;
    char* lb = la + PFB_TILE;
#pragma unroll
    for (int i = 0; i < R; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(ar[i] + kt * ROW_BYTES), (lptr_t)(la + (i * NW + wid) * 1024), 16, 0,
                                       0);
#pragma unroll
    for (int i = 0; i < R; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * ROW_BYTES), (lptr_t)(lb + (i * NW + wid) * 1024),
                                       16, 0, 0);
  };

  // scale_a: image q holds K-tiles 4 q .. 4 q + 3 of the tile's rows; lane l of round i fetches tile row
  // (i NW + wid) 16 + l / 4, K-tile 4 q + l % 4 (the last K-tile where that is past the end), from the pair's scale row
  const float* srow[RS];
#pragma unroll
  for (int i = 0; i < RS; ++i) srow[i] = sa + src_row(rows[(i * NW + wid) * 16 + (lane >> 2)]) * sa_stride;
  auto stage_scales = [&](int q) {
    char* img = lds + 2 * 2 * PFB_TILE + (q & 1) * PFB_SIMG;
    const int g = q * PFB_SQ + (lane & 3);
    const int gc = g < nk ? g : nk - 1;
#pragma unroll
    for (int i = 0; i < RS; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(srow[i] + gc), (lptr_t)(img + (i * NW + wid) * 256), 4, 0, 0);
  };
  // scale_b: one value per wave and K-tile, from the expert's block row
  const float* sbw = sb + (static_cast<size_t>(e) * (N / 128) + (col0 + wc * WT) / 128) * nk;
  int crow[WT / 8];  // the pair of wave-tile row 8 i + lane / 8
#pragma unroll
  for (int i = 0; i < WT / 8; ++i) crow[i] = rows[wr * WT + i * 8 + (lane >> 3)];

  f32x4 acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const auto fold = [&](f32x4& c, const f32x4& p, float s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = __builtin_fmaf(p[j], s, c[j]);
  };
  // the last PFB_LAG fragments of the K-tile before and their scale; zeros fold to nothing in front of K-tile 0
  f32x4 carry[PFB_LAG];
#pragma unroll
  for (int i = 0; i < PFB_LAG; ++i) carry[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float scarry = 0.f;

  stage_scales(0);
  stage(0, 0);
  float sb_next = sbw[0];
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const float sbk = sb_next;
    if (kt + 1 < nk) {
      if (((kt + 1) & (PFB_SQ - 1)) == 0) stage_scales((kt + 1) / PFB_SQ);
      stage(kt + 1, buf ^ 1);
      sb_next = sbw[kt + 1];
    }
    const char* la = lds + buf * 2 * PFB_TILE;
    const char* lb = la + PFB_TILE;
    const char* img = lds + 2 * 2 * PFB_TILE + ((kt / PFB_SQ) & 1) * PFB_SIMG + (kt & (PFB_SQ - 1)) * 4;
    frag bfr[NR][2];
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        bfr[n][c] = *reinterpret_cast<const frag*>(lb + swz(wc * WT + n * 16 + fr, c * 4 + fq));
    float s[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
      s[m] = *reinterpret_cast<const float*>(img + (wr * WT + m * 16 + fr) * PFB_SROW) * sbk;

    f32x4 p[F];
    frag af[2];
    static_for<F>([&](auto f) {
      constexpr int m = f / NR, n = f % NR;
      if constexpr (n == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) af[c] = *reinterpret_cast<const frag*>(la + swz(wr * WT + m * 16 + fr, c * 4 + fq));
      }
      p[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      OP::mma(p[f], bfr[n], af);  // B first: register j is column 4 fq + j, the lane's row of the tile is fr
      if constexpr (f < PFB_LAG) {
        fold(acc[MR - 1][NR - PFB_LAG + f], carry[f], scarry);
      } else {
        fold(acc[(f - PFB_LAG) / NR][(f - PFB_LAG) % NR], p[f - PFB_LAG], s[(f - PFB_LAG) / NR]);
      }
    });
#pragma unroll
    for (int i = 0; i < PFB_LAG; ++i) carry[i] = p[F - PFB_LAG + i];
    scarry = s[MR - 1];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PFB_LAG; ++i) fold(acc[MR - 1][NR - PFB_LAG + i], carry[i], scarry);

  // Epilogue through LDS, in a region private to the wave: a 64 x 64 bf16 tile whose rows are 8 chunks of 16 B, chunk c
  // of row r at position c ^ (r & 7) (the 16 lanes of a write hold 16 rows of one column).
  char* ct = lds + wid * (WT * WT * 2);
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int r = m * 16 + fr, c = n * 2 + (fq >> 1);
      i32x2 v;
      v[0] = static_cast<int>(f2bf(acc[m][n][0]) | (static_cast<uint32_t>(f2bf(acc[m][n][1])) << 16));
      v[1] = static_cast<int>(f2bf(acc[m][n][2]) | (static_cast<uint32_t>(f2bf(acc[m][n][3])) << 16));
      *reinterpret_cast<i32x2*>(ct + r * (WT * 2) + ((c ^ (r & 7)) << 4) + (fq & 1) * 8) = v;
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  uint16_t* Cw = C + col0 + wc * WT;
#pragma unroll
  for (int i = 0; i < WT / 8; ++i) {  // 8 rows per store instruction, 8 lanes per row
    const int r = i * 8 + (lane >> 3), c = lane & 7;
    const i32x4 v = *reinterpret_cast<const i32x4*>(ct + r * (WT * 2) + ((c ^ (r & 7)) << 4));
    if (static_cast<uint32_t>(crow[i]) < static_cast<uint32_t>(P))
      *reinterpret_cast<i32x4*>(Cw + static_cast<size_t>(crow[i]) * N + c * 8) = v;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct PfbArgs {
  const void* A;
  int a_div;
  const void* B;
  void* C;
  const int32_t* plan;
  int M, topk, E, N, K;
  const float* sa;
  int64_t sa_stride;
  const float* sb;
};

static int pfb_validate(const char* who, const PfbArgs& a) {
  if (int rc = pf_sizes(who, a.M, a.topk, a.E)) return rc;
  if (a.a_div < 1) return pf_refuse(who, "need a_div >= 1");
  if (a.N <= 0 || a.N % PF_BN || a.K <= 0 || a.K % ROW_BYTES) return pf_refuse(who, "need N%128==0, K%128==0");
  if (!a.A || !a.B || !a.C || !a.plan || !a.sa || !a.sb)
    return pf_refuse(who, "A, B, C, plan, scale_a and scale_b must not be NULL");
  if ((pf_bits(a.A) | pf_bits(a.B) | pf_bits(a.C)) % 16) return pf_refuse(who, "operands must be 16-B aligned");
  if ((pf_bits(a.plan) | pf_bits(a.sa) | pf_bits(a.sb)) % 4)
    return pf_refuse(who, "plan, scale_a and scale_b must be 4-B aligned");
  // a lane's offset inside a B tile is an int, as in the dense launcher
  if (static_cast<int64_t>(PF_BN - 1) * a.K + (ROW_BYTES - CHUNK) > INT32_MAX)
    return pf_refuse(who, "K too large: 128 rows of K elements must stay below 2^31");
  if (pf_tmax(a.M, a.topk, a.E) * (a.N / PF_BN) > INT32_MAX)
    return pf_refuse(who, "N too large: (N / 128) * T_max workgroups must stay below 2^31");
  const uint64_t g = static_cast<uint64_t>(a.K) / 128;
  if (a.sa_stride < static_cast<int64_t>(g)) return pf_refuse(who, "need sa_stride >= K/128");
  const uint64_t P = static_cast<uint64_t>(a.M) * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const PfSpan c{a.C, P * a.N * 2};
  const PfSpan in[] = {{a.A, a_rows * a.K},
                       {a.B, static_cast<uint64_t>(a.E) * a.N * a.K},
                       {a.plan, pf_plan_ints(a.M, a.topk, a.E) * 4},
                       {a.sa, ((a_rows - 1) * static_cast<uint64_t>(a.sa_stride) + g) * 4},
                       {a.sb, static_cast<uint64_t>(a.E) * (a.N / 128) * g * 4}};
  for (const PfSpan& s : in)
    if (pf_overlap(c, s)) return pf_refuse(who, "C must not overlap A, B, plan, scale_a or scale_b");
  return 0;
}

static int pfb_run(const char* who, void* stream, const PfbArgs& a) {
  // 68 KiB of dynamic LDS has to be asked for, per device, as in the dense launcher (gemm_tile.h)
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (int rc = current_device(who, &dev)) return rc;
  if (!attr[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pfb_gemm_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, PFB_LDS);
    if (e != hipSuccess) return fail(e, who);
    attr[dev].store(true, std::memory_order_release);
  }
  const int T_max = static_cast<int>(pf_tmax(a.M, a.topk, a.E));
  hipLaunchKernelGGL(pfb_gemm_kernel, dim3(T_max * (a.N / PF_BN)), dim3(256), PFB_LDS, S(stream),
                     static_cast<const uint8_t*>(a.A), static_cast<const uint8_t*>(a.B), static_cast<uint16_t*>(a.C),
                     a.plan, T_max, a.M * a.topk, a.E, a.a_div, a.N, a.K, a.sa, a.sa_stride, a.sb);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct PfbCfg {
  const char* name;
  int bm, bn, waves;
  int (*run)(const char* who, void* stream, const PfbArgs& a);
};
constexpr PfbCfg kPfbCfgs[] = {{"128x128/4w-gather", PF_BM, PF_BN, 4, &pfb_run}};
constexpr int kNumPfbCfgs = sizeof(kPfbCfgs) / sizeof(kPfbCfgs[0]);
static const PfbCfg* pfb_row(int cfg) { return cfg >= 0 && cfg < kNumPfbCfgs ? &kPfbCfgs[cfg] : nullptr; }

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_moe_prefill_gemm_fp8_block_cfg_name(int cfg) { return pfb_row(cfg) ? pfb_row(cfg)->name : nullptr; }

int gsx_moe_prefill_gemm_fp8_block_cfg_shape(int cfg, int* bm, int* bn, int* waves) {
  const PfbCfg* c = pfb_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  *waves = c->waves;
  return 0;
}

int gsx_moe_prefill_gemm_fp8_block_nt_launch_cfg(void* stream, const void* A, int a_div, const void* B, void* C,
                                                 const int32_t* plan, int M, int topk, int E, int N, int K,
                                                 const float* scale_a, int64_t sa_stride, const float* scale_b,
                                                 int cfg) {
  const char* who = "gsx_moe_prefill_gemm_fp8_block_nt_launch_cfg";
  const PfbCfg* c = pfb_row(cfg);
  if (!c) return pf_refuse(who, "unknown config");
  const PfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  if (int rc = pfb_validate(who, a)) return rc;
  return c->run(who, stream, a);
}

int gsx_moe_prefill_gemm_fp8_block_nt(void* stream, const void* A, int a_div, const void* B, void* C,
                                      const int32_t* plan, int M, int topk, int E, int N, int K, const float* scale_a,
                                      int64_t sa_stride, const float* scale_b) {
  const char* who = "gsx_moe_prefill_gemm_fp8_block_nt";
  const PfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  if (int rc = pfb_validate(who, a)) return rc;
  return kPfbCfgs[0].run(who, stream, a);
}

int gsx_event_time_moe_prefill_gemm_fp8_block(void* stream, const void* A, int a_div, const void* B, void* C,
                                              const int32_t* plan, int M, int topk, int E, int N, int K,
                                              const float* scale_a, int64_t sa_stride, const float* scale_b, int iters,
                                              float* ms) {
  const char* who = "gsx_moe_prefill_gemm_fp8_block_nt";
  const PfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = pfb_validate(who, a)) return rc;
  return event_time(stream, iters, ms, [&] { return kPfbCfgs[0].run(who, stream, a); });
}

}  // extern "C"
