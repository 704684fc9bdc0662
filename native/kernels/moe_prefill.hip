// Mixture-of-experts prefill for the pod workload: the router, the tile plan, the grouped 128x128 GEMM and the combine
// at prefill row counts (1 <= M <= 32768 tokens, P = M topk pairs).  The decode forms (moe.hip, gemm_decode.hip) stop at
// 16 rows and stream weights past one MFMA fragment; here the grouped GEMM is compute-bound and an expert owns whole
// 128-row tiles.  Ids, weights, plan and scratch stay on the device: the chain needs no host synchronisation.  C ABI
// and numeric contract in gsx_kernels.h.  bf16 only here; the grouped GEMM on block-scaled fp8 operands is
// moe_prefill_fp8_block.hip, over the same plan.
//
// pf_route_kernel: 4 waves per workgroup, a wave owns a token.  moe_route_kernel's selection and weights, operation by
//   operation: a lane holds the E / 64 logits l, l + 64, .. of the row as (key << 10 | 1023 - index) + 1, topk rounds of
//   a wave maximum by xor shuffles, every lane computes the weights.  A row never leaves its wave; no LDS, no barrier.
// The plan (a stable counting sort of the pairs by expert, padded per expert to 128 rows) is three launches over
// blocks of 1024 pairs, with NB * E int32 of caller's scratch between them:
//   pf_hist_kernel   block b counts its pairs per expert in LDS (integer adds: the counts do not depend on their order)
//                    and writes hist[b][0..E); the blocks together also set every entry of rows to -1.
//   pf_scan_kernel   one workgroup, thread e: c_e = sum over b of hist[b][e], tiles_e = ceil(c_e / 128), an exclusive
//                    scan of tiles_e over e (tile_base), then hist[b][e] becomes the slot in rows of block b's first
//                    pair of expert e: 128 tile_base[e] + the pairs of e in lower blocks.  Writes header and tile_expert.
//   pf_place_kernel  block b ranks its pairs stably: a pair's rank among its wave's pairs of the same expert by 64
//                    lane reads, and the waves take their turn in order on a running count per expert in LDS.  Where a
//                    pair lands is a function of topk_ids alone; no atomic orders rows.
// pf_gemm_kernel: gemm_kernel<Bf16, 128, 128, 2, 2> (gemm_tile.h) with gathered A rows and row-scattered C; see there.
// pf_combine_kernel: a thread owns a 16-B chunk of a token's row; the topk loads are issued before the first is used.
// Contraction is off for the whole file: the router's and the combine's contracts round every multiply and add on
// its own.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>

#include "bf16_key.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "moe_prefill_plan.h"

#pragma clang fp contract(off)

namespace gsxgemm {

constexpr int PF_ROUTE_WAVES = 4;
constexpr int PF_PER_LANE = PF_MAX_E / 64;
constexpr int PF_BLOCK = 1024;  // pairs per block of the plan's passes
constexpr int PF_COMBINE_THREADS = 256;

__device__ __forceinline__ float pf_bf16(uint32_t code) { return __uint_as_float(code << 16); }

// ---------------------------------------------------------------------------
// Router
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PF_ROUTE_WAVES * 64) void pf_route_kernel(const uint16_t* __restrict__ logits,
                                                                      int64_t stride, int32_t* __restrict__ topk_ids,
                                                                      float* __restrict__ topk_w, int M, int E,
                                                                      int topk) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * PF_ROUTE_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (m >= M) return;
  const uint16_t* const row = logits + m * stride;
  uint32_t comp[PF_PER_LANE];
  static_for<PF_PER_LANE>([&](auto i) {
    const int idx = i * 64 + lane;
    comp[i] = idx < E ? ((sm_key(row[idx]) << 10) | static_cast<uint32_t>(1023 - idx)) + 1u : 0u;
  });
  int id[PF_MAX_TOPK];
  uint32_t code[PF_MAX_TOPK];
  static_for<PF_MAX_TOPK>([&](auto j) {
    id[j] = 0;
    code[j] = 0;
    if (j >= topk) return;  // uniform
    uint32_t best = 0;
#pragma unroll
    for (int i = 0; i < PF_PER_LANE; ++i) best = comp[i] > best ? comp[i] : best;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t v = __shfl_xor(best, o);
      best = v > best ? v : best;
    }
    // topk <= E: there is a logit left, so best >= 1 and the index below lies in [0, E)
#pragma unroll
    for (int i = 0; i < PF_PER_LANE; ++i) comp[i] = comp[i] == best ? 0u : comp[i];
    id[j] = 1023 - static_cast<int>((best - 1u) & 1023u);
    code[j] = row[id[j]];
  });
  // the weights: a softmax over the selected logits, in the order of j
  const float l0 = pf_bf16(code[0]);
  const bool finite0 = (code[0] & 0x7f80u) != 0x7f80u;
  float p[PF_MAX_TOPK];
  float sum = 0.f;
  static_for<PF_MAX_TOPK>([&](auto j) {
    p[j] = 0.f;
    if (j >= topk) return;
    if (!finite0) {
      p[j] = j == 0 ? 1.0f : 0.f;
    } else if ((code[j] & 0x7f80u) != 0x7f80u) {  // -inf and NaN weigh nothing
      const float d = pf_bf16(code[j]) - l0;
      const float x = d * 0x1.715476p+0f;
      p[j] = x == 0.f ? 1.0f : __builtin_amdgcn_exp2f(x);
    }
    sum = j == 0 ? p[j] : sum + p[j];
  });
  static_for<PF_MAX_TOPK>([&](auto j) {
    if (j >= topk || lane != j) return;
    const int64_t pair = static_cast<int64_t>(m) * topk + j;
    topk_ids[pair] = id[j];
    topk_w[pair] = p[j] / sum;  // sum >= p[0] = 1
  });
}

// ---------------------------------------------------------------------------
// Tile plan
// ---------------------------------------------------------------------------
__device__ __forceinline__ int pf_id(const int32_t* __restrict__ ids, int p, int P, int E) {
  if (p >= P) return -1;
  const int v = ids[p];
  return static_cast<uint32_t>(v) < static_cast<uint32_t>(E) ? v : -1;  // dropped, not clamped
}

__global__ __launch_bounds__(PF_BLOCK) void pf_hist_kernel(const int32_t* __restrict__ ids, int32_t* __restrict__ hist,
                                                           int32_t* __restrict__ rows, int P, int E, int n_rows) {
  __shared__ int32_t cnt[PF_MAX_E];
  const int t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  const int id = pf_id(ids, blockIdx.x * PF_BLOCK + t, P, E);
  if (id >= 0) atomicAdd(&cnt[id], 1);
  __syncthreads();
  if (t < E) hist[static_cast<size_t>(blockIdx.x) * E + t] = cnt[t];
  for (int i = blockIdx.x * PF_BLOCK + t; i < n_rows; i += gridDim.x * PF_BLOCK) rows[i] = -1;
}

__global__ __launch_bounds__(PF_BLOCK) void pf_scan_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ plan,
                                                           int NB, int P, int E, int T_max) {
  __shared__ int32_t scan[PF_BLOCK];
  const int t = threadIdx.x;
  int c = 0;
  if (t < E)
    for (int b = 0; b < NB; ++b) c += hist[static_cast<size_t>(b) * E + t];
  const int tiles = (c + PF_BM - 1) / PF_BM;
  scan[t] = tiles;
  __syncthreads();
  for (int o = 1; o < PF_BLOCK; o <<= 1) {  // inclusive
    const int v = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int n_tiles = scan[PF_BLOCK - 1];  // <= T_max: at most min(E, P) experts have a ragged last tile
  const int base = scan[t] - tiles;
  int32_t* const tile_expert = plan + 4;
  if (t < E) {
    int run = base * PF_BM;
    for (int b = 0; b < NB; ++b) {
      const size_t at = static_cast<size_t>(b) * E + t;
      const int v = hist[at];
      hist[at] = run;
      run += v;
    }
    for (int i = base; i < base + tiles && i < T_max; ++i) tile_expert[i] = t;
  }
  for (int i = n_tiles + t; i < T_max; i += PF_BLOCK) tile_expert[i] = -1;
  if (t == 0) {
    plan[0] = n_tiles;
    plan[1] = P;
    plan[2] = E;
    plan[3] = PF_BM;
  }
}

__global__ __launch_bounds__(PF_BLOCK) void pf_place_kernel(const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ hist,
                                                            int32_t* __restrict__ rows, int P, int E, int n_rows) {
  __shared__ int32_t next[PF_MAX_E];  // where the block's next pair of an expert goes
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  if (t < E) next[t] = hist[static_cast<size_t>(blockIdx.x) * E + t];
  const int p = blockIdx.x * PF_BLOCK + t;
  const int id = pf_id(ids, p, P, E);
  int before = 0, total = 0;  // the wave's pairs of this lane's expert: in lower lanes, in all
  for (int l = 0; l < 64; ++l) {
    const int same = __shfl(id, l) == id;
    before += same & (l < lane);
    total += same;
  }
  __syncthreads();
  for (int w = 0; w < PF_BLOCK / 64; ++w) {
    if (w == wid && id >= 0) {
      const int first = next[id];
      __builtin_amdgcn_wave_barrier();  // every lane of the wave has read before
      if (before == total - 1) next[id] = first + total;  // one lane per expert moves the count on
      const int dest = first + before;
      if (static_cast<uint32_t>(dest) < static_cast<uint32_t>(n_rows)) rows[dest] = p;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Grouped GEMM: C[p][0..N) = A[p / a_div][0..K) * B[e][N][K]^T for the pairs p of a plan tile of expert e.
//
// gemm_kernel<Bf16, 128, 128, 2, 2> with three differences:
//   * A is gathered: LDS row r of the tile holds A row rows[tile * 128 + r] / a_div.  Each lane stages 4 rows (one per
//     global_load_lds round); their 64-bit addresses are made once, before the K loop, and held in registers.  An
//     entry outside [0, P), the -1 of the padding included, points at row 0 of A: valid memory, result discarded.
//   * the epilogue goes through store_wave_tile's LDS staging, but row rr of the wave tile goes to row
//     rows[tile * 128 + wr * 64 + rr] of C (64-bit offset), and to nowhere for an entry outside [0, P).  The eight
//     entries a lane stores by are read before the K loop.
//   * the grid is (N / 128) * T_max workgroups whatever the routing: a workgroup whose tile is at or past
//     min(n_tiles, T_max), or whose tile_expert is outside [0, E), returns before its first barrier.
// Workgroup order: tile_of<128, 128, GROUP_M = 8> on T_max row tiles by N / 128 column tiles, the dense kernel's rule:
// ids are first remapped so that an XCD takes a contiguous run, then runs go group by group of 8 consecutive row tiles,
// the row tile fastest.  An expert's row tiles are consecutive, so the up to 8 workgroups that are neighbours on an XCD
// read one 128-column panel of one expert's B (where an expert has fewer tiles, of neighbouring experts), and the N / 128
// column tiles of a group re-read its 8 gathered A panels from L2.  Unused tiles sort last and leave at once.
// Summation order per output element: K-tiles in order and within one the two MFMA k-steps in order, as gemm_kernel.
// ---------------------------------------------------------------------------
constexpr int PF_GROUP_M = 8;
constexpr int PF_TILE = PF_BM * ROW_BYTES;  // bytes per operand tile (BM == BN)
constexpr int PF_LDS = 2 * 2 * PF_TILE;     // [buf][A|B]

__global__ __launch_bounds__(256) void pf_gemm_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                      uint16_t* __restrict__ C, const int32_t* __restrict__ plan,
                                                      int T_max, int P, int E, int a_div, int N, int K) {
  constexpr int BK = Bf16::BK, NW = 4, WN = 2, WT = 64, MR = 4, NR = 4, R = PF_TILE / 1024 / NW;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WN, wc = wid % WN;

  int tm, tn;
  tile_of<PF_BM, PF_BN, PF_GROUP_M>(blockIdx.x, gridDim.x, T_max * PF_BM, N, tm, tn);
  const int n_tiles = plan[0];
  if (tm >= (n_tiles < T_max ? n_tiles : T_max)) return;  // a negative n_tiles: every tile
  const int e = plan[4 + tm];
  if (static_cast<uint32_t>(e) >= static_cast<uint32_t>(E)) return;
  const int32_t* const rows = plan + 4 + T_max + static_cast<size_t>(tm) * PF_BM;
  const int col0 = tn * PF_BN;

  int off[R];             // B: as gemm_kernel
  const uint16_t* ar[R];  // A: the lane's row of round i, at the chunk its LDS slot holds
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int p = (i * NW + wid) * 64 + lane;
    off[i] = (p >> 3) * K + glds_col<uint16_t>(p);
    const int pair = rows[p >> 3];
    const int src = static_cast<uint32_t>(pair) < static_cast<uint32_t>(P) ? pair / a_div : 0;
    ar[i] = A + static_cast<size_t>(src) * K + glds_col<uint16_t>(p);
  }
  int crow[WT / 8];  // the pair of wave-tile row 8 i + lane / 8
#pragma unroll
  for (int i = 0; i < WT / 8; ++i) crow[i] = rows[wr * WT + i * 8 + (lane >> 3)];
  const uint16_t* Bb = B + (static_cast<size_t>(e) * N + col0) * K;

  auto stage = [&](int kt, int buf) {
    char* la = lds + buf * 2 * PF_TILE;
    char* lb = la + PF_TILE;
#pragma unroll
    for (int i = 0; i < R; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(ar[i] + kt * BK), (lptr_t)(la + (i * NW + wid) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < R; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * BK), (lptr_t)(lb + (i * NW + wid) * 1024), 16, 0,
                                       0);
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
    const char* la = lds + buf * 2 * PF_TILE;
    const char* lb = la + PF_TILE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 bfr[NR];
#pragma unroll
      for (int n = 0; n < NR; ++n)
        bfr[n] = *reinterpret_cast<const bf16x8*>(lb + swz(wc * WT + n * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(la + swz(wr * WT + m * 16 + fr, kk * 4 + fq));
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < NR; ++n) Bf16::mma(acc[m][n], &af, &bfr[n]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
  }
  uint16_t* ct = reinterpret_cast<uint16_t*>(lds + wid * (WT * WT * 2));
  scatter16<WT>(ct, acc, fr, fq);
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < WT / 8; ++i) {
    const int rr = i * 8 + (lane >> 3), cc = (lane & 7) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(ct + rr * WT + cc);
    if (static_cast<uint32_t>(crow[i]) < static_cast<uint32_t>(P))
      *reinterpret_cast<uint4*>(C + static_cast<size_t>(crow[i]) * N + col0 + wc * WT + cc) = v;
  }
}

// ---------------------------------------------------------------------------
// Combine
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PF_COMBINE_THREADS) void pf_combine_kernel(const uint16_t* __restrict__ Y,
                                                                        int64_t y_stride,
                                                                        const float* __restrict__ topk_w,
                                                                        uint16_t* __restrict__ out, int64_t out_stride,
                                                                        int topk, int H) {
  const int c = blockIdx.x * PF_COMBINE_THREADS + threadIdx.x;
  if (c >= (H >> 3)) return;
  const int64_t m = blockIdx.y;
  i32x4 yv[PF_MAX_TOPK];
  float w[PF_MAX_TOPK];
  static_for<PF_MAX_TOPK>([&](auto j) {
    if (j >= topk) return;
    yv[j] = *reinterpret_cast<const i32x4*>(Y + (m * topk + j) * y_stride + 8 * static_cast<int64_t>(c));
    w[j] = topk_w[m * topk + j];
  });
  float acc[8];
  static_for<PF_MAX_TOPK>([&](auto j) {
    if (j >= topk) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t word = static_cast<uint32_t>(yv[j][e >> 1]);
      const float y = __uint_as_float((e & 1) ? word & 0xffff0000u : word << 16);
      const float prod = w[j] * y;
      acc[e] = j == 0 ? prod : acc[e] + prod;
    }
  });
  i32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = static_cast<int>(f2bf(acc[2 * i]) | (static_cast<uint32_t>(f2bf(acc[2 * i + 1])) << 16));
  *reinterpret_cast<i32x4*>(out + m * out_stride + 8 * static_cast<int64_t>(c)) = o;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

// PfSpan, pf_overlap, pf_bits, pf_refuse, pf_sizes, pf_tmax and pf_plan_ints: moe_prefill_plan.h

static int pf_blocks(int M, int topk) { return (M * topk + PF_BLOCK - 1) / PF_BLOCK; }
static uint64_t pf_ws_bytes(int M, int topk, int E) { return static_cast<uint64_t>(pf_blocks(M, topk)) * E * 4; }

struct PfRouteArgs {
  const void* logits;
  int64_t stride;
  int32_t* ids;
  float* w;
  int M, E, topk;
};

static int pf_route_validate(const char* who, const PfRouteArgs& a) {
  if (int rc = pf_sizes(who, a.M, a.topk, a.E)) return rc;
  if (a.stride < a.E || a.stride % 8) return pf_refuse(who, "need logits_stride >= E and logits_stride % 8 == 0");
  if (!a.logits || !a.ids || !a.w) return pf_refuse(who, "logits, topk_ids and topk_w must not be NULL");
  if (pf_bits(a.logits) % 16) return pf_refuse(who, "logits must be 16-B aligned");
  if ((pf_bits(a.ids) | pf_bits(a.w)) % 4) return pf_refuse(who, "topk_ids and topk_w must be 4-B aligned");
  const uint64_t pairs = static_cast<uint64_t>(a.M) * a.topk;
  const PfSpan lg{a.logits, (static_cast<uint64_t>(a.M - 1) * a.stride + a.E) * 2}, id{a.ids, pairs * 4},
      w{a.w, pairs * 4};
  if (pf_overlap(id, lg) || pf_overlap(w, lg) || pf_overlap(id, w))
    return pf_refuse(who, "topk_ids and topk_w must not overlap logits or each other");
  return 0;
}

static int pf_route_run(const char* who, void* stream, const PfRouteArgs& a) {
  hipLaunchKernelGGL(pf_route_kernel, dim3((a.M + PF_ROUTE_WAVES - 1) / PF_ROUTE_WAVES), dim3(PF_ROUTE_WAVES * 64), 0,
                     S(stream), static_cast<const uint16_t*>(a.logits), a.stride, a.ids, a.w, a.M, a.E, a.topk);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct PfPlanArgs {
  const int32_t* ids;
  int32_t* plan;
  int M, topk, E;
  void* ws;
  uint64_t ws_bytes;
};

static int pf_plan_validate(const char* who, const PfPlanArgs& a) {
  if (int rc = pf_sizes(who, a.M, a.topk, a.E)) return rc;
  if (!a.ids || !a.plan || !a.ws) return pf_refuse(who, "topk_ids, plan and workspace must not be NULL");
  if ((pf_bits(a.ids) | pf_bits(a.plan) | pf_bits(a.ws)) % 4)
    return pf_refuse(who, "topk_ids, plan and workspace must be 4-B aligned");
  const uint64_t need = pf_ws_bytes(a.M, a.topk, a.E);
  if (a.ws_bytes < need) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%s: workspace too small: need %llu bytes", who,
                  static_cast<unsigned long long>(need));
    return fail_arg(msg);
  }
  const PfSpan id{a.ids, static_cast<uint64_t>(a.M) * a.topk * 4}, pl{a.plan, pf_plan_ints(a.M, a.topk, a.E) * 4},
      ws{a.ws, need};
  if (pf_overlap(pl, id) || pf_overlap(ws, id) || pf_overlap(pl, ws))
    return pf_refuse(who, "plan and workspace must not overlap topk_ids or each other");
  return 0;
}

static int pf_plan_run(const char* who, void* stream, const PfPlanArgs& a) {
  const int P = a.M * a.topk, NB = pf_blocks(a.M, a.topk), T_max = static_cast<int>(pf_tmax(a.M, a.topk, a.E));
  const int n_rows = T_max * PF_BM;
  int32_t* const hist = static_cast<int32_t*>(a.ws);
  int32_t* const rows = a.plan + 4 + T_max;
  hipLaunchKernelGGL(pf_hist_kernel, dim3(NB), dim3(PF_BLOCK), 0, S(stream), a.ids, hist, rows, P, a.E, n_rows);
  hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(PF_BLOCK), 0, S(stream), hist, a.plan, NB, P, a.E, T_max);
  hipLaunchKernelGGL(pf_place_kernel, dim3(NB), dim3(PF_BLOCK), 0, S(stream), a.ids, hist, rows, P, a.E, n_rows);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct PfGemmArgs {
  const void* A;
  int a_div;
  const void* B;
  void* C;
  const int32_t* plan;
  int M, topk, E, N, K;
};

static int pf_gemm_validate(const char* who, const PfGemmArgs& a) {
  if (int rc = pf_sizes(who, a.M, a.topk, a.E)) return rc;
  if (a.a_div < 1) return pf_refuse(who, "need a_div >= 1");
  if (a.N <= 0 || a.N % PF_BN || a.K <= 0 || a.K % Bf16::BK) return pf_refuse(who, "need N%128==0, K%64==0");
  if (!a.A || !a.B || !a.C || !a.plan) return pf_refuse(who, "A, B, C and plan must not be NULL");
  if ((pf_bits(a.A) | pf_bits(a.B) | pf_bits(a.C)) % 16) return pf_refuse(who, "operands must be 16-B aligned");
  if (pf_bits(a.plan) % 4) return pf_refuse(who, "plan must be 4-B aligned");
  // a lane's offset inside a B tile is an int, as in the dense launcher
  if (static_cast<int64_t>(PF_BN - 1) * a.K + (Bf16::BK - 8) > INT32_MAX)
    return pf_refuse(who, "K too large: 128 rows of K elements must stay below 2^31");
  if (pf_tmax(a.M, a.topk, a.E) * (a.N / PF_BN) > INT32_MAX)
    return pf_refuse(who, "N too large: (N / 128) * T_max workgroups must stay below 2^31");
  const uint64_t P = static_cast<uint64_t>(a.M) * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const PfSpan c{a.C, P * a.N * 2};
  const PfSpan in[] = {{a.A, a_rows * a.K * 2},
                       {a.B, static_cast<uint64_t>(a.E) * a.N * a.K * 2},
                       {a.plan, pf_plan_ints(a.M, a.topk, a.E) * 4}};
  for (const PfSpan& s : in)
    if (pf_overlap(c, s)) return pf_refuse(who, "C must not overlap A, B or plan");
  return 0;
}

static int pf_gemm_run(const char* who, void* stream, const PfGemmArgs& a) {
  // 64 KiB of dynamic LDS has to be asked for, per device, as in the dense launcher (gemm_tile.h)
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (int rc = current_device(who, &dev)) return rc;
  if (!attr[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pf_gemm_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS);
    if (e != hipSuccess) return fail(e, who);
    attr[dev].store(true, std::memory_order_release);
  }
  const int T_max = static_cast<int>(pf_tmax(a.M, a.topk, a.E));
  hipLaunchKernelGGL(pf_gemm_kernel, dim3(T_max * (a.N / PF_BN)), dim3(256), PF_LDS, S(stream),
                     static_cast<const uint16_t*>(a.A), static_cast<const uint16_t*>(a.B), static_cast<uint16_t*>(a.C),
                     a.plan, T_max, a.M * a.topk, a.E, a.a_div, a.N, a.K);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct PfGemmCfg {
  const char* name;
  int bm, bn, waves;
  int (*run)(const char* who, void* stream, const PfGemmArgs& a);
};
constexpr PfGemmCfg kPfGemmCfgs[] = {{"128x128/4w-gather", PF_BM, PF_BN, 4, &pf_gemm_run}};
constexpr int kNumPfGemmCfgs = sizeof(kPfGemmCfgs) / sizeof(kPfGemmCfgs[0]);
static const PfGemmCfg* pf_gemm_row(int cfg) { return cfg >= 0 && cfg < kNumPfGemmCfgs ? &kPfGemmCfgs[cfg] : nullptr; }

struct PfCombineArgs {
  const void* Y;
  int64_t y_stride;
  const float* w;
  void* out;
  int64_t out_stride;
  int M, topk, H;
};

static int pf_combine_validate(const char* who, const PfCombineArgs& a) {
  if (a.M < 1 || a.M > PF_MAX_M) return pf_refuse(who, "need 1 <= M <= 32768");
  if (a.topk < 1 || a.topk > PF_MAX_TOPK) return pf_refuse(who, "need 1 <= topk <= 8");
  if (a.H < 8 || a.H % 8) return pf_refuse(who, "need H >= 8 and H % 8 == 0");
  if (a.y_stride < a.H || a.y_stride % 8) return pf_refuse(who, "need y_stride >= H and y_stride % 8 == 0");
  if (a.out_stride < a.H || a.out_stride % 8) return pf_refuse(who, "need out_stride >= H and out_stride % 8 == 0");
  if (!a.Y || !a.w || !a.out) return pf_refuse(who, "Y, topk_w and out must not be NULL");
  if ((pf_bits(a.Y) | pf_bits(a.out)) % 16) return pf_refuse(who, "Y and out must be 16-B aligned");
  if (pf_bits(a.w) % 4) return pf_refuse(who, "topk_w must be 4-B aligned");
  const uint64_t pairs = static_cast<uint64_t>(a.M) * a.topk, h = static_cast<uint64_t>(a.H);
  const PfSpan y{a.Y, ((pairs - 1) * a.y_stride + h) * 2}, w{a.w, pairs * 4},
      o{a.out, (static_cast<uint64_t>(a.M - 1) * a.out_stride + h) * 2};
  if (pf_overlap(o, y) || pf_overlap(o, w)) return pf_refuse(who, "out must not overlap Y or topk_w");
  return 0;
}

static int pf_combine_run(const char* who, void* stream, const PfCombineArgs& a) {
  const dim3 grid((a.H / 8 + PF_COMBINE_THREADS - 1) / PF_COMBINE_THREADS, a.M);
  hipLaunchKernelGGL(pf_combine_kernel, grid, dim3(PF_COMBINE_THREADS), 0, S(stream),
                     static_cast<const uint16_t*>(a.Y), a.y_stride, a.w, static_cast<uint16_t*>(a.out), a.out_stride,
                     a.topk, a.H);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

int gsx_moe_prefill_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids, float* topk_w,
                          int M, int E, int topk) {
  const PfRouteArgs a{logits, logits_stride, topk_ids, topk_w, M, E, topk};
  if (int rc = pf_route_validate("gsx_moe_prefill_route", a)) return rc;
  return pf_route_run("gsx_moe_prefill_route", stream, a);
}

int gsx_event_time_moe_prefill_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids,
                                     float* topk_w, int M, int E, int topk, int iters, float* ms) {
  const PfRouteArgs a{logits, logits_stride, topk_ids, topk_w, M, E, topk};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = pf_route_validate("gsx_moe_prefill_route", a)) return rc;
  return event_time(stream, iters, ms, [&] { return pf_route_run("gsx_moe_prefill_route", stream, a); });
}

int gsx_moe_prefill_plan_ints(int M, int topk, int E, uint64_t* ints) {
  const char* who = "gsx_moe_prefill_plan_ints";
  if (!ints) return pf_refuse(who, "ints must not be NULL");
  if (int rc = pf_sizes(who, M, topk, E)) return rc;
  *ints = pf_plan_ints(M, topk, E);
  return 0;
}

int gsx_moe_prefill_workspace_bytes(int M, int topk, int E, uint64_t* bytes) {
  const char* who = "gsx_moe_prefill_workspace_bytes";
  if (!bytes) return pf_refuse(who, "bytes must not be NULL");
  if (int rc = pf_sizes(who, M, topk, E)) return rc;
  *bytes = pf_ws_bytes(M, topk, E);
  return 0;
}

int gsx_moe_prefill_plan(void* stream, const int32_t* topk_ids, int32_t* plan, int M, int topk, int E, void* workspace,
                         uint64_t workspace_bytes) {
  const PfPlanArgs a{topk_ids, plan, M, topk, E, workspace, workspace_bytes};
  if (int rc = pf_plan_validate("gsx_moe_prefill_plan", a)) return rc;
  return pf_plan_run("gsx_moe_prefill_plan", stream, a);
}

int gsx_event_time_moe_prefill_plan(void* stream, const int32_t* topk_ids, int32_t* plan, int M, int topk, int E,
                                    void* workspace, uint64_t workspace_bytes, int iters, float* ms) {
  const PfPlanArgs a{topk_ids, plan, M, topk, E, workspace, workspace_bytes};
  if (int rc = pf_plan_validate("gsx_moe_prefill_plan", a)) return rc;
  return event_time(stream, iters, ms, [&] { return pf_plan_run("gsx_moe_prefill_plan", stream, a); });
}

const char* gsx_moe_prefill_gemm_cfg_name(int cfg) { return pf_gemm_row(cfg) ? pf_gemm_row(cfg)->name : nullptr; }

int gsx_moe_prefill_gemm_cfg_shape(int cfg, int* bm, int* bn, int* waves) {
  const PfGemmCfg* c = pf_gemm_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  *waves = c->waves;
  return 0;
}

int gsx_moe_prefill_gemm_nt_launch_cfg(void* stream, const void* A, int a_div, const void* B, void* C,
                                       const int32_t* plan, int M, int topk, int E, int N, int K, int cfg) {
  const char* who = "gsx_moe_prefill_gemm_nt_launch_cfg";
  const PfGemmCfg* c = pf_gemm_row(cfg);
  if (!c) return fail_arg("gsx_moe_prefill_gemm_nt_launch_cfg: unknown config");
  const PfGemmArgs a{A, a_div, B, C, plan, M, topk, E, N, K};
  if (int rc = pf_gemm_validate(who, a)) return rc;
  return c->run(who, stream, a);
}

int gsx_moe_prefill_gemm_nt(void* stream, const void* A, int a_div, const void* B, void* C, const int32_t* plan, int M,
                            int topk, int E, int N, int K) {
  const PfGemmArgs a{A, a_div, B, C, plan, M, topk, E, N, K};
  if (int rc = pf_gemm_validate("gsx_moe_prefill_gemm_nt", a)) return rc;
  return kPfGemmCfgs[0].run("gsx_moe_prefill_gemm_nt", stream, a);
}

int gsx_event_time_moe_prefill_gemm(void* stream, const void* A, int a_div, const void* B, void* C,
                                    const int32_t* plan, int M, int topk, int E, int N, int K, int iters, float* ms) {
  const PfGemmArgs a{A, a_div, B, C, plan, M, topk, E, N, K};
  if (int rc = pf_gemm_validate("gsx_moe_prefill_gemm_nt", a)) return rc;
  return event_time(stream, iters, ms, [&] { return kPfGemmCfgs[0].run("gsx_moe_prefill_gemm_nt", stream, a); });
}

int gsx_moe_prefill_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out,
                            int64_t out_stride, int M, int topk, int H) {
  const PfCombineArgs a{Y, y_stride, topk_w, out, out_stride, M, topk, H};
  if (int rc = pf_combine_validate("gsx_moe_prefill_combine", a)) return rc;
  return pf_combine_run("gsx_moe_prefill_combine", stream, a);
}

int gsx_event_time_moe_prefill_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out,
                                       int64_t out_stride, int M, int topk, int H, int iters, float* ms) {
  const PfCombineArgs a{Y, y_stride, topk_w, out, out_stride, M, topk, H};
  if (int rc = pf_combine_validate("gsx_moe_prefill_combine", a)) return rc;
  return event_time(stream, iters, ms, [&] { return pf_combine_run("gsx_moe_prefill_combine", stream, a); });
}

}  // extern "C"
