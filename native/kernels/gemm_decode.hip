// Decode GEMM family for the pod workload: C[M][N] (bf16) = A[M][K] * B[N][K]^T with 1 <= M <= 16, the shape of an
// inference server's decode phase.  A few activation rows meet weights that are read once: the work is bound by HBM
// bandwidth, not by the matrix cores.  Operands are those of the three GEMM families (bf16; OCP e4m3 with the fp32
// scales of gemm_fp8.hip; e2m1 with e8m0 block scales as in gemm_mxfp4.hip), the MFMAs gemm_tile.h's operand kinds
// Bf16, Fp8K128 and Mxfp4 with its fragment convention: lane (fr, fq) holds chunks fq and 4 + fq of its row of a
// 128-B K-tile row.  C ABI in gsx_kernels.h.
//
// One kernel, decode_kernel:
//   * a workgroup owns a strip of BN = 16 NF columns of C (NF fragments) over all of K; the grid is N / BN strips
//     and nothing passes between workgroups;
//   * its W waves split the strip's K-tiles, interleaved: wave w takes tiles w, w + W, ..., so the workgroup as a
//     whole walks its rows of B front to back;
//   * B goes from global memory to VGPRs in fragment shape, two 16-B loads per lane, fragment and K-tile, with no
//     LDS in between; a wave keeps F K-tiles in flight in a register ring and waits for a tile (a counted vmcnt,
//     which the compiler places) just before the tile's MFMAs;
//   * A comes in the same shape (it is small and stays in L2), through bounds-checked buffer loads whose range is
//     exactly the M rows: a lane whose row is >= M gets zeros from the hardware, in registers, and no access to
//     memory is made for it.  That is a predicate on the load without a branch.  With a branch around the loads of
//     a lane's row the compiler waits vmcnt(0) in front of every K-tile's MFMAs instead of leaving F - 1 tiles in
//     flight, and the mxfp4 kernel needs 176 VGPRs instead of 103.  Configuration "16/8w-f4-masked" keeps that
//     form: it is the ablation (mxfp4 5 to 21 % slower in 8 of 9 shapes, bf16 and fp8 within 4 %: other waves of
//     the CU cover the wait), and what every configuration falls back to when 16 rows of A do not fit a buffer's
//     32-bit range, K >= 2^27 in bf16.  scale_a likewise.  Rows >= M of C are not stored;
//   * MXFP4: a lane reads the 8 scale codes of its row and K-tile with one 8-B load (four lanes per address) and
//     shifts byte fq (first MFMA of the tile) or byte 4 + fq (second) down to byte 0, which is the byte select of
//     every MFMA;
//   * the waves' fp32 accumulators meet in LDS and wave 0 adds them in the order of the wave index, applies the fp8
//     scales, (acc * sa) * sb, converts once (f2bf) and stores.
// So the result does not depend on where or when a workgroup runs; its summation order, K-tiles w, w + W, ... within
// a wave and then the waves in order, is not the one of gsx_gemm_*_nt.
// Row offsets into B, scale_b and C are 64-bit; the offset inside a row is an int (K is an int).
//
// The configurations (one table for the three kinds) vary W, F, BN and the cache policy of the loads of B; the
// dispatch rule and the measurements behind it are at decode_pick() below and in profiles/gemm_decode/README.md.
//
// The grouped form (gsx_moe_gemm_nt, for a mixture of experts) is the same kernel with GRP = MoePlan: a workgroup is
// (strip, slot of a plan in device memory), its fragment rows are the slot's (token, expert) pairs, A's rows are
// gathered by the offset of the same buffer load, B is the slot's expert, and stores go to the pairs' rows of C.  The
// K loop, the ring, the waves' split of K and the reduction are shared, so a row has the bits the plain kernel gives
// it; with GRP = NoGroup every `if constexpr (GROUPED)` falls away and the plain instantiations have the registers,
// LDS and scratch they had (profiles/gemm_decode/README.md; profiles/moe/README.md has the grouped ones).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

// one 16-B chunk from global memory; NT: with the non-temporal hint (the line is not kept for a second use)
template <class FRAG, bool NT>
__device__ __forceinline__ FRAG load_chunk(const void* p) {
  const i32x4* q = static_cast<const i32x4*>(p);
  const i32x4 v = NT ? __builtin_nontemporal_load(q) : *q;
  return __builtin_bit_cast(FRAG, v);
}

// A raw buffer over `bytes` bytes at `base`: a load at or past the end returns zeros and touches nothing.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_buffer(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, static_cast<int>(bytes), 0x00020000);
}

// What the grouped form (gsx_moe_gemm_nt) passes instead of NoGroup: a plan in device memory, which gsx_moe_route
// wrote, or anyone.  Workgroup (strip, slot); grid.y is min(E, P) <= 128.
struct MoePlan {
  const int32_t* plan;
  int P, E, a_div, a_rows;
};
struct NoGroup {};
// A workgroup's slot of the plan.  Fragment row r < M (the slot's clamped count) is pair rows[begin + r]; the pair
// reads row pair / a_div of A's a_rows rows, meets expert `expert` of B and of scale_b, and is stored to row `pair`
// of C.
struct MoeGroup {
  const int32_t* rows;  // the plan's rows[GSX_MOE_MAX_PAIRS]
  int begin, P, a_div, a_rows;
  size_t expert;
};

// The pair of fragment row r, or -1: an index into rows outside [0, 128) and a pair outside [0, P) are dropped.
__device__ __forceinline__ int moe_pair(const MoeGroup& g, int r, int M) {
  const uint32_t idx = static_cast<uint32_t>(g.begin) + static_cast<uint32_t>(r);
  if (r >= M || idx >= static_cast<uint32_t>(GSX_MOE_MAX_PAIRS)) return -1;
  const int p = g.rows[idx];
  return p >= 0 && p < g.P ? p : -1;
}

// MASKED: the loads of A and scale_a are plain loads inside `if (row < M)` instead of buffer loads.
// GRP = MoePlan (never MASKED) is the grouped form: M is not passed but read, the slot's count; rows of A and C and the
// expert of B come from the plan; the buffer over A covers all its a_rows rows, and a lane without a pair gets an
// offset at its end.  A slot at or past n_active, one whose expert is outside [0, E) and one without a row return
// before any barrier and read nothing of B; the count is clamped to 16, and moe_pair() drops what the rows of the plan
// must not name.
template <class OP, int NF, int W, int F, bool NT, bool MASKED, class GRP, typename... EP>
__global__ __launch_bounds__(W * 64) void decode_kernel(const typename OP::elem* __restrict__ A,
                                                       const typename OP::elem* __restrict__ B,
                                                       uint16_t* __restrict__ C, int M, int N, int K, GRP gp,
                                                       EP... ep) {
  constexpr bool GROUPED = std::is_same_v<GRP, MoePlan>;
  static_assert(!(GROUPED && MASKED), "the grouped form has no masked form");
  [[maybe_unused]] MoeGroup grp{};
  if constexpr (GROUPED) {
    constexpr int S = GSX_MOE_MAX_PAIRS;
    const int slot = blockIdx.y;
    if (slot >= gp.plan[0] || slot >= S) return;
    const int e = gp.plan[4 + slot];
    if (e < 0 || e >= gp.E) return;
    const int count = gp.plan[4 + 2 * S + slot];
    if (count <= 0) return;
    M = count > 16 ? 16 : count;
    grp = MoeGroup{gp.plan + 4 + 3 * S, gp.plan[4 + S + slot], gp.P, gp.a_div, gp.a_rows, static_cast<size_t>(e)};
  }
  using T = typename OP::elem;
  using frag = typename OP::frag;
  constexpr int CH = OP::CH;
  constexpr bool MX = OP::MX;
  constexpr int BKU = OP::BK / OP::EPU;                      // a K-tile in units of T: 128 B
  constexpr int CU = CHUNK / static_cast<int>(sizeof(T));    // a chunk in units of T
  const int ld = K / OP::EPU, nk = K / OP::BK;
  __shared__ f32x4 red[W][NF][64];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const size_t col0 = static_cast<size_t>(blockIdx.x) * (NF * 16);
  const int mine = wid < nk ? (nk - wid + W - 1) / W : 0;  // K-tiles wid, wid + W, ...: tile j of the wave
  const bool arow = fr < M;

  // the lane's row of every operand, at chunk fq of K-tile 0.  A's as a pointer only where the row exists (MASKED),
  // otherwise as a byte offset into the buffer of A's M rows, which is past its end for a row >= M
  [[maybe_unused]] const T* ap = A + (arow ? static_cast<size_t>(fr) * ld : 0) + fq * CU;
  const uint32_t arow_bytes = static_cast<uint32_t>(ld) * sizeof(T);
  // grouped: the pair's row of A's a_rows rows, or a_rows (the end of the buffer) for a lane without a pair
  [[maybe_unused]] uint32_t ar = 0, an = 0;
  if constexpr (GROUPED) {
    const int p = moe_pair(grp, fr, M);
    an = static_cast<uint32_t>(grp.a_rows);
    ar = p >= 0 ? static_cast<uint32_t>(p / grp.a_div) : an;
    B += grp.expert * static_cast<size_t>(N) * ld;
  }
  const __amdgpu_buffer_rsrc_t abuf = rows_buffer(A, GROUPED ? an * arow_bytes : M * arow_bytes);
  const int aoff = static_cast<int>((GROUPED ? ar * arow_bytes : fr * arow_bytes) + fq * CHUNK);
  const T* bp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) bp[f] = B + (col0 + f * 16 + fr) * ld + fq * CU;
  [[maybe_unused]] const uint8_t* sap = nullptr;
  [[maybe_unused]] const uint8_t* sbp[NF] = {};
  [[maybe_unused]] __amdgpu_buffer_rsrc_t sabuf = abuf;
  if constexpr (MX) {
    const auto mx = from_args<MxArgs, MX>(ep...);
    sap = mx.sa + (arow ? static_cast<size_t>(fr) * (K / 32) : 0);
    // 1 / 16 of A's bytes
    sabuf = rows_buffer(mx.sa, (GROUPED ? an : static_cast<uint32_t>(M)) * (K / 32));
    const uint8_t* sb = mx.sb;
    if constexpr (GROUPED) sb += grp.expert * static_cast<size_t>(N) * (K / 32);
#pragma unroll
    for (int f = 0; f < NF; ++f) sbp[f] = sb + (col0 + f * 16 + fr) * (K / 32);
  }

  // the ring: slot i holds one K-tile's fragments of A and of B, and for MX the 8 codes of the lane's rows
  frag ra[F][2], rb[F][NF][2];
  [[maybe_unused]] i32x2 rsa[F], rsb[F][NF];
  [[maybe_unused]] const frag zero = __builtin_bit_cast(frag, i32x4{0, 0, 0, 0});

  auto load = [&](auto slot, int j) {
    constexpr int i = decltype(slot)::value;
    const int kt = wid + j * W;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int c = 0; c < 2; ++c) rb[i][f][c] = load_chunk<frag, NT>(bp[f] + kt * BKU + c * 4 * CU);
    if constexpr (MX) {
#pragma unroll
      for (int f = 0; f < NF; ++f) rsb[i][f] = *reinterpret_cast<const i32x2*>(sbp[f] + kt * MX_ROW);
    }
    if constexpr (MASKED) {
      ra[i][0] = ra[i][1] = zero;
      if constexpr (MX) rsa[i] = i32x2{0, 0};
      if (arow) {
#pragma unroll
        for (int c = 0; c < 2; ++c) ra[i][c] = load_chunk<frag, false>(ap + kt * BKU + c * 4 * CU);
        if constexpr (MX) rsa[i] = *reinterpret_cast<const i32x2*>(sap + kt * MX_ROW);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        ra[i][c] = __builtin_bit_cast(
            frag, __builtin_amdgcn_raw_buffer_load_b128(abuf, aoff + c * 4 * CHUNK, kt * ROW_BYTES, 0));
      if constexpr (MX)
        rsa[i] = __builtin_bit_cast(
            i32x2, __builtin_amdgcn_raw_buffer_load_b64(
                       sabuf, GROUPED ? static_cast<int>(ar * (K / 32)) : fr * (K / 32), kt * MX_ROW, 0));
    }
  };

  f32x4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mma = [&](auto slot) {
    constexpr int i = decltype(slot)::value;
#pragma unroll
    for (int kk = 0; kk < 2 / CH; ++kk) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if constexpr (MX) {
          const int sa = static_cast<int>(static_cast<uint32_t>(kk ? rsa[i].y : rsa[i].x) >> (8 * fq));
          const int sb = static_cast<int>(static_cast<uint32_t>(kk ? rsb[i][f].y : rsb[i][f].x) >> (8 * fq));
          OP::template mma<0, 0>(acc[f], &ra[i][kk], &rb[i][f][kk], sa, sb);
        } else {
          OP::mma(acc[f], &ra[i][kk * CH], &rb[i][f][kk * CH]);
        }
      }
    }
  };

  // Slot i holds tile t + i until its MFMAs, then tile t + i + F.  The steady loop has no condition inside: every
  // slot is consumed and refilled.  It is entered only behind an unconditional prologue, so that on every path to its
  // top the F tiles were issued in slot order and the wait for slot 0 leaves the F - 1 younger tiles in flight.  The
  // last 2 F - 1 tiles or fewer (all of them, for a short K) drain in two conditional passes.
  int t = 0;
  if (mine >= 2 * F) {
    static_for<F>([&](auto i) {
      load(i, i);
      __builtin_amdgcn_sched_barrier(0);  // tile by tile, as in the loop: its waits are counted from this order too
    });
    do {
      static_for<F>([&](auto i) {
        mma(i);
        load(i, t + i + F);
        // keep the slots in this order: left alone the scheduler gathers the MFMAs of all slots in front of all the
        // loads, and the wait for the first becomes a wait for everything
        __builtin_amdgcn_sched_barrier(0);
      });
      t += F;
    } while (t + 2 * F <= mine);
  } else {
    static_for<F>([&](auto i) {
      if (i < mine) load(i, i);
    });
  }
  static_for<F>([&](auto i) {
    if (t + i < mine) {
      mma(i);
      if (t + i + F < mine) load(i, t + i + F);
    }
  });
  static_for<F>([&](auto i) {
    if (t + F + i < mine) mma(i);
  });

  // a wave without a tile contributes its zeros
#pragma unroll
  for (int f = 0; f < NF; ++f) red[wid][f][lane] = acc[f];
  __syncthreads();
  if (wid != 0) return;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f32x4 s = red[0][f][lane];
#pragma unroll
    for (int w = 1; w < W; ++w) {
      const f32x4 v = red[w][f][lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += v[j];
    }
    // 16x16 C map: column fr, row 4 fq + j
    const size_t col = col0 + f * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = fq * 4 + j;
      if (row >= M) continue;
      float v = s[j];
      if constexpr (GROUPED) {
        const int p = moe_pair(grp, row, M);
        if (p < 0) continue;
        if constexpr (!MX && sizeof...(EP) != 0) {  // a scale per row of A and per (expert, column), or none
          const auto sc = from_args<Scaled, true>(ep...);
          if (sc.sa != nullptr) v = (v * sc.sa[p / grp.a_div]) * sc.sb[grp.expert * static_cast<size_t>(N) + col];
        }
        C[static_cast<size_t>(p) * N + col] = f2bf(v);
      } else {
        if constexpr (!MX && sizeof...(EP) != 0) {
          const auto sc = from_args<Scaled, true>(ep...);
          if (sc.sa != nullptr) v = (v * sc.sa[static_cast<size_t>(row) * sc.stride]) * sc.sb[col * sc.stride];
        }
        C[static_cast<size_t>(row) * N + col] = f2bf(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

constexpr int kDecodeKinds = 3;
constexpr int kDecodeKTile[kDecodeKinds] = {Bf16::BK, Fp8K128::BK, Mxfp4::BK};  // indexed by GSX_DECODE_*

// Everything the entry points refuse, before the first device call.  `bn`: the columns of a strip.
static int decode_validate(const char* who, int kind, int bn, const void* A, const void* B, const void* C, int M,
                           int N, int K, const void* sa, const void* sb, int mode) {
  char msg[160];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (kind < 0 || kind >= kDecodeKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, kind);
    return fail_arg(msg);
  }
  if (M < 1 || M > 16) return refuse("need 1 <= M <= 16");
  if (N <= 0 || N % bn || K <= 0 || K % kDecodeKTile[kind]) {
    std::snprintf(msg, sizeof(msg), "%s: need N%%%d==0, K%%%d==0", who, bn, kDecodeKTile[kind]);
    return fail_arg(msg);
  }
  if (!A || !B || !C) return refuse("A, B and C must not be NULL");
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) % 16)
    return refuse("operands must be 16-B aligned");
  const uintptr_t sbits = reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb);
  if (kind == GSX_DECODE_BF16) {
    if (sa || sb || mode != GSX_GEMM_SCALE_NONE)
      return refuse("bf16 takes no scales: scale_a and scale_b must be NULL and scale_mode NONE");
  } else if (kind == GSX_DECODE_FP8) {
    if (mode != GSX_GEMM_SCALE_NONE && mode != GSX_GEMM_SCALE_TENSOR && mode != GSX_GEMM_SCALE_ROW) {
      std::snprintf(msg, sizeof(msg), "%s: unknown scale_mode %d", who, mode);
      return fail_arg(msg);
    }
    if (mode != GSX_GEMM_SCALE_NONE) {
      if (!sa || !sb) return refuse("scale_a and scale_b must not be NULL in this scale_mode");
      if (sbits % 4) return refuse("scale_a and scale_b must be 4-B aligned");
    }
  } else {
    if (mode != GSX_GEMM_SCALE_NONE) return refuse("mxfp4 takes scale_mode NONE: its scales are the e8m0 blocks");
    if (!sa || !sb) return refuse("scale_a and scale_b must not be NULL");
    if (sbits % 16) return refuse("scale_a and scale_b must be 16-B aligned");
  }
  return 0;
}

using decode_launch_t = int (*)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N,
                                int K, const void* sa, const void* sb, int mode);

template <int KIND, int NF, int W, int F, bool NT, bool MASKED>
int decode_launch_as(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                     const void* sa, const void* sb, int mode) {
  const dim3 grid(N / (NF * 16)), block(W * 64);
  uint16_t* c = static_cast<uint16_t*>(C);
  if constexpr (KIND == GSX_DECODE_BF16) {
    hipLaunchKernelGGL((decode_kernel<Bf16, NF, W, F, NT, MASKED, NoGroup>), grid, block, 0, s,
                       static_cast<const uint16_t*>(A), static_cast<const uint16_t*>(B), c, M, N, K, NoGroup{});
  } else if constexpr (KIND == GSX_DECODE_FP8) {
    const bool scaled = mode != GSX_GEMM_SCALE_NONE;  // the kernel gets (nullptr, nullptr, 0) for no scales
    hipLaunchKernelGGL((decode_kernel<Fp8K128, NF, W, F, NT, MASKED, NoGroup, const float*, const float*, int>), grid,
                       block, 0, s, static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(B), c, M, N, K,
                       NoGroup{}, scaled ? static_cast<const float*>(sa) : nullptr,
                       scaled ? static_cast<const float*>(sb) : nullptr, mode == GSX_GEMM_SCALE_ROW ? 1 : 0);
  } else {
    hipLaunchKernelGGL((decode_kernel<Mxfp4, NF, W, F, NT, MASKED, NoGroup, const uint8_t*, const uint8_t*>), grid,
                       block, 0, s, static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(B), c, M, N, K,
                       NoGroup{}, static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb));
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

// A buffer's range and a lane's offset into it are 32-bit: the buffer form needs 16 rows of A below 4 GiB.  With a
// longer K (2^27 and more in bf16, 2^28 in fp8, 2^29 in mxfp4) every configuration runs as "16/8w-f4-masked", whose
// strips of 16 columns take every N the others take.
template <int KIND, int NF, int W, int F, bool NT, bool MASKED>
int decode_launch(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                  const void* sa, const void* sb, int mode) {
  constexpr int UNIT_BITS = KIND == GSX_DECODE_BF16 ? 16 : KIND == GSX_DECODE_FP8 ? 8 : 4;
  const bool wide = 16ull * (static_cast<uint64_t>(K) * UNIT_BITS / 8) > UINT32_MAX;
  if (MASKED || wide) return decode_launch_as<KIND, 1, 8, 4, false, true>(who, s, A, B, C, M, N, K, sa, sb, mode);
  return decode_launch_as<KIND, NF, W, F, NT, false>(who, s, A, B, C, M, N, K, sa, sb, mode);
}

struct DecodeCfg {
  const char* name;
  int bn, waves, inflight;
  decode_launch_t launch[kDecodeKinds];  // indexed by GSX_DECODE_*
};
template <int NF, int W, int F, bool NT = false, bool MASKED = false>
constexpr DecodeCfg decode_cfg(const char* name) {
  return {name, NF * 16, W, F,
          {&decode_launch<GSX_DECODE_BF16, NF, W, F, NT, MASKED>, &decode_launch<GSX_DECODE_FP8, NF, W, F, NT, MASKED>,
           &decode_launch<GSX_DECODE_MXFP4, NF, W, F, NT, MASKED>}};
}

// name: columns of a strip / waves per workgroup - K-tiles in flight per wave
constexpr DecodeCfg kDecodeCfgs[] = {
    decode_cfg<1, 4, 4>("16/4w-f4"),
    decode_cfg<1, 8, 4>("16/8w-f4"),
    decode_cfg<1, 8, 8>("16/8w-f8"),
    decode_cfg<1, 16, 4>("16/16w-f4"),
    decode_cfg<2, 8, 4>("32/8w-f4"),
    decode_cfg<1, 8, 4, true>("16/8w-f4-nt"),  // ablation: non-temporal loads of B
    decode_cfg<1, 8, 4, false, true>("16/8w-f4-masked"),  // ablation: A through plain loads under `if (row < M)`
};
constexpr int kNumDecodeCfgs = sizeof(kDecodeCfgs) / sizeof(kDecodeCfgs[0]);

static const DecodeCfg* decode_row(int cfg) {
  return cfg >= 0 && cfg < kNumDecodeCfgs ? &kDecodeCfgs[cfg] : nullptr;
}

// The dispatch rule, by N and K alone (a stream's CU mask is not known here, and M is left out on purpose: one rule
// per weight matrix).  With nk the K-tiles of 128 B in a row of B:
//   nk >= 224 and N % 32 == 0   "32/8w-f4": rows so long that 256 or more workgroups of 8 waves stream for long
//                               enough each, and A is fetched once for 32 columns instead of 16
//   otherwise, strips of 16     as many waves as leave each about 2 F = 8 K-tiles, so that every wave runs the steady
//                               loop: 16 waves from nk = 128, 8 from nk = 64, 4 below
// The starting point was the decomposition rule for streaming kernels, 8 or more waves on each of the 256 CUs.  At
// the shapes measured every configuration has that many (N / 16 >= 512 strips of 4 or more waves), and what tells
// them apart is the K-tiles a wave gets.  Measured on one MI355X on a ring of more than 2 GiB, TB/s of weight bytes
// at M = 1 / 4 / 16, N x K (profiles/gemm_decode/README.md has every configuration, torch and the read yardstick):
//                          nk  16/16w-f4           16/8w-f4            16/4w-f4            32/8w-f4
//   bf16  8192 x 8192    128  5.22 / 5.09 / 4.06  5.00 / 4.97 / 4.08  4.74 / 4.75 / 3.97  3.88 / 3.86 / 3.97
//   fp8   8192 x 8192     64  4.76 / 4.61 / 3.68  4.88 / 4.88 / 3.91  4.64 / 4.70 / 3.91  4.16 / 4.09 / 3.98
//   mxfp4 28672 x 8192    32  3.48 / 3.04 / 2.50  4.34 / 3.83 / 3.13  4.35 / 3.91 / 3.02  3.89 / 3.65 / 3.16
//   bf16  8192 x 28672   448  5.80 / 5.57 / 3.92  5.76 / 5.57 / 3.91  5.71 / 5.50 / 3.71  5.66 / 5.62 / 5.18
//   fp8   8192 x 28672   224  5.32 / 5.13 / 4.12  5.38 / 5.30 / 4.26  5.26 / 5.18 / 4.24  5.19 / 5.16 / 5.02
// The rule is not the best row everywhere: at M = 16 "32/8w-f4" is ahead by 1 to 16 % at the shorter K too, and for
// mxfp4 at 8192 x 28672 (nk 112) the rule's 8 waves are 2 to 19 % behind "32/8w-f4".
static int decode_pick(int N, int nk) {
  if (nk >= 224 && N % 32 == 0) return 4;
  return nk >= 128 ? 3 : nk >= 64 ? 1 : 0;
}

// ---------------------------------------------------------------------------
// The grouped form (gsx_moe_gemm_nt): host side
// ---------------------------------------------------------------------------

struct MoeGemmArgs {
  int kind;
  const void* A;
  int a_div;
  const void* B;
  void* C;
  const int32_t* plan;
  int M, topk, E, N, K;
  const void* sa;
  const void* sb;
  int mode;
};

static uint64_t moe_row_bytes(int kind, int K) {
  return static_cast<uint64_t>(K) * (kind == GSX_DECODE_BF16 ? 16 : kind == GSX_DECODE_FP8 ? 8 : 4) / 8;
}

// Everything gsx_moe_gemm_nt and its _launch_cfg refuse, before the first device call.  `bn`: the columns of a strip.
static int moe_gemm_validate(const char* who, int bn, const MoeGemmArgs& a) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind < 0 || a.kind >= kDecodeKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (a.M < 1 || a.M > 16) return refuse("need 1 <= M <= 16");
  if (a.E < 1) return refuse("need E >= 1");
  if (a.topk < 1 || a.topk > 8 || a.topk > a.E) return refuse("need 1 <= topk <= min(8, E)");
  if (a.a_div < 1) return refuse("need a_div >= 1");
  if (a.N <= 0 || a.N % bn || a.K <= 0 || a.K % kDecodeKTile[a.kind]) {
    std::snprintf(msg, sizeof(msg), "%s: need N%%%d==0, K%%%d==0", who, bn, kDecodeKTile[a.kind]);
    return fail_arg(msg);
  }
  if (!a.A || !a.B || !a.C || !a.plan) return refuse("A, B, C and plan must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.B) | reinterpret_cast<uintptr_t>(a.C)) % 16)
    return refuse("operands must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(a.plan) % 4) return refuse("plan must be 4-B aligned");
  const uintptr_t sbits = reinterpret_cast<uintptr_t>(a.sa) | reinterpret_cast<uintptr_t>(a.sb);
  if (a.kind == GSX_DECODE_BF16) {
    if (a.sa || a.sb || a.mode != GSX_GEMM_SCALE_NONE)
      return refuse("bf16 takes no scales: scale_a and scale_b must be NULL and scale_mode NONE");
  } else if (a.kind == GSX_DECODE_FP8) {
    if (a.mode != GSX_GEMM_SCALE_NONE && a.mode != GSX_GEMM_SCALE_ROW)
      return refuse("fp8 takes scale_mode NONE or ROW");
    if (a.mode == GSX_GEMM_SCALE_ROW) {
      if (!a.sa || !a.sb) return refuse("scale_a and scale_b must not be NULL in this scale_mode");
      if (sbits % 4) return refuse("scale_a and scale_b must be 4-B aligned");
    }
  } else {
    if (a.mode != GSX_GEMM_SCALE_NONE) return refuse("mxfp4 takes scale_mode NONE: its scales are the e8m0 blocks");
    if (!a.sa || !a.sb) return refuse("scale_a and scale_b must not be NULL");
    if (sbits % 16) return refuse("scale_a and scale_b must be 16-B aligned");
  }
  // A lane without a row reads at the end of the buffer over A, plus its place in the row: one row more than A has
  // must fit the 32-bit range too.  scale_a's rows are 1 / 16 of A's.
  const uint64_t P = static_cast<uint64_t>(a.M) * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const uint64_t row = moe_row_bytes(a.kind, a.K);
  if ((a_rows + 1) * row > UINT32_MAX) return refuse("A (and one row more) must fit a 32-bit buffer range");
  struct Span {
    const void* p;
    uint64_t bytes;
  };
  const bool scaled = a.kind == GSX_DECODE_MXFP4 || a.mode == GSX_GEMM_SCALE_ROW;
  const uint64_t en = static_cast<uint64_t>(a.E) * a.N, blocks = a.K / 32;
  const Span c{a.C, P * a.N * 2};
  const Span in[] = {{a.A, a_rows * row},
                     {a.B, en * row},
                     {a.plan, GSX_MOE_PLAN_INTS * 4ull},
                     {scaled ? a.sa : nullptr, a.kind == GSX_DECODE_MXFP4 ? a_rows * blocks : a_rows * 4},
                     {scaled ? a.sb : nullptr, a.kind == GSX_DECODE_MXFP4 ? en * blocks : en * 4}};
  for (const Span& s : in) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(c.p), y = reinterpret_cast<uintptr_t>(s.p);
    if (s.p && x < y + s.bytes && y < x + c.bytes) return refuse("C must not overlap A, B, plan, scale_a or scale_b");
  }
  return 0;
}

using moe_launch_t = int (*)(const char* who, hipStream_t s, const MoeGemmArgs& a);

template <int KIND, int NF, int W, int F>
int moe_launch(const char* who, hipStream_t s, const MoeGemmArgs& a) {
  const int P = a.M * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const dim3 grid(a.N / (NF * 16), a.E < P ? a.E : P), block(W * 64);
  uint16_t* c = static_cast<uint16_t*>(a.C);
  const MoePlan gp{a.plan, P, a.E, a.a_div, a_rows};
  if constexpr (KIND == GSX_DECODE_BF16) {
    hipLaunchKernelGGL((decode_kernel<Bf16, NF, W, F, false, false, MoePlan>), grid, block, 0, s,
                       static_cast<const uint16_t*>(a.A), static_cast<const uint16_t*>(a.B), c, 0, a.N, a.K, gp);
  } else if constexpr (KIND == GSX_DECODE_FP8) {
    const bool scaled = a.mode != GSX_GEMM_SCALE_NONE;  // the kernel gets (nullptr, nullptr, 0) for no scales
    hipLaunchKernelGGL((decode_kernel<Fp8K128, NF, W, F, false, false, MoePlan, const float*, const float*, int>),
                       grid, block, 0, s, static_cast<const uint8_t*>(a.A), static_cast<const uint8_t*>(a.B), c, 0,
                       a.N, a.K, gp, scaled ? static_cast<const float*>(a.sa) : nullptr,
                       scaled ? static_cast<const float*>(a.sb) : nullptr, scaled ? 1 : 0);
  } else {
    hipLaunchKernelGGL((decode_kernel<Mxfp4, NF, W, F, false, false, MoePlan, const uint8_t*, const uint8_t*>),
                       grid, block, 0, s, static_cast<const uint8_t*>(a.A), static_cast<const uint8_t*>(a.B), c, 0,
                       a.N, a.K, gp, static_cast<const uint8_t*>(a.sa), static_cast<const uint8_t*>(a.sb));
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct MoeCfg {
  int decode;  // the row of kDecodeCfgs it equals: same NF, W and F, and so the same summation order
  moe_launch_t launch[kDecodeKinds];
};
template <int NF, int W, int F>
constexpr MoeCfg moe_cfg(int decode) {
  return {decode,
          {&moe_launch<GSX_DECODE_BF16, NF, W, F>, &moe_launch<GSX_DECODE_FP8, NF, W, F>,
           &moe_launch<GSX_DECODE_MXFP4, NF, W, F>}};
}
// the four shapes decode_pick() dispatches to, under their names in kDecodeCfgs
constexpr MoeCfg kMoeCfgs[] = {moe_cfg<1, 4, 4>(0), moe_cfg<1, 8, 4>(1), moe_cfg<1, 16, 4>(3), moe_cfg<2, 8, 4>(4)};
constexpr int kNumMoeCfgs = sizeof(kMoeCfgs) / sizeof(kMoeCfgs[0]);

static const MoeCfg* moe_row(int cfg) { return cfg >= 0 && cfg < kNumMoeCfgs ? &kMoeCfgs[cfg] : nullptr; }

// decode_pick()'s rule, as a row of kMoeCfgs.  It was measured on dense 8192-wide matrices; what it does on expert
// shapes is in profiles/moe/README.md.
static const MoeCfg& moe_pick(int N, int nk) {
  const int d = decode_pick(N, nk);
  for (const MoeCfg& c : kMoeCfgs)
    if (c.decode == d) return c;
  return kMoeCfgs[0];
}

static int moe_gemm_run(const char* who, void* stream, const MoeGemmArgs& a) {
  return moe_pick(a.N, a.K / kDecodeKTile[a.kind]).launch[a.kind](who, S(stream), a);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_decode_gemm_cfg_name(int cfg) { return decode_row(cfg) ? decode_row(cfg)->name : nullptr; }

int gsx_decode_gemm_cfg_shape(int cfg, int* bn, int* waves, int* inflight) {
  const DecodeCfg* c = decode_row(cfg);
  if (!c) return -1;
  *bn = c->bn;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_decode_gemm_nt_launch_cfg(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                                  const void* scale_a, const void* scale_b, int scale_mode, int cfg) {
  const char* who = "gsx_decode_gemm_nt_launch_cfg";
  const DecodeCfg* c = decode_row(cfg);
  if (!c) return fail_arg("gsx_decode_gemm_nt_launch_cfg: unknown config");
  if (int rc = decode_validate(who, kind, c->bn, A, B, C, M, N, K, scale_a, scale_b, scale_mode)) return rc;
  return c->launch[kind](who, S(stream), A, B, C, M, N, K, scale_a, scale_b, scale_mode);
}

int gsx_decode_gemm_nt(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                       const void* scale_a, const void* scale_b, int scale_mode) {
  const char* who = "gsx_decode_gemm_nt";
  if (int rc = decode_validate(who, kind, 16, A, B, C, M, N, K, scale_a, scale_b, scale_mode)) return rc;
  const DecodeCfg& c = kDecodeCfgs[decode_pick(N, K / kDecodeKTile[kind])];
  return c.launch[kind](who, S(stream), A, B, C, M, N, K, scale_a, scale_b, scale_mode);
}

int gsx_event_time_decode_gemm(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                               const void* scale_a, const void* scale_b, int scale_mode, int iters, float* ms) {
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = decode_validate("gsx_decode_gemm_nt", kind, 16, A, B, C, M, N, K, scale_a, scale_b, scale_mode))
    return rc;
  return event_time(stream, iters, ms, [&] {
    return gsx_decode_gemm_nt(stream, kind, A, B, C, M, N, K, scale_a, scale_b, scale_mode);
  });
}

const char* gsx_moe_gemm_cfg_name(int cfg) { return moe_row(cfg) ? kDecodeCfgs[moe_row(cfg)->decode].name : nullptr; }

int gsx_moe_gemm_cfg_shape(int cfg, int* bn, int* waves, int* inflight, int* decode_cfg) {
  const MoeCfg* c = moe_row(cfg);
  if (!c) return -1;
  *decode_cfg = c->decode;
  return gsx_decode_gemm_cfg_shape(c->decode, bn, waves, inflight);
}

int gsx_moe_gemm_nt_launch_cfg(void* stream, int kind, const void* A, int a_div, const void* B, void* C,
                               const int32_t* plan, int M, int topk, int E, int N, int K, const void* scale_a,
                               const void* scale_b, int scale_mode, int cfg) {
  const char* who = "gsx_moe_gemm_nt_launch_cfg";
  const MoeCfg* c = moe_row(cfg);
  if (!c) return fail_arg("gsx_moe_gemm_nt_launch_cfg: unknown config");
  const MoeGemmArgs a{kind, A, a_div, B, C, plan, M, topk, E, N, K, scale_a, scale_b, scale_mode};
  if (int rc = moe_gemm_validate(who, kDecodeCfgs[c->decode].bn, a)) return rc;
  return c->launch[kind](who, S(stream), a);
}

int gsx_moe_gemm_nt(void* stream, int kind, const void* A, int a_div, const void* B, void* C, const int32_t* plan,
                    int M, int topk, int E, int N, int K, const void* scale_a, const void* scale_b, int scale_mode) {
  const MoeGemmArgs a{kind, A, a_div, B, C, plan, M, topk, E, N, K, scale_a, scale_b, scale_mode};
  if (int rc = moe_gemm_validate("gsx_moe_gemm_nt", 16, a)) return rc;
  return moe_gemm_run("gsx_moe_gemm_nt", stream, a);
}

int gsx_event_time_moe_gemm(void* stream, int kind, const void* A, int a_div, const void* B, void* C,
                            const int32_t* plan, int M, int topk, int E, int N, int K, const void* scale_a,
                            const void* scale_b, int scale_mode, int iters, float* ms) {
  const MoeGemmArgs a{kind, A, a_div, B, C, plan, M, topk, E, N, K, scale_a, scale_b, scale_mode};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = moe_gemm_validate("gsx_moe_gemm_nt", 16, a)) return rc;
  return event_time(stream, iters, ms, [&] { return moe_gemm_run("gsx_moe_gemm_nt", stream, a); });
}

}  // extern "C"
