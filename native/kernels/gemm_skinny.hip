// Skinny GEMM for the pod workload: C[M][N] (bf16) = A[M][K] * B[N][K]^T with 1 <= M <= 128, the shape of a server that
// decodes up to 128 sequences at once.  It fills the hole between the decode GEMM (gemm_decode.hip, M <= 16) and the
// large GEMMs (M % 128 == 0): the weights are still read from HBM exactly once, but with up to eight row fragments A
// is no longer negligible, and a workgroup has more accumulators than a strip of 16 columns can pay for.  Operands,
// scale modes and epilogue are those of gsx_decode_gemm_nt for GSX_DECODE_BF16 and GSX_DECODE_FP8, the MFMAs
// gemm_tile.h's operand kinds Bf16 and Fp8K128 with its fragment convention: lane (fr, fq) holds chunks fq and 4 + fq
// of its row of a 128-B K-tile row.  C ABI in gsx_kernels.h.
//
// Two kernels.  skinny_kernel:
//   * a workgroup is (strip, split): a strip of BN = 16 NF columns of C and all MF = ceil(M / 16) row fragments, over
//     one of `splits` runs of consecutive K-tiles (run s: tiles s per .. s per + per - 1, per = ceil(nk / splits)).
//     The grid is (N / BN, splits): wide strips alone are too few workgroups for 256 CUs (N / 64 = 128 at N = 8192),
//     the split of K makes up for it;
//   * its W waves split the run's K-tiles, interleaved: wave w takes tiles w, w + W, ... of the run.  Every wave holds
//     the whole MF x NF block of accumulators, so a fragment of B it has loaded meets all rows and a fragment of A all
//     the strip's columns: a byte that reaches a wave's registers is used MF or NF times and no operand passes through
//     LDS;
//   * B ONCE: B goes from global memory to VGPRs in fragment shape, two 16-B loads per lane, fragment and K-tile, as in
//     decode_kernel; a wave keeps F K-tiles (of A and of B) in flight in a register ring behind counted waits.  Each
//     byte of B is loaded by exactly one wave of one workgroup;
//   * A'S TRAFFIC: the workgroups of a strip fetch A's M x K once between them (each its run of K), from L2: M / BN
//     times the bytes of B.  The dispatch rule takes BN = 32 only up to M = 64 and BN = 64 otherwise, so A is at most
//     2x B's bytes, which it reaches at M = 128.  The waves of a workgroup read disjoint K-tiles of A, so there is nothing for
//     them to share through LDS;
//   * ROWS PAST M: MF is a template parameter, chosen at launch: M = 32 runs the kernel with two row fragments of
//     accumulators and MFMAs.  A comes through bounds-checked buffer loads whose range is exactly the M rows (the trick
//     decode_kernel documents): the row's offset is in the lane's offset, which is the one that is checked, so a lane
//     of the ragged last fragment whose row is >= M gets zeros in registers and makes no access; there is no branch
//     around a load.  scale_a is read, and C and the partials are written, under `row < M`;
//   * the waves' fp32 accumulators meet in LDS one after the other: wave 0 writes its block, wave 1 adds its own to it,
//     and so on (W - 1 barriers; one block of MF NF KiB instead of W); the last wave holds the sum.  With splits == 1
//     it applies the scales, (acc * sa) * sb, converts once (f2bf) and stores C; otherwise it stores its fp32 block to
//     the workspace, part[split][row][col] over exactly M rows.  A split without a K-tile stores zeros.
// skinny_reduce_kernel (splits > 1 only, the next launch on the same stream): adds the partials of an element in the
// order of the split index, applies the same epilogue and stores C.  No atomics, and no workgroup waits for another.
//
// DETERMINISM: fp32 accumulation with one rounding to bf16, in a fixed order: a wave's K-tiles in order, the waves by
// index, the splits by index.  A row's accumulators never meet another row's, and neither MF nor the ragged fragment
// changes what is added to them, so row i of C has the same bits at every M that contains it, given the configuration
// and `splits`.  The order is not that of gsx_decode_gemm_nt or gsx_gemm_*_nt.
//
// REGISTERS: the block of accumulators is 4 MF NF registers (128 at MF = 8, NF = 4) and a slot of the ring 8 (MF + NF).
// All configurations have 4 waves, one per SIMD, so a wave may use all 512 registers of a lane (VGPRs and AGPRs).
// The counts of every instantiation are in profiles/gemm_skinny/README.md: none uses scratch.
//
// Row offsets into B, scale_b, C and the workspace are 64-bit (B may exceed 4 GiB); the offset inside a row is an int.
// A buffer's range and a lane's offset into it are 32-bit: 16 MF rows of A have to stay below 4 GiB, which is refused
// otherwise.
//
// The configurations vary BN and F; the dispatch rule and what is known about it are at skinny_pick() below and in
// profiles/gemm_skinny/README.md.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int kSkinnyMaxM = 128, kSkinnyMaxMF = kSkinnyMaxM / 16, kSkinnyMaxSplits = 16;

// c = (acc * sa[row]) * sb[col], as Scaled (gemm_tile.h) does it; sa == nullptr leaves the accumulator alone
__device__ __forceinline__ float skinny_scaled(float v, const float* sa, const float* sb, int stride, size_t row,
                                               size_t col) {
  return sa == nullptr ? v : (v * sa[row * stride]) * sb[col * stride];
}

// `part` is the workspace, or nullptr with a grid of one split; `per` the K-tiles of a split's run.
template <class OP, int MF, int NF, int W, int F>
__global__ __launch_bounds__(W * 64) void skinny_kernel(const typename OP::elem* __restrict__ A,
                                                       const typename OP::elem* __restrict__ B,
                                                       uint16_t* __restrict__ C, float* __restrict__ part, int M,
                                                       int N, int K, int per, const float* __restrict__ sa,
                                                       const float* __restrict__ sb, int stride) {
  using T = typename OP::elem;
  using frag = typename OP::frag;
  static_assert(!OP::MX && OP::EPU == 1, "bf16 and fp8 only");
  constexpr int CH = OP::CH;
  constexpr int BKU = OP::BK;                              // a K-tile in units of T: 128 B
  constexpr int CU = CHUNK / static_cast<int>(sizeof(T));  // a chunk in units of T
  const int ld = K, nk = K / OP::BK;
  __shared__ f32x4 red[MF * NF][64];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const size_t col0 = static_cast<size_t>(blockIdx.x) * (NF * 16);
  const int split = blockIdx.y;
  const int first = split * per;  // the run's first K-tile; splits * per < nk + 16, no overflow
  const int run = nk - first < per ? (nk - first > 0 ? nk - first : 0) : per;
  const int mine = wid < run ? (run - wid + W - 1) / W : 0;  // K-tiles first + wid, first + wid + W, ...

  // A's rows as byte offsets into the buffer of exactly M rows: past its end for a row >= M
  const uint32_t arow_bytes = static_cast<uint32_t>(ld) * sizeof(T);
  const __amdgpu_buffer_rsrc_t abuf = rows_buffer(A, static_cast<uint32_t>(M) * arow_bytes);
  const uint32_t aoff = static_cast<uint32_t>(fr) * arow_bytes + fq * CHUNK;
  const T* bp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) bp[f] = B + (col0 + f * 16 + fr) * ld + fq * CU;

  // the ring: slot i holds one K-tile's fragments of A and of B
  frag ra[F][MF][2], rb[F][NF][2];

  auto load = [&](auto slot, int j) {
    constexpr int i = decltype(slot)::value;
    const int kt = first + wid + j * W;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int c = 0; c < 2; ++c) rb[i][f][c] = load_chunk<frag, false>(bp[f] + kt * BKU + c * 4 * CU);
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        ra[i][m][c] = __builtin_bit_cast(
            frag, __builtin_amdgcn_raw_buffer_load_b128(
                      abuf, static_cast<int>(aoff + m * 16 * arow_bytes + c * 4 * CHUNK), kt * ROW_BYTES, 0));
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[m][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mma = [&](auto slot) {
    constexpr int i = decltype(slot)::value;
#pragma unroll
    for (int kk = 0; kk < 2 / CH; ++kk)
#pragma unroll
      for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) OP::mma(acc[m][f], &ra[i][m][kk * CH], &rb[i][f][kk * CH]);
  };

  // decode_kernel's loop: slot i holds tile t + i until its MFMAs, then tile t + i + F.  The steady loop has no
  // condition inside and is entered behind an unconditional prologue, so that on every path to its top the F tiles
  // were issued in slot order and the wait for slot 0 leaves the F - 1 younger tiles in flight; the last 2 F - 1
  // tiles or fewer drain in two conditional passes.
  int t = 0;
  if (mine >= 2 * F) {
    static_for<F>([&](auto i) {
      load(i, i);
      __builtin_amdgcn_sched_barrier(0);
    });
    do {
      static_for<F>([&](auto i) {
        mma(i);
        load(i, t + i + F);
        __builtin_amdgcn_sched_barrier(0);  // slot by slot: the waits are counted from this order
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

  // The waves' blocks meet in the order of the wave index: after barrier w, red holds the sum of waves 0 .. w.  A wave
  // without a tile contributes its zeros.  Every wave reaches every barrier.
  for (int w = 0; w + 1 < W; ++w) {
    if (wid == w) {
#pragma unroll
      for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          if (w > 0) {
            const f32x4 v = red[m * NF + f][lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][f][j] = v[j] + acc[m][f][j];
          }
          red[m * NF + f][lane] = acc[m][f];
        }
    }
    __syncthreads();
  }
  if (wid != W - 1) return;
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      f32x4 s = acc[m][f];
      if constexpr (W > 1) {
        const f32x4 v = red[m * NF + f][lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = v[j] + s[j];
      }
      // 16x16 C map: column fr, row 4 fq + j
      const size_t col = col0 + f * 16 + fr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = m * 16 + fq * 4 + j;
        if (row >= M) continue;
        if (part != nullptr)
          part[(static_cast<size_t>(split) * M + row) * N + col] = s[j];
        else
          C[static_cast<size_t>(row) * N + col] = f2bf(skinny_scaled(s[j], sa, sb, stride, row, col));
      }
    }
}

// One thread per four columns of a row: part[0] + part[1] + ... in this order, the epilogue, one rounding.
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* __restrict__ part, uint16_t* __restrict__ C,
                                                            int M, int N, int splits, const float* __restrict__ sa,
                                                            const float* __restrict__ sb, int stride) {
  const size_t quads = static_cast<size_t>(N / 4);
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= quads * M) return;
  const size_t row = t / quads, col = (t % quads) * 4;
  const size_t plane = static_cast<size_t>(M) * N, at = row * N + col;
  f32x4 s = *reinterpret_cast<const f32x4*>(part + at);
  for (int i = 1; i < splits; ++i) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + i * plane + at);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j];
  }
  uint16_t out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = f2bf(skinny_scaled(s[j], sa, sb, stride, row, col + j));
  *reinterpret_cast<uint2*>(C + at) = uint2{out[0] | static_cast<uint32_t>(out[1]) << 16,
                                            out[2] | static_cast<uint32_t>(out[3]) << 16};
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

constexpr int kSkinnyKinds = 2;
constexpr int kSkinnyKTile[kSkinnyKinds] = {Bf16::BK, Fp8K128::BK};  // indexed by GSX_DECODE_*

struct SkinnyArgs {
  int kind;
  const void* A;
  const void* B;
  void* C;
  int M, N, K;
  const void* sa;
  const void* sb;
  int mode;
  void* ws;
  uint64_t ws_bytes;
};

static uint64_t skinny_workspace(int M, int N, int splits) {
  return splits > 1 ? static_cast<uint64_t>(splits) * M * N * sizeof(float) : 0;
}

// Everything the entry points refuse but the workspace, before the first device call.  `bn`: the columns of a strip.
static int skinny_validate(const char* who, int bn, const SkinnyArgs& a) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind == GSX_DECODE_MXFP4) return refuse("mxfp4 is not supported by the skinny GEMM");
  if (a.kind < 0 || a.kind >= kSkinnyKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (a.M < 1 || a.M > kSkinnyMaxM) return refuse("need 1 <= M <= 128");
  const int step = bn > 64 ? bn : 64;  // N % 64 == 0 for every entry point, and the strip's columns
  if (a.N <= 0 || a.N % step || a.N % bn || a.K <= 0 || a.K % kSkinnyKTile[a.kind]) {
    std::snprintf(msg, sizeof(msg), "%s: need N%%%d==0, K%%%d==0", who, step, kSkinnyKTile[a.kind]);
    return fail_arg(msg);
  }
  if (!a.A || !a.B || !a.C) return refuse("A, B and C must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.B) | reinterpret_cast<uintptr_t>(a.C) |
       reinterpret_cast<uintptr_t>(a.ws)) % 16)
    return refuse("operands and workspace must be 16-B aligned");
  const uintptr_t sbits = reinterpret_cast<uintptr_t>(a.sa) | reinterpret_cast<uintptr_t>(a.sb);
  if (a.kind == GSX_DECODE_BF16) {
    if (a.sa || a.sb || a.mode != GSX_GEMM_SCALE_NONE)
      return refuse("bf16 takes no scales: scale_a and scale_b must be NULL and scale_mode NONE");
  } else {
    if (a.mode != GSX_GEMM_SCALE_NONE && a.mode != GSX_GEMM_SCALE_TENSOR && a.mode != GSX_GEMM_SCALE_ROW) {
      std::snprintf(msg, sizeof(msg), "%s: unknown scale_mode %d", who, a.mode);
      return fail_arg(msg);
    }
    if (a.mode != GSX_GEMM_SCALE_NONE) {
      if (!a.sa || !a.sb) return refuse("scale_a and scale_b must not be NULL in this scale_mode");
      if (sbits % 4) return refuse("scale_a and scale_b must be 4-B aligned");
    }
  }
  // a lane's offset into the buffer over A's rows is 32-bit, the rows of the ragged fragment included
  const uint64_t row = static_cast<uint64_t>(a.K) * (a.kind == GSX_DECODE_BF16 ? 2 : 1);
  if ((a.M + 15) / 16 * 16 * row > UINT32_MAX)
    return refuse("K too large: the row fragments of A must fit a 32-bit buffer range");
  return 0;
}

// What depends on `splits`: its range, the workspace, and that C overlaps nothing, the workspace included.
static int skinny_validate_splits(const char* who, const SkinnyArgs& a, int splits) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (splits < 1 || splits > kSkinnyMaxSplits) return refuse("need 1 <= splits <= 16");
  const uint64_t need = skinny_workspace(a.M, a.N, splits);
  if (need && (!a.ws || a.ws_bytes < need)) {
    std::snprintf(msg, sizeof(msg), "%s: workspace too small: splits %d needs %llu bytes", who, splits,
                  static_cast<unsigned long long>(need));
    return fail_arg(msg);
  }
  struct Span {
    const void* p;
    uint64_t bytes;
  };
  const uint64_t row = static_cast<uint64_t>(a.K) * (a.kind == GSX_DECODE_BF16 ? 2 : 1);
  const bool scaled = a.mode != GSX_GEMM_SCALE_NONE, rows = a.mode == GSX_GEMM_SCALE_ROW;
  const Span c{a.C, static_cast<uint64_t>(a.M) * a.N * 2};
  const Span in[] = {{a.A, a.M * row},
                     {a.B, a.N * row},
                     {scaled ? a.sa : nullptr, rows ? a.M * 4ull : 4ull},
                     {scaled ? a.sb : nullptr, rows ? a.N * 4ull : 4ull},
                     {need ? a.ws : nullptr, need}};
  for (const Span& s : in) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(c.p), y = reinterpret_cast<uintptr_t>(s.p);
    if (s.p && x < y + s.bytes && y < x + c.bytes)
      return refuse("C must not overlap A, B, scale_a, scale_b or the workspace");
  }
  return 0;
}

using skinny_launch_t = int (*)(const char* who, hipStream_t s, const SkinnyArgs& a, int splits);

template <int KIND, int MF, int NF, int W, int F>
int skinny_launch(const char* who, hipStream_t s, const SkinnyArgs& a, int splits) {
  using OP = std::conditional_t<KIND == GSX_DECODE_BF16, Bf16, Fp8K128>;
  using T = typename OP::elem;
  const int nk = a.K / OP::BK, per = (nk + splits - 1) / splits;
  const bool scaled = a.mode != GSX_GEMM_SCALE_NONE;  // the kernels get (nullptr, nullptr, 0) for no scales
  const float* sa = scaled ? static_cast<const float*>(a.sa) : nullptr;
  const float* sb = scaled ? static_cast<const float*>(a.sb) : nullptr;
  const int stride = a.mode == GSX_GEMM_SCALE_ROW ? 1 : 0;
  uint16_t* c = static_cast<uint16_t*>(a.C);
  float* part = splits > 1 ? static_cast<float*>(a.ws) : nullptr;
  hipLaunchKernelGGL((skinny_kernel<OP, MF, NF, W, F>), dim3(a.N / (NF * 16), splits), dim3(W * 64), 0, s,
                     static_cast<const T*>(a.A), static_cast<const T*>(a.B), c, part, a.M, a.N, a.K, per, sa, sb,
                     stride);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, who);
  if (splits > 1) {
    const uint64_t quads = static_cast<uint64_t>(a.M) * (a.N / 4);
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3(static_cast<uint32_t>((quads + 255) / 256)), dim3(256), 0, s, part, c,
                       a.M, a.N, splits, sa, sb, stride);
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : fail(e, who);
}

struct SkinnyCfg {
  const char* name;
  int bn, waves, inflight;
  skinny_launch_t launch[kSkinnyKinds][kSkinnyMaxMF];  // indexed by GSX_DECODE_* and MF - 1
};
template <int NF, int W, int F, int... MF>
constexpr SkinnyCfg skinny_cfg(const char* name, std::integer_sequence<int, MF...>) {
  return {name, NF * 16, W, F,
          {{&skinny_launch<GSX_DECODE_BF16, MF + 1, NF, W, F>...}, {&skinny_launch<GSX_DECODE_FP8, MF + 1, NF, W, F>...}}};
}
template <int NF, int W, int F>
constexpr SkinnyCfg skinny_cfg(const char* name) {
  return skinny_cfg<NF, W, F>(name, std::make_integer_sequence<int, kSkinnyMaxMF>{});
}

// name: columns of a strip / waves per workgroup - K-tiles in flight per wave
constexpr SkinnyCfg kSkinnyCfgs[] = {
    skinny_cfg<2, 4, 2>("32/4w-f2"),
    skinny_cfg<4, 4, 2>("64/4w-f2"),
    skinny_cfg<4, 4, 3>("64/4w-f3"),
};
constexpr int kNumSkinnyCfgs = sizeof(kSkinnyCfgs) / sizeof(kSkinnyCfgs[0]);

static const SkinnyCfg* skinny_row(int cfg) {
  return cfg >= 0 && cfg < kNumSkinnyCfgs ? &kSkinnyCfgs[cfg] : nullptr;
}

// The dispatch rule, by MF = ceil(M / 16), N and the K-tiles nk of a row of B:
//   configuration   "64/4w-f2", except "32/4w-f2" where M <= 64 and N < 8192.  The wide strip fetches A half as often
//                   and is ahead wherever it still gives 128 strips; below that the narrow strip's workgroups count
//                   for more.  Above M = 64 the narrow strip would pull more than twice B's bytes of A from L2 (M / BN
//                   > 2) and is not dispatched, although it measured faster at N = 1024 (below).
//   splits          as many as give 256 workgroups of the wide strip (one per CU: its accumulators leave room for one
//                   at MF >= 5) or 512 of the narrow one (8 waves per CU), but no more than leave every wave 2 F = 4
//                   K-tiles, so that it runs the steady loop, and at most 16.  It does not depend on M or on the
//                   strip: N / 32 strips and 512 give what N / 64 strips and 256 give.
// The starting point was the decomposition rule for streaming kernels (8 or more waves per CU, each with enough K-tiles
// for a steady loop), which put the narrow strip at every M <= 64.  Measured on one MI355X on a ring of more than
// 2 GiB, TB/s of weight bytes at M = 17 / 32 / 64 / 128 with the splits of the rule (2 at N = 8192; 8 and 4 at N = 1024;
// profiles/gemm_skinny/README.md has every row, other splits and the yardsticks):
//                         nk  32/4w-f2                    64/4w-f2                    64/4w-f3
//   bf16  8192 x 8192    128  3.47 / 3.12 / 2.30 / 1.44   3.61 / 3.45 / 2.95 / 2.07   3.59 / 3.51 / 3.02 / 2.11
//   bf16  8192 x 28672   448  4.24 / 3.59 / 2.71 / 1.73   4.46 / 4.14 / 3.50 / 2.55   4.64 / 4.32 / 3.59 / 2.63
//   bf16  1024 x 8192    128  1.53 / 1.37 / 1.09 / 0.78   1.23 / 1.11 / 0.85 / 0.59   1.21 / 1.11 / 0.84 / 0.59
//   fp8   8192 x 8192     64  3.44 / 2.95 / 2.17 / 1.21   3.28 / 3.07 / 2.46 / 1.64   3.24 / 3.07 / 2.43 / 1.61
//   fp8   8192 x 28672   224  4.32 / 3.70 / 2.63 / 1.58   5.19 / 4.75 / 3.57 / 2.45   5.19 / 4.75 / 3.64 / 2.43
//   fp8   1024 x 8192     64  0.85 / 0.78 / 0.61 / 0.42   0.68 / 0.63 / 0.47 / 0.31   0.66 / 0.61 / 0.46 / 0.30
// The rule is not the best row everywhere: "64/4w-f3" is 1 to 4 % ahead of it in bf16 at N = 8192; at fp8 8192 x 8192
// and M = 17 the narrow strip is 5 % ahead; at N = 1024 and M = 128 the narrow strip is 32 to 35 % ahead; and with the
// narrow strip one split was 6 to 19 % ahead of two at N = 8192, K = 8192 and M <= 64.  The split counts of the wide
// strip at N = 8192 other than 2 are in the profile.
struct SkinnyPick {
  int cfg, splits;
};
static SkinnyPick skinny_pick(int mf, int N, int nk) {
  const int cfg = mf <= 4 && N / 64 < 128 ? 0 : 1;
  const SkinnyCfg& c = kSkinnyCfgs[cfg];
  const int strips = N / c.bn, want = cfg == 0 ? 512 : 256;
  int splits = (want + strips - 1) / strips;
  const int steady = nk / (c.waves * 2 * c.inflight);
  if (splits > steady) splits = steady;
  if (splits > kSkinnyMaxSplits) splits = kSkinnyMaxSplits;
  return {cfg, splits < 1 ? 1 : splits};
}

static int skinny_run(const char* who, void* stream, const SkinnyArgs& a) {
  const SkinnyPick p = skinny_pick((a.M + 15) / 16, a.N, a.K / kSkinnyKTile[a.kind]);
  if (int rc = skinny_validate_splits(who, a, p.splits)) return rc;
  return kSkinnyCfgs[p.cfg].launch[a.kind][(a.M + 15) / 16 - 1](who, S(stream), a, p.splits);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_skinny_gemm_cfg_name(int cfg) { return skinny_row(cfg) ? skinny_row(cfg)->name : nullptr; }

int gsx_skinny_gemm_cfg_shape(int cfg, int* bn, int* waves, int* inflight) {
  const SkinnyCfg* c = skinny_row(cfg);
  if (!c) return -1;
  *bn = c->bn;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_skinny_gemm_pick(int kind, int M, int N, int K, int* cfg, int* splits) {
  const char* who = "gsx_skinny_gemm_pick";
  if (kind == GSX_DECODE_MXFP4) return fail_arg("gsx_skinny_gemm_pick: mxfp4 is not supported by the skinny GEMM");
  if (kind < 0 || kind >= kSkinnyKinds) return fail_arg("gsx_skinny_gemm_pick: unknown kind");
  if (M < 1 || M > kSkinnyMaxM) return fail_arg("gsx_skinny_gemm_pick: need 1 <= M <= 128");
  if (N <= 0 || N % 64 || K <= 0 || K % kSkinnyKTile[kind]) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%s: need N%%64==0, K%%%d==0", who, kSkinnyKTile[kind]);
    return fail_arg(msg);
  }
  const SkinnyPick p = skinny_pick((M + 15) / 16, N, K / kSkinnyKTile[kind]);
  *cfg = p.cfg;
  *splits = p.splits;
  return 0;
}

int gsx_skinny_gemm_workspace_bytes(int M, int N, int K, uint64_t* bytes) {
  if (M < 1 || M > kSkinnyMaxM) return fail_arg("gsx_skinny_gemm_workspace_bytes: need 1 <= M <= 128");
  if (N <= 0 || N % 64 || K <= 0 || K % 64) return fail_arg("gsx_skinny_gemm_workspace_bytes: need N%64==0, K%64==0");
  uint64_t most = 0;
  for (int kind = 0; kind < kSkinnyKinds; ++kind) {
    if (K % kSkinnyKTile[kind]) continue;
    const uint64_t b = skinny_workspace(M, N, skinny_pick((M + 15) / 16, N, K / kSkinnyKTile[kind]).splits);
    most = b > most ? b : most;
  }
  *bytes = most;
  return 0;
}

int gsx_skinny_gemm_nt_launch_cfg(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                                  const void* scale_a, const void* scale_b, int scale_mode, void* workspace,
                                  uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_skinny_gemm_nt_launch_cfg";
  const SkinnyCfg* c = skinny_row(cfg);
  if (!c) return fail_arg("gsx_skinny_gemm_nt_launch_cfg: unknown config");
  const SkinnyArgs a{kind, A, B, C, M, N, K, scale_a, scale_b, scale_mode, workspace, workspace_bytes};
  if (int rc = skinny_validate(who, c->bn, a)) return rc;
  if (int rc = skinny_validate_splits(who, a, splits)) return rc;
  return c->launch[kind][(M + 15) / 16 - 1](who, S(stream), a, splits);
}

int gsx_skinny_gemm_nt(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                       const void* scale_a, const void* scale_b, int scale_mode, void* workspace,
                       uint64_t workspace_bytes) {
  const SkinnyArgs a{kind, A, B, C, M, N, K, scale_a, scale_b, scale_mode, workspace, workspace_bytes};
  if (int rc = skinny_validate("gsx_skinny_gemm_nt", 64, a)) return rc;
  return skinny_run("gsx_skinny_gemm_nt", stream, a);
}

int gsx_event_time_skinny_gemm(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                               const void* scale_a, const void* scale_b, int scale_mode, void* workspace,
                               uint64_t workspace_bytes, int iters, float* ms) {
  const SkinnyArgs a{kind, A, B, C, M, N, K, scale_a, scale_b, scale_mode, workspace, workspace_bytes};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = skinny_validate("gsx_skinny_gemm_nt", 64, a)) return rc;
  const SkinnyPick p = skinny_pick((M + 15) / 16, N, K / kSkinnyKTile[kind]);
  if (int rc = skinny_validate_splits("gsx_skinny_gemm_nt", a, p.splits)) return rc;
  return event_time(stream, iters, ms, [&] { return skinny_run("gsx_skinny_gemm_nt", stream, a); });
}

}  // extern "C"
