// Block-scaled fp8 skinny GEMM: C[M][N] (bf16) = A[M][K] * B[N][K]^T with 1 <= M <= 128 on the operands of
// gsx_gemm_fp8_block_nt (gemm_fp8_block.hip): OCP e4m3, one fp32 scale per 1 x 128 group of a row of A and one per
// 128 x 128 block of B.  It is the skinny GEMM (gemm_skinny.hip) for the weight format of the DeepSeek-V3 / R1, Kimi K2
// and Qwen3 "-FP8" checkpoints: the weights are read from HBM exactly once and rows past M cost nothing beyond the last
// fragment of 16.  C ABI and the numeric contract in gsx_kernels.h.
//
// The plan is skinny_kernel's: a workgroup is (strip, split), a strip of BN = 16 NF columns and all MF = ceil(M / 16)
// row fragments over one of `splits` runs of consecutive K-tiles; its W waves interleave the run's K-tiles (wave w takes
// tiles w, w + W, ...); B goes from global memory to VGPRs in fragment shape, two 16-B loads per lane, fragment and
// K-tile, each byte loaded by exactly one wave of one workgroup; A comes through bounds-checked buffer loads whose range
// is exactly the M rows; a wave keeps F K-tiles in flight in a register ring behind counted waits; the waves'
// accumulators meet in LDS in the order of the wave index.  A K-tile is 128 B of a row, which in e4m3 is exactly one
// scale block and one v_mfma_f32_16x16x128_f8f6f4.
//
// What the scales change:
// * THE PRODUCT IS TRANSPOSED.  A scale that changes along K cannot wait for the epilogue: the MFMA of a K-tile starts
//   from a zero accumulator and its result p is folded into the running sum on the VALU, acc = fma(p, s, acc) with
//   s = fl(scale_a[row][g] * scale_b[nb][g]).  B's fragment is the MFMA's first operand, as in gemm_fp8_block.hip, so
//   lane (fr, fq) holds row fr of A's fragment against columns 4 fq .. 4 fq + 3 of B's: one row of A per lane and
//   fragment, hence one scale_a value and one product s per fragment and K-tile instead of four, and the four FMAs of a
//   fragment share their multiplier (v_pk_fma_f32 with one broadcast operand).  The store gains as well: a lane's four
//   values are four consecutive columns of one row, 8 B of bf16 to C or 16 B of fp32 to the workspace.
// * scale_b IS A SCALAR.  N % 64 == 0 and BN <= 64, so a strip never crosses a multiple of 128 columns, and a wave's
//   K-tile is uniform over the wave: scale_b[col0 / 128][g] is one scalar load per wave and K-tile, issued with the
//   K-tile's operands and held in the ring.
// * scale_a RIDES IN THE RING with its K-tile: MF buffer loads of 4 B per lane and K-tile, over a buffer whose range
//   is M rows of sa_stride floats, the row in the lane's offset (the checked one) and the K-tile in the scalar offset.
//   A lane of the ragged last fragment whose row is >= M gets a zero scale against the zero product of its zero row of
//   A, with no branch, and nothing of scale_a is read past row M - 1.  The alternative, staging the run's scales in
//   LDS once per workgroup, was not built: the image is M x (K-tiles of the run) floats, 112 KiB at M = 128, K = 28672
//   and one split, so it would have to be restaged in pieces behind barriers, and the waves of this kernel otherwise
//   do not meet before the end; the ring needs no barrier and its cost is bounded (MF of 2 (MF + NF) + MF loads and MF
//   registers per slot).  The lanes of a load read 16 different rows, 4 lanes each: 16 sectors per instruction, all in
//   L2 after the first workgroup of a split (scale_a is M K / 32 bytes, 1 / 32 of A).
// * THE FOLD SITS BEHIND THE LOADS.  Per slot of the ring, in this order: the MF products s; then m-major, the NF MFMAs
//   of row fragment m into p[m & 1] followed by the fold of row fragment m - 1, whose MFMAs have left the pipe by then
//   (the VALU works under the matrix pipe); then the loads of the K-tile F ahead into the slot's registers; then the
//   fold of the last row fragment, which so runs behind the loads just issued and in front of the wait for the next
//   slot.  p is 2 x NF fragments, 8 NF registers, not MF NF.
// * REGISTERS.  acc 4 MF NF (128 at MF = 8, NF = 4), p 8 NF, a slot 8 (MF + NF) + MF and one SGPR.  An instantiation
//   that fits 256 registers by this count is given amdgpu_waves_per_eu(2): allowed 512 the compiler puts MFMA results
//   into AGPRs and every fold pays v_accvgpr_read first (profiles/gemm_fp8_block/README.md).  The larger ones have 4
//   waves, one per SIMD, and may use all 512; there an empty asm with a "v" constraint in front of the fold says
//   where the result has to be, and the AGPRs take ring registers instead.  The wide strip keeps ONE K-tile in flight
//   (F = 1): with two, MF = 7 and 8 at NF = 4 did not compile into 512 registers without scratch (acc 128 + ring 208 +
//   p 32 + scales 24 is 392, the compiler needed 580), and a configuration serves every M.  The counts of every
//   instantiation are in profiles/gemm_skinny_fp8_block/README.md: none uses scratch.
//
// sfb_reduce_kernel (splits > 1 only, the next launch on the same stream): the partials in the workspace are already
// scaled, so it only adds them in the order of the split index and rounds once.  No atomics, and no workgroup waits
// for another.
//
// DETERMINISM: a wave folds its K-tiles in ascending order, the waves' sums are added by index, the splits' by index,
// one rounding to bf16.  A row's accumulators never meet another row's, and neither MF nor the ragged fragment changes
// what is added to them: row i of C has the same bits at every M that contains it, given the configuration and
// `splits`.  The order is not that of gsx_gemm_fp8_block_nt (one chain over all g).
//
// Row offsets into B, scale_b, C and the workspace are 64-bit; a buffer's range and a lane's offset into it are 32-bit:
// 16 MF rows of A and of scale_a have to stay below 4 GiB, which is refused otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int kSfbMaxM = 128, kSfbMaxMF = kSfbMaxM / 16, kSfbMaxSplits = 16;

// Whether an instantiation fits 256 registers: the count above with 2 MF + 2 NF + 52 for offsets, addresses and what
// the compiler keeps besides, set so that every instantiation it lets through compiles into 256 without scratch.
constexpr bool sfb_fits_256(int MF, int NF, int F) {
  return 4 * MF * NF + 8 * NF + F * (8 * (MF + NF) + MF) + 3 * MF + 2 * NF + 52 <= 256;
}

// `part` is the workspace, or nullptr with a grid of one split; `per` the K-tiles of a split's run.
template <int MF, int NF, int W, int F>
__global__ __launch_bounds__(W * 64) __attribute__((amdgpu_waves_per_eu(sfb_fits_256(MF, NF, F) ? 2 : 1)))
void sfb_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, uint16_t* __restrict__ C,
                float* __restrict__ part, int M, int N, int K, int per, const float* __restrict__ sa,
                uint32_t sa_stride, const float* __restrict__ sb) {
  using OP = Fp8K128;
  using frag = OP::frag;
  const int nk = K / ROW_BYTES;
  __shared__ f32x4 red[MF * NF][64];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const size_t col0 = static_cast<size_t>(blockIdx.x) * (NF * 16);
  const int split = blockIdx.y;
  const int first = split * per;  // the run's first K-tile; splits * per < nk + 16, no overflow
  const int run = nk - first < per ? (nk - first > 0 ? nk - first : 0) : per;
  const int mine = wid < run ? (run - wid + W - 1) / W : 0;  // K-tiles first + wid, first + wid + W, ...

  // A's rows and scale_a's as byte offsets into buffers of exactly M rows: past the end for a row >= M
  const uint32_t arow_bytes = static_cast<uint32_t>(K);
  const __amdgpu_buffer_rsrc_t abuf = rows_buffer(A, static_cast<uint32_t>(M) * arow_bytes);
  const __amdgpu_buffer_rsrc_t sbuf = rows_buffer(sa, static_cast<uint32_t>(M) * sa_stride * 4);
  const uint32_t aoff = static_cast<uint32_t>(fr) * arow_bytes + fq * CHUNK;
  const uint32_t soff = static_cast<uint32_t>(fr) * sa_stride * 4;
  const uint8_t* bp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) bp[f] = B + (col0 + f * 16 + fr) * K + fq * CHUNK;
  const float* sbw = sb + (col0 / 128) * nk;  // the strip's block row of scale_b

  // the ring: slot i holds one K-tile's fragments of A and of B, its MF values of scale_a and its value of scale_b
  frag ra[F][MF][2], rb[F][NF][2];
  float rs[F][MF], rsb[F];

  auto load = [&](auto slot, int j) {
    constexpr int i = decltype(slot)::value;
    const int kt = first + wid + j * W;
    rsb[i] = sbw[kt];
#pragma unroll
    for (int m = 0; m < MF; ++m)
      rs[i][m] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                               sbuf, static_cast<int>(soff + m * 16 * sa_stride * 4), kt * 4, 0));
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int c = 0; c < 2; ++c) rb[i][f][c] = load_chunk<frag, false>(bp[f] + kt * ROW_BYTES + c * 4 * CHUNK);
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

  // One K-tile: its MFMAs from zero, its folds one row fragment behind them, and (`refill`) the loads of the wave's
  // tile `next` into the slot in front of the last fold.
  auto tile = [&](auto slot, bool refill, int next) {
    constexpr int i = decltype(slot)::value;
    float s[MF];
#pragma unroll
    for (int m = 0; m < MF; ++m) s[m] = rs[i][m] * rsb[i];
    f32x4 p[2][NF];
    const auto fold = [&](int m) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        // allowed 512 registers the compiler would put the MFMA's result into AGPRs: this keeps it in VGPRs
        if constexpr (!sfb_fits_256(MF, NF, F)) asm volatile("" : "+v"(p[m & 1][f]));
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][f][j] = __builtin_fmaf(p[m & 1][f][j], s[m], acc[m][f][j]);
      }
    };
    static_for<MF>([&](auto mm) {
      constexpr int m = decltype(mm)::value;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        p[m & 1][f] = f32x4{0.f, 0.f, 0.f, 0.f};
        OP::mma(p[m & 1][f], rb[i][f], ra[i][m]);  // B first: register j is column 4 fq + j, the lane's row of A is fr
      }
      if constexpr (m > 0) fold(m - 1);
      __builtin_amdgcn_sched_barrier(0);  // or every MFMA of the K-tile is issued first and all MF NF results live
    });
    if (refill) load(slot, next);
    fold(MF - 1);
  };

  // skinny_kernel's loop: slot i holds tile t + i until its MFMAs, then tile t + i + F.  The steady loop has no
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
        tile(i, true, t + i + F);
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
    if (t + i < mine) tile(i, t + i + F < mine, t + i + F);
  });
  static_for<F>([&](auto i) {
    if (t + F + i < mine) tile(i, false, 0);
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
  for (int m = 0; m < MF; ++m) {
    const int row = m * 16 + fr;  // transposed 16x16 map: row fr, columns 4 fq .. 4 fq + 3
    if (row >= M) continue;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      f32x4 s = acc[m][f];
      if constexpr (W > 1) {
        const f32x4 v = red[m * NF + f][lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = v[j] + s[j];
      }
      const size_t col = col0 + f * 16 + fq * 4;
      if (part != nullptr) {
        *reinterpret_cast<f32x4*>(part + (static_cast<size_t>(split) * M + row) * N + col) = s;
      } else {
        i32x2 v;
        v[0] = static_cast<int>(f2bf(s[0]) | (static_cast<uint32_t>(f2bf(s[1])) << 16));
        v[1] = static_cast<int>(f2bf(s[2]) | (static_cast<uint32_t>(f2bf(s[3])) << 16));
        *reinterpret_cast<i32x2*>(C + static_cast<size_t>(row) * N + col) = v;
      }
    }
  }
}

// One thread per four columns of a row: part[0] + part[1] + ... in this order, one rounding.
__global__ __launch_bounds__(256) void sfb_reduce_kernel(const float* __restrict__ part, uint16_t* __restrict__ C,
                                                         int M, int N, int splits) {
  const size_t quads = static_cast<size_t>(N / 4);
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= quads * M) return;
  const size_t plane = static_cast<size_t>(M) * N, at = t * 4;  // row t / quads, column (t % quads) * 4
  f32x4 s = *reinterpret_cast<const f32x4*>(part + at);
  for (int i = 1; i < splits; ++i) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + i * plane + at);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j];
  }
  i32x2 v;
  v[0] = static_cast<int>(f2bf(s[0]) | (static_cast<uint32_t>(f2bf(s[1])) << 16));
  v[1] = static_cast<int>(f2bf(s[2]) | (static_cast<uint32_t>(f2bf(s[3])) << 16));
  *reinterpret_cast<i32x2*>(C + at) = v;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct SfbArgs {
  const void* A;
  const void* B;
  void* C;
  int M, N, K;
  const float* sa;
  int64_t sa_stride;
  const float* sb;
  void* ws;
  uint64_t ws_bytes;
};

static int sfb_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

static uint64_t sfb_workspace(int M, int N, int splits) {
  return splits > 1 ? static_cast<uint64_t>(splits) * M * N * sizeof(float) : 0;
}

// Everything the entry points refuse but what depends on `splits`, before the first device call.  `bn`: the columns
// of a strip.
static int sfb_validate(const char* who, int bn, const SfbArgs& a) {
  if (a.M < 1 || a.M > kSfbMaxM) return sfb_refuse(who, "need 1 <= M <= 128");
  if (a.N <= 0 || a.N % 64 || a.N % bn || a.K <= 0 || a.K % 128) return sfb_refuse(who, "need N%64==0, K%128==0");
  if (!a.A || !a.B || !a.C || !a.sa || !a.sb) return sfb_refuse(who, "A, B, C, scale_a and scale_b must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.B) | reinterpret_cast<uintptr_t>(a.C) |
       reinterpret_cast<uintptr_t>(a.ws)) % 16)
    return sfb_refuse(who, "operands and workspace must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.sa) | reinterpret_cast<uintptr_t>(a.sb)) % 4)
    return sfb_refuse(who, "scale_a and scale_b must be 4-B aligned");
  if (a.sa_stride < a.K / 128) return sfb_refuse(who, "need sa_stride >= K/128");
  // a lane's offset into the buffers over A's and scale_a's rows is 32-bit, the rows of the ragged fragment included
  const uint64_t rows = static_cast<uint64_t>((a.M + 15) / 16 * 16);
  if (rows * static_cast<uint64_t>(a.K) > UINT32_MAX)
    return sfb_refuse(who, "K too large: the row fragments of A must fit a 32-bit buffer range");
  if (static_cast<uint64_t>(a.sa_stride) > UINT32_MAX / (rows * 4))
    return sfb_refuse(who, "sa_stride too large: the row fragments of scale_a must fit a 32-bit buffer range");
  return 0;
}

// What depends on `splits`: its range, the workspace, and that C overlaps nothing, the workspace included.
static int sfb_validate_splits(const char* who, const SfbArgs& a, int splits) {
  if (splits < 1 || splits > kSfbMaxSplits) return sfb_refuse(who, "need 1 <= splits <= 16");
  const uint64_t need = sfb_workspace(a.M, a.N, splits);
  if (need && (!a.ws || a.ws_bytes < need)) {
    char msg[200];
    std::snprintf(msg, sizeof(msg), "%s: workspace too small: splits %d needs %llu bytes", who, splits,
                  static_cast<unsigned long long>(need));
    return fail_arg(msg);
  }
  struct Span {
    const void* p;
    uint64_t bytes;
  };
  const uint64_t m = a.M, n = a.N, k = a.K, g = k / 128;
  const Span in[] = {{a.A, m * k},
                     {a.B, n * k},
                     {a.sa, ((m - 1) * static_cast<uint64_t>(a.sa_stride) + g) * 4},
                     {a.sb, (n + 127) / 128 * g * 4},
                     {need ? a.ws : nullptr, need}};
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.C);
  for (const Span& s : in) {
    const uintptr_t y = reinterpret_cast<uintptr_t>(s.p);
    if (s.p && x < y + s.bytes && y < x + m * n * 2)
      return sfb_refuse(who, "C must not overlap A, B, scale_a, scale_b or the workspace");
  }
  return 0;
}

using sfb_launch_t = int (*)(const char* who, hipStream_t s, const SfbArgs& a, int splits);

template <int MF, int NF, int W, int F>
int sfb_launch(const char* who, hipStream_t s, const SfbArgs& a, int splits) {
  const int nk = a.K / 128, per = (nk + splits - 1) / splits;
  uint16_t* c = static_cast<uint16_t*>(a.C);
  float* part = splits > 1 ? static_cast<float*>(a.ws) : nullptr;
  hipLaunchKernelGGL((sfb_kernel<MF, NF, W, F>), dim3(a.N / (NF * 16), splits), dim3(W * 64), 0, s,
                     static_cast<const uint8_t*>(a.A), static_cast<const uint8_t*>(a.B), c, part, a.M, a.N, a.K, per,
                     a.sa, static_cast<uint32_t>(a.sa_stride), a.sb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, who);
  if (splits > 1) {
    const uint64_t quads = static_cast<uint64_t>(a.M) * (a.N / 4);
    hipLaunchKernelGGL(sfb_reduce_kernel, dim3(static_cast<uint32_t>((quads + 255) / 256)), dim3(256), 0, s, part, c,
                       a.M, a.N, splits);
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : fail(e, who);
}

struct SfbCfg {
  const char* name;
  int bn, waves, inflight;
  sfb_launch_t launch[kSfbMaxMF];  // indexed by MF - 1
};
template <int NF, int W, int F, int... MF>
constexpr SfbCfg sfb_cfg(const char* name, std::integer_sequence<int, MF...>) {
  return {name, NF * 16, W, F, {&sfb_launch<MF + 1, NF, W, F>...}};
}
template <int NF, int W, int F>
constexpr SfbCfg sfb_cfg(const char* name) {
  return sfb_cfg<NF, W, F>(name, std::make_integer_sequence<int, kSfbMaxMF>{});
}

// name: columns of a strip / waves per workgroup - K-tiles in flight per wave
constexpr SfbCfg kSfbCfgs[] = {
    sfb_cfg<2, 4, 2>("32/4w-f2"),
    sfb_cfg<4, 4, 1>("64/4w-f1"),
    sfb_cfg<2, 4, 1>("32/4w-f1"),
};
constexpr int kNumSfbCfgs = sizeof(kSfbCfgs) / sizeof(kSfbCfgs[0]);

static const SfbCfg* sfb_row(int cfg) { return cfg >= 0 && cfg < kNumSfbCfgs ? &kSfbCfgs[cfg] : nullptr; }

// The dispatch rule, by MF = ceil(M / 16), N and the K-tiles nk of a row of B.  It is skinny_pick()'s (gemm_skinny.hip):
//   configuration   "64/4w-f1", except "32/4w-f2" where M <= 64 and N < 8192: the wide strip fetches A and scale_a half
//                   as often and is taken wherever it still gives 128 strips;
//   splits          as many as give 256 workgroups of the wide strip or 512 of the narrow one, but no more than leave
//                   every wave 2 F K-tiles, so that it runs the steady loop, and at most 16.
// The rule was taken over and then measured, not tuned.  On one MI355X on a ring of more than 2 GiB, TB/s of weight
// bytes at M = 17 / 32 / 64 / 128, dispatched (profiles/gemm_skinny_fp8_block/README.md has every cell):
//   8192 x 8192    3.39 / 3.27 / 2.49 / 1.62      padded to 128 rows on gsx_gemm_fp8_block_nt: 0.96
//   8192 x 28672   4.96 / 4.29 / 3.13 / 2.00                                                   1.00
//   1024 x 8192    0.95 / 0.84 / 0.64 / 0.44                                                   0.12
//   4096 x 7168    2.10 / 1.77 / 1.25 / 1.15                                                   0.47
//   7168 x 16384   3.37 / 2.77 / 1.82 / 1.23                                                   0.90
// The padded large GEMM wins no row.  The rule is not the best cell in 12 of these 20 rows: at N = 4096 and 7168 with
// M <= 64 it takes the narrow strip where the wide one is up to 26 % faster; at N = 1024 eight splits are 8 to 15 %
// ahead of four at M <= 64 and the narrow strips 22 % ahead of the wide one at M = 128; at 7168 x 16384 one split is 4
// to 8 % ahead of three at M <= 64 and six 13 % ahead at M = 128; at 8192 x 8192 and M = 17 four splits are 8 % ahead
// of two.
struct SfbPick {
  int cfg, splits;
};
static SfbPick sfb_pick(int mf, int N, int nk) {
  const int cfg = mf <= 4 && N / 64 < 128 ? 0 : 1;
  const SfbCfg& c = kSfbCfgs[cfg];
  const int strips = N / c.bn, want = cfg == 0 ? 512 : 256;
  int splits = (want + strips - 1) / strips;
  const int steady = nk / (c.waves * 2 * c.inflight);
  if (splits > steady) splits = steady;
  if (splits > kSfbMaxSplits) splits = kSfbMaxSplits;
  return {cfg, splits < 1 ? 1 : splits};
}

static int sfb_run(const char* who, void* stream, const SfbArgs& a) {
  const SfbPick p = sfb_pick((a.M + 15) / 16, a.N, a.K / 128);
  if (int rc = sfb_validate_splits(who, a, p.splits)) return rc;
  return kSfbCfgs[p.cfg].launch[(a.M + 15) / 16 - 1](who, S(stream), a, p.splits);
}

static int sfb_shape(const char* who, int M, int N, int K) {
  if (M < 1 || M > kSfbMaxM) return sfb_refuse(who, "need 1 <= M <= 128");
  if (N <= 0 || N % 64 || K <= 0 || K % 128) return sfb_refuse(who, "need N%64==0, K%128==0");
  return 0;
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_skinny_gemm_fp8_block_cfg_name(int cfg) { return sfb_row(cfg) ? sfb_row(cfg)->name : nullptr; }

int gsx_skinny_gemm_fp8_block_cfg_shape(int cfg, int* bn, int* waves, int* inflight) {
  const SfbCfg* c = sfb_row(cfg);
  if (!c) return -1;
  *bn = c->bn;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_skinny_gemm_fp8_block_pick(int M, int N, int K, int* cfg, int* splits) {
  if (int rc = sfb_shape("gsx_skinny_gemm_fp8_block_pick", M, N, K)) return rc;
  const SfbPick p = sfb_pick((M + 15) / 16, N, K / 128);
  *cfg = p.cfg;
  *splits = p.splits;
  return 0;
}

int gsx_skinny_gemm_fp8_block_workspace_bytes(int M, int N, int K, uint64_t* bytes) {
  if (int rc = sfb_shape("gsx_skinny_gemm_fp8_block_workspace_bytes", M, N, K)) return rc;
  *bytes = sfb_workspace(M, N, sfb_pick((M + 15) / 16, N, K / 128).splits);
  return 0;
}

int gsx_skinny_gemm_fp8_block_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                            const float* scale_a, int64_t sa_stride, const float* scale_b,
                                            void* workspace, uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_skinny_gemm_fp8_block_nt_launch_cfg";
  const SfbCfg* c = sfb_row(cfg);
  if (!c) return sfb_refuse(who, "unknown config");
  const SfbArgs a{A, B, C, M, N, K, scale_a, sa_stride, scale_b, workspace, workspace_bytes};
  if (int rc = sfb_validate(who, c->bn, a)) return rc;
  if (int rc = sfb_validate_splits(who, a, splits)) return rc;
  return c->launch[(M + 15) / 16 - 1](who, S(stream), a, splits);
}

int gsx_skinny_gemm_fp8_block_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                 const float* scale_a, int64_t sa_stride, const float* scale_b, void* workspace,
                                 uint64_t workspace_bytes) {
  const SfbArgs a{A, B, C, M, N, K, scale_a, sa_stride, scale_b, workspace, workspace_bytes};
  if (int rc = sfb_validate("gsx_skinny_gemm_fp8_block_nt", 64, a)) return rc;
  return sfb_run("gsx_skinny_gemm_fp8_block_nt", stream, a);
}

int gsx_event_time_skinny_gemm_fp8_block(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                         const float* scale_a, int64_t sa_stride, const float* scale_b,
                                         void* workspace, uint64_t workspace_bytes, int iters, float* ms) {
  const char* who = "gsx_skinny_gemm_fp8_block_nt";  // refused before the events are made, under the timed name
  const SfbArgs a{A, B, C, M, N, K, scale_a, sa_stride, scale_b, workspace, workspace_bytes};
  if (int rc = sfb_validate(who, 64, a)) return rc;
  if (int rc = sfb_validate_splits(who, a, sfb_pick((M + 15) / 16, N, K / 128).splits)) return rc;
  return event_time(stream, iters, ms, [&] { return sfb_run(who, stream, a); });
}

}  // extern "C"
