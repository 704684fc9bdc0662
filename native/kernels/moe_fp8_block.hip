// Block-scaled fp8 grouped expert GEMM for MoE decode: for every pair p of a plan of gsx_moe_route, with e the expert
// of its slot, C[p][0..N) (bf16) = A[p / a_div][0..K) * B[e][N][K]^T on the operands of gsx_gemm_fp8_block_nt grouped
// by expert: OCP e4m3, one fp32 scale per 1 x 128 group of a row of A and one per 128 x 128 block of an expert's matrix.
// It is what gsx_moe_gemm_nt (gemm_decode.hip) is for per-row scales, for the weight format of the DeepSeek-V3 / R1,
// Kimi K2 and Qwen3 "-FP8" checkpoints: only the experts that were hit are read, each byte once, and nothing goes
// through the host.  C ABI and the numeric contract in gsx_kernels.h.
//
// THE PLAN OF THE KERNEL
// * A workgroup is (strip of BN = 16 NF columns, slot of the plan); the grid is (N / BN, min(E, P)) whatever the plan
//   holds.  A workgroup whose slot is not active (slot >= n_active, an expert outside [0, E), no row) returns before
//   any barrier and has read four words of the plan and nothing else.  No split of K over workgroups, no workspace, no
//   atomics, one launch.
// * An expert has at most 16 rows, so there is ONE row fragment: the transposed product of gemm_skinny_fp8_block.hip at
//   MF = 1.  B's fragment is the MFMA's first operand, lane (fr, fq) holds row fr of the slot against columns
//   4 fq .. 4 fq + 3 of each of the NF column fragments: one row of A, one pair, one scale_a value per lane.
// * The W waves interleave the K-tiles of 128 (wave w takes w, w + W, ...).  B goes from HBM to VGPRs in fragment shape,
//   two 16-B loads per lane, column fragment and K-tile, each byte of an active expert by exactly one wave of one
//   workgroup.  A wave keeps F K-tiles in flight in a register ring behind counted waits.  A slot of the ring is
//   8 NF + 8 + 1 registers and one SGPR (at MF = 8 the skinny kernel pays 8 NF + 72), so the narrow strips afford
//   F = 8 and F = 4 where that kernel had one or two: the short rows of an expert (K = 2048 is 16 K-tiles) leave a wave
//   few tiles, and what hides the latency of HBM is how many of them are in the air at once, over all waves of a CU.
// * A and scale_a are GATHERED through the plan: the lane's row is pair / a_div of the pair its fragment row holds, as
//   the checked (vector) offset of a buffer load over exactly ceil(P / a_div) rows, the K-tile in the scalar offset.
//   A lane without a pair (fragment row >= count, an index or a pair the plan must not name) gets the offset of row
//   ceil(P / a_div), which is the end of both buffers: zeros for A and a zero scale, no branch, nothing read.
// * scale_b is one scalar load per wave and K-tile, from block row col0 / 128 of expert e (N % 64 == 0 and BN <= 64: a
//   strip never crosses a multiple of 128 columns); the expert's offset e * ceil(N / 128) * (K / 128) is 64-bit.
// * Per K-tile: s = scale_a * scale_b; NF MFMAs from a zero accumulator; the loads of the tile F ahead into the slot
//   just read; then the fold acc = fma(p, s, acc), which so runs behind the loads just issued and in front of the wait
//   for the next slot.
// * The waves' accumulators meet in LDS: waves 0 .. W - 2 write theirs, one barrier, and wave W - 1 adds them in the
//   order of the wave index, its own last, rounds once to bf16 and stores 8 B per lane and column fragment to row
//   `pair` of C.  ((w0 + w1) + w2) + w3 is the chain of sfb_kernel, so at W = 4 a pair's row has the bits that
//   gsx_skinny_gemm_fp8_block_nt_launch_cfg gives at splits = 1.
// * REGISTERS.  acc 4 NF, p 4 NF, the ring F (8 NF + 9): at most 160 by this count.  Every instantiation is given
//   amdgpu_waves_per_eu(2), 256 registers, so that the MFMA results stay in VGPRs for the fold (allowed 512 the
//   compiler puts them into AGPRs; profiles/gemm_fp8_block/README.md).  The counts of every instantiation are in
//   profiles/moe_fp8_block/README.md: none uses scratch.
//
// SAFETY: the plan is device memory anyone may have written.  The rules are gsx_moe_gemm_nt's: a slot >= n_active or
// >= GSX_MOE_MAX_PAIRS returns, an expert outside [0, E) is skipped, slot_count is clamped to [0, 16], an index into
// rows outside [0, GSX_MOE_MAX_PAIRS) and a pair outside [0, P) are dropped, no load and no store.
//
// DETERMINISM: a wave folds its K-tiles in ascending order and the waves' sums are added by index: the bits of a pair's
// row depend on W and on nothing else, not on M, the routing, the slot or where workgroups run.
//
// Offsets into B, scale_b and C are 64-bit; a buffer's range and a lane's offset into it are 32-bit: A's rows and
// scale_a's, and one row more, have to stay below 4 GiB, which is refused otherwise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

struct MfbPlan {
  const int32_t* plan;
  int P, E, a_div, a_rows;
};

template <int NF, int W, int F>
__global__ __launch_bounds__(W * 64) __attribute__((amdgpu_waves_per_eu(2)))
void mfb_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, uint16_t* __restrict__ C, MfbPlan gp,
                int N, int K, const float* __restrict__ sa, uint32_t sa_stride, const float* __restrict__ sb) {
  using OP = Fp8K128;
  using frag = OP::frag;
  constexpr int S = GSX_MOE_MAX_PAIRS;
  const int slot = blockIdx.y;
  if (slot >= gp.plan[0] || slot >= S) return;
  const int e = gp.plan[4 + slot];
  if (e < 0 || e >= gp.E) return;
  const int count = gp.plan[4 + 2 * S + slot];
  if (count <= 0) return;
  const int M = count > 16 ? 16 : count;
  const int begin = gp.plan[4 + S + slot];
  const int32_t* const rows = gp.plan + 4 + 3 * S;

  const int nk = K / ROW_BYTES;
  __shared__ f32x4 red[W > 1 ? W - 1 : 1][NF][64];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const size_t col0 = static_cast<size_t>(blockIdx.x) * (NF * 16);
  const int mine = wid < nk ? (nk - wid + W - 1) / W : 0;  // K-tiles wid, wid + W, ...

  // the pair of the lane's fragment row, or -1: what the plan must not name is dropped
  int pair = -1;
  const uint32_t idx = static_cast<uint32_t>(begin) + static_cast<uint32_t>(fr);
  if (fr < M && idx < static_cast<uint32_t>(S)) {
    const int p = rows[idx];
    pair = p >= 0 && p < gp.P ? p : -1;
  }
  // the pair's row of A and of scale_a as byte offsets into buffers of exactly a_rows rows; without a pair, their end
  const uint32_t an = static_cast<uint32_t>(gp.a_rows);
  const uint32_t ar = pair >= 0 ? static_cast<uint32_t>(pair / gp.a_div) : an;
  const uint32_t arow_bytes = static_cast<uint32_t>(K);
  const __amdgpu_buffer_rsrc_t abuf = rows_buffer(A, an * arow_bytes);
  const __amdgpu_buffer_rsrc_t sbuf = rows_buffer(sa, an * sa_stride * 4);
  const int aoff = static_cast<int>(ar * arow_bytes + fq * CHUNK);
  const int soff = static_cast<int>(ar * sa_stride * 4);
  const uint8_t* const be = B + static_cast<size_t>(e) * N * K;
  const uint8_t* bp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) bp[f] = be + (col0 + f * 16 + fr) * K + fq * CHUNK;
  // the strip's block row of the expert's scale_b
  const float* const sbw = sb + (static_cast<size_t>(e) * ((N + 127) / 128) + col0 / 128) * nk;

  // the ring: slot i holds one K-tile's fragments of A and of B, its value of scale_a and its value of scale_b
  frag ra[F][2], rb[F][NF][2];
  float rs[F], rsb[F];

  auto load = [&](auto ring, int j) {
    constexpr int i = decltype(ring)::value;
    const int kt = wid + j * W;
    rsb[i] = sbw[kt];
    rs[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sbuf, soff, kt * 4, 0));
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int c = 0; c < 2; ++c) rb[i][f][c] = load_chunk<frag, false>(bp[f] + kt * ROW_BYTES + c * 4 * CHUNK);
#pragma unroll
    for (int c = 0; c < 2; ++c)
      ra[i][c] = __builtin_bit_cast(
          frag, __builtin_amdgcn_raw_buffer_load_b128(abuf, aoff + c * 4 * CHUNK, kt * ROW_BYTES, 0));
  };

  f32x4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  // One K-tile: its MFMAs from zero, (`refill`) the loads of the wave's tile `next` into the slot, then its fold.
  auto tile = [&](auto ring, bool refill, int next) {
    constexpr int i = decltype(ring)::value;
    const float s = rs[i] * rsb[i];
    f32x4 p[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      p[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      OP::mma(p[f], rb[i][f], ra[i]);  // B first: register j is column 4 fq + j, the lane's row of A is fr
    }
    __builtin_amdgcn_sched_barrier(0);  // the loads go behind the MFMAs that free their registers, the fold behind them
    if (refill) load(ring, next);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[f][j] = __builtin_fmaf(p[f][j], s, acc[f][j]);
  };

  // sfb_kernel's loop: slot i holds tile t + i until its MFMAs, then tile t + i + F.  The steady loop has no condition
  // inside and is entered behind an unconditional prologue, so that on every path to its top the F tiles were issued
  // in slot order and the wait for slot 0 leaves the F - 1 younger tiles in flight; the last 2 F - 1 tiles or fewer
  // drain in two conditional passes.
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

  // Waves 0 .. W - 2 leave their blocks in LDS; a wave without a tile leaves its zeros.  Every wave reaches the barrier.
  if constexpr (W > 1) {
    if (wid != W - 1) {
#pragma unroll
      for (int f = 0; f < NF; ++f) red[wid][f][lane] = acc[f];
    }
    __syncthreads();
  }
  if (wid != W - 1 || pair < 0) return;
  uint16_t* const crow = C + static_cast<size_t>(pair) * N + col0 + fq * 4;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f32x4 s = acc[f];
    if constexpr (W > 1) {
      s = red[0][f][lane];  // ((w0 + w1) + ...) + w(W-1): the order of the wave index
#pragma unroll
      for (int w = 1; w < W - 1; ++w) {
        const f32x4 v = red[w][f][lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] + v[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = s[j] + acc[f][j];
    }
    i32x2 v;
    v[0] = static_cast<int>(f2bf(s[0]) | (static_cast<uint32_t>(f2bf(s[1])) << 16));
    v[1] = static_cast<int>(f2bf(s[2]) | (static_cast<uint32_t>(f2bf(s[3])) << 16));
    *reinterpret_cast<i32x2*>(crow + f * 16) = v;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct MfbArgs {
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

static int mfb_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

// Everything the entry points refuse, before the first device call.  `bn`: the columns of a strip.
static int mfb_validate(const char* who, int bn, const MfbArgs& a) {
  if (a.M < 1 || a.M > 16) return mfb_refuse(who, "need 1 <= M <= 16");
  if (a.E < 1) return mfb_refuse(who, "need E >= 1");
  if (a.topk < 1 || a.topk > 8 || a.topk > a.E) return mfb_refuse(who, "need 1 <= topk <= min(8, E)");
  if (a.a_div < 1) return mfb_refuse(who, "need a_div >= 1");
  if (a.N <= 0 || a.N % 64 || a.N % bn || a.K <= 0 || a.K % 128) return mfb_refuse(who, "need N%64==0, K%128==0");
  if (!a.A || !a.B || !a.C || !a.plan || !a.sa || !a.sb)
    return mfb_refuse(who, "A, B, C, plan, scale_a and scale_b must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.B) | reinterpret_cast<uintptr_t>(a.C)) % 16)
    return mfb_refuse(who, "operands must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.sa) | reinterpret_cast<uintptr_t>(a.sb) | reinterpret_cast<uintptr_t>(a.plan)) % 4)
    return mfb_refuse(who, "scale_a, scale_b and plan must be 4-B aligned");
  if (a.sa_stride < a.K / 128) return mfb_refuse(who, "need sa_stride >= K/128");
  // A lane without a pair points at the end of the buffers over A and scale_a, plus its place in the row: one row more
  // than they have must fit the 32-bit range too.
  const uint64_t P = static_cast<uint64_t>(a.M) * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const uint64_t k = a.K, g = k / 128;
  if ((a_rows + 1) * k > UINT32_MAX) return mfb_refuse(who, "A (and one row more) must fit a 32-bit buffer range");
  if (static_cast<uint64_t>(a.sa_stride) > UINT32_MAX / ((a_rows + 1) * 4))
    return mfb_refuse(who, "sa_stride too large: scale_a (and one row more) must fit a 32-bit buffer range");
  struct Span {
    const void* p;
    uint64_t bytes;
  };
  const uint64_t en = static_cast<uint64_t>(a.E) * a.N, eb = static_cast<uint64_t>(a.E) * ((a.N + 127) / 128);
  const Span in[] = {{a.A, a_rows * k},
                     {a.B, en * k},
                     {a.plan, GSX_MOE_PLAN_INTS * 4ull},
                     {a.sa, ((a_rows - 1) * static_cast<uint64_t>(a.sa_stride) + g) * 4},
                     {a.sb, eb * g * 4}};
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.C);
  for (const Span& s : in) {
    const uintptr_t y = reinterpret_cast<uintptr_t>(s.p);
    if (x < y + s.bytes && y < x + P * a.N * 2)
      return mfb_refuse(who, "C must not overlap A, B, plan, scale_a or scale_b");
  }
  return 0;
}

using mfb_launch_t = int (*)(const char* who, hipStream_t s, const MfbArgs& a);

template <int NF, int W, int F>
int mfb_launch(const char* who, hipStream_t s, const MfbArgs& a) {
  const int P = a.M * a.topk, a_rows = (P + a.a_div - 1) / a.a_div;
  const dim3 grid(a.N / (NF * 16), a.E < P ? a.E : P), block(W * 64);
  hipLaunchKernelGGL((mfb_kernel<NF, W, F>), grid, block, 0, s, static_cast<const uint8_t*>(a.A),
                     static_cast<const uint8_t*>(a.B), static_cast<uint16_t*>(a.C),
                     MfbPlan{a.plan, P, a.E, a.a_div, a_rows}, a.N, a.K, a.sa, static_cast<uint32_t>(a.sa_stride),
                     a.sb);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct MfbCfg {
  const char* name;
  int bn, waves, inflight;
  mfb_launch_t launch;
};
template <int NF, int W, int F>
constexpr MfbCfg mfb_cfg(const char* name) {
  return {name, NF * 16, W, F, &mfb_launch<NF, W, F>};
}

// name: columns of a strip / waves per workgroup - K-tiles in flight per wave
constexpr MfbCfg kMfbCfgs[] = {
    mfb_cfg<1, 4, 8>("16/4w-f8"), mfb_cfg<1, 8, 4>("16/8w-f4"), mfb_cfg<2, 4, 4>("32/4w-f4"),
    mfb_cfg<2, 8, 2>("32/8w-f2"), mfb_cfg<4, 4, 2>("64/4w-f2"),
};
constexpr int kNumMfbCfgs = sizeof(kMfbCfgs) / sizeof(kMfbCfgs[0]);

static const MfbCfg* mfb_row(int cfg) { return cfg >= 0 && cfg < kNumMfbCfgs ? &kMfbCfgs[cfg] : nullptr; }

// The dispatch rule, by N and the K-tiles nk of a row alone (the host does not know how many experts are hit):
//   nk >= 32        "32/8w-f2": eight waves still have four K-tiles each or more;
//   8 <= nk < 32    "32/4w-f4": four waves, a wave's whole share of a short row in flight at once;
//   nk < 8          "64/4w-f2": a wave has one or two K-tiles, and only a wider strip puts more bytes in the air.
// N does not enter.  Measured on one MI355X on rings of more than 2 GiB at M = 1 / 8 / 16, TB/s over the active experts'
// bytes, (hidden, ffn, experts, topk) up and down (profiles/moe_fp8_block/README.md has every cell):
//   (2048, 768, 128, 8)    1536 x 2048: 3.01 / 5.28 / 5.66     2048 x 768:   2.03 / 4.32 / 4.65
//   (4096, 14336, 8, 2)    28672 x 4096: 5.28 / 5.88 / 5.81    4096 x 14336: 4.80 / 5.19 / 5.77
//   (7168, 2048, 256, 8)   4096 x 7168: 5.30 / 5.96 / 6.21     7168 x 2048:  5.31 / 6.01 / 6.28
// The rule is more than 3 % behind the best cell in two of these 18: at 4096 x 14336 and M = 8 "16/8w-f4" is 4 % ahead
// (the only cell a 16-column strip wins), and at 2048 x 768 and M = 1 "32/4w-f4" is 5 % ahead of the wide strip, which
// at M = 8 and 16 is 22 and 25 % ahead of it.
static const MfbCfg& mfb_pick(int N, int nk) {
  (void)N;
  return kMfbCfgs[nk >= 32 ? 3 : nk >= 8 ? 2 : 4];
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_moe_gemm_fp8_block_cfg_name(int cfg) { return mfb_row(cfg) ? mfb_row(cfg)->name : nullptr; }

int gsx_moe_gemm_fp8_block_cfg_shape(int cfg, int* bn, int* waves, int* inflight) {
  const MfbCfg* c = mfb_row(cfg);
  if (!c) return -1;
  *bn = c->bn;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_moe_gemm_fp8_block_nt_launch_cfg(void* stream, const void* A, int a_div, const void* B, void* C,
                                         const int32_t* plan, int M, int topk, int E, int N, int K,
                                         const float* scale_a, int64_t sa_stride, const float* scale_b, int cfg) {
  const char* who = "gsx_moe_gemm_fp8_block_nt_launch_cfg";
  const MfbCfg* c = mfb_row(cfg);
  if (!c) return mfb_refuse(who, "unknown config");
  const MfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  if (int rc = mfb_validate(who, c->bn, a)) return rc;
  return c->launch(who, S(stream), a);
}

int gsx_moe_gemm_fp8_block_nt(void* stream, const void* A, int a_div, const void* B, void* C, const int32_t* plan,
                              int M, int topk, int E, int N, int K, const float* scale_a, int64_t sa_stride,
                              const float* scale_b) {
  const char* who = "gsx_moe_gemm_fp8_block_nt";
  const MfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  if (int rc = mfb_validate(who, 64, a)) return rc;
  return mfb_pick(N, K / 128).launch(who, S(stream), a);
}

int gsx_event_time_moe_gemm_fp8_block(void* stream, const void* A, int a_div, const void* B, void* C,
                                      const int32_t* plan, int M, int topk, int E, int N, int K, const float* scale_a,
                                      int64_t sa_stride, const float* scale_b, int iters, float* ms) {
  const char* who = "gsx_moe_gemm_fp8_block_nt";  // refused before the events are made, under the timed name
  const MfbArgs a{A, a_div, B, C, plan, M, topk, E, N, K, scale_a, sa_stride, scale_b};
  if (int rc = mfb_validate(who, 64, a)) return rc;
  return event_time(stream, iters, ms, [&] { return mfb_pick(N, K / 128).launch(who, S(stream), a); });
}

}  // extern "C"
