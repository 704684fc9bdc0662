// Block-scaled fp8 GEMM and its activation quantiser: C[M][N] (bf16) = A[M][K] * B[N][K]^T on OCP e4m3 operands with
// one fp32 scale per 1 x 128 group of a row of A and one per 128 x 128 block of B, the format of the DeepSeek-V3 / R1,
// Kimi K2 and Qwen3 "-FP8" checkpoints.  C ABI and the numeric contract in gsx_kernels.h.
//
// A scale that changes along K cannot wait for the epilogue: every K block's partial product is scaled before it is
// added.  v_mfma_f32_16x16x128_f8f6f4 covers exactly one scale block per instruction, so the plan is
//
//   p   = MFMA(fragment of K-tile g, from a zero accumulator)        matrix pipe, a fresh 4 registers
//   acc = fma(p, s_g, acc),  s_g = fl(scale_a[row][g] * scale_b[nb][g])   VALU, 4 v_fma_f32 (2 v_pk_fma_f32)
//
// and everything else serves to keep the second line in the shadow of the first.
//
// * Block tile.  BN is 128 or 256 and a wave tile never straddles a multiple of 128 columns, so scale_b is one value
//   per wave and K-tile: a scalar load, issued one K-tile ahead.  A K-tile of the pipeline is one scale block.
//   Staging, swizzle and tile map are gemm_tile.h's (global_load_lds of 16 B, two LDS buffers, one __syncthreads per
//   K-tile); 128x128 with 4 waves is the baseline, 256x128 and 256x256 with 8 waves are the larger tiles.
// * Which operand is the MFMA's first.  B's rows are: the product is computed transposed, as the decode attention does
//   it.  In the 16x16 result lane (fr, fq) then holds row fr of A against columns 4 fq .. 4 fq + 3 of the fragment:
//   one row of A per lane and fragment.  A lane so needs MR = 4 values of scale_a per K-tile (one per 16 rows) and
//   forms MR products s_g; with A first it would hold four rows per fragment: 16 values, 16 multiplies and 12 more
//   live registers per K-tile, and every fma would take its own scale, which rules out v_pk_fma_f32 with one broadcast
//   multiplier.  The price is the epilogue: a lane's four values are four consecutive columns of one row, written to
//   LDS as one 8-B store and leaving in 16-B row stores, which is the transpose through LDS the family's epilogue is.
// * Two accumulators per fragment.  acc[MR][NR] stays in registers for the whole K loop (64 VGPRs for a 64x64 wave
//   tile, 128 for 128x64); p lives for LAG = 2 fragments.  Fragments go m-major; after the MFMA of fragment f is
//   issued the fold of fragment f - LAG follows, whose MFMA has left the pipe by then, so the VALU works while the
//   matrix pipe runs fragment f.  The last LAG folds of a K-tile are not done at its end, where nothing would cover
//   them before the barrier: they are carried over and issue behind the first MFMAs of the next K-tile (and once more
//   after the loop).
// * How scale_a reaches the lanes.  Through LDS, four K-tiles at a time: the image of a tile is [row][4 floats], 16 B
//   per row, 2 KiB for 128 rows, double-buffered behind the operand buffers.  It is written by global_load_lds of 4 B
//   per lane (lane l of a round: row l / 4, K-tile l % 4; 2 loads per wave and four K-tiles), not by one 16-B load per
//   row: scale_a is 4-B aligned and sa_stride is any number, so a row's four values are not 16-B aligned.  A lane whose
//   K-tile is past the last one fetches the last one again, so nothing beyond a row's K / 128 entries is read.  The
//   image of K-tiles 4 q .. 4 q + 3 is staged with the operands of K-tile 4 q, one K-tile before its first use, and
//   the buffer it replaces was last read two barriers earlier.  A lane reads its MR values per K-tile with ds_read_b32.
// * No atomics, no split of K, ascending g: the result does not depend on where or when a workgroup runs.
//
// The quantiser (gsx_quant_fp8_block): a group of 128 bf16 is 16 chunks of 16 B, one per lane of a 16-lane team, four
// teams to a wave; the amax goes round the team by xor shuffles (a max does not depend on order), and the rule is
// GSX_ACT_OUT_FP8_ROW's with the conversion norm_act.hip uses (e4m3_convert.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "e4m3_convert.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int FB_SQ = 4;             // K-tiles per scale image
constexpr int FB_SROW = FB_SQ * 4;   // bytes of a row of a scale image
constexpr int FB_LAG = 2;            // fragments between an MFMA and its fold

template <int BM, int BN>
constexpr int fb_lds_bytes() {
  return 2 * (BM + BN) * ROW_BYTES + 2 * BM * FB_SROW;
}

// Two waves per SIMD at least (two blocks of 4 waves or one of 8 per CU): with at most 256 registers a wave the
// compiler keeps the MFMA results in VGPRs, where the fold reads them; allowed 512 it puts them in AGPRs and every
// fold pays four v_accvgpr_read first.
template <int BM, int BN, int WM, int WN, int GROUP_M>
__global__ __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(2))) void gemm_fp8_block_kernel(const uint8_t* __restrict__ A,
                                                                     const uint8_t* __restrict__ B,
                                                                     uint16_t* __restrict__ C, int M, int N, int K,
                                                                     const float* __restrict__ sa, int64_t sa_stride,
                                                                     const float* __restrict__ sb) {
  using OP = Fp8K128;
  using frag = OP::frag;
  constexpr int NW = WM * WN;
  constexpr int TA = BM * ROW_BYTES, TB = BN * ROW_BYTES;  // bytes per operand tile
  constexpr int WTM = BM / WM, WTN = BN / WN;              // wave tile
  constexpr int MR = WTM / 16, NR = WTN / 16, F = MR * NR;
  constexpr int RA = TA / 1024 / NW, RB = TB / 1024 / NW;  // glds rounds per wave (1 KiB each)
  constexpr int RS = BM / 16 / NW;                         // and of a scale image (16 rows each)
  constexpr int SIMG = BM * FB_SROW;
  static_assert(RA >= 1 && RB >= 1 && TA % (1024 * NW) == 0 && TB % (1024 * NW) == 0, "tile/wave mismatch");
  static_assert(RS >= 1 && BM % (16 * NW) == 0, "scale image/wave mismatch");
  static_assert(BN % 128 == 0 && 128 % WTN == 0, "scale_b must be uniform over a wave tile");
  static_assert(WTN == 64, "the epilogue's swizzle is written for rows of 8 chunks");
  static_assert(FB_LAG >= 1 && FB_LAG <= NR, "the carried fragments share the last m");
  static_assert(NW * WTM * WTN * 2 <= 2 * (TA + TB), "epilogue staging must fit in the operand buffers");
  extern __shared__ __attribute__((aligned(16))) char lds[];  // [buf][A|B], [buf] scale images

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / WN, wc = wid % WN;
  const int fr = lane & 15, fq = lane >> 4;

  int tm, tn;
  tile_of<BM, BN, GROUP_M>(blockIdx.x, gridDim.x, M, N, tm, tn);
  const int row0 = tm * BM, col0 = tn * BN;
  const int nk = K / ROW_BYTES;

  int off[RA > RB ? RA : RB];  // round i loads the same rows and slots of an A tile and of a B tile
#pragma unroll
  for (int i = 0; i < (RA > RB ? RA : RB); ++i) {
    const int p = (i * NW + wid) * 64 + lane;
    off[i] = (p >> 3) * K + glds_col<uint8_t>(p);
  }
  const uint8_t* Ab = A + static_cast<size_t>(row0) * K;
  const uint8_t* Bb = B + static_cast<size_t>(col0) * K;
  auto stage = [&](int kt, int buf) {
    char* la = lds + buf * (TA + TB);
    char* lb = la + TA;
#pragma unroll
    for (int i = 0; i < RA; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Ab + off[i] + kt * ROW_BYTES), (lptr_t)(la + (i * NW + wid) * 1024),
                                       16, 0, 0);
#pragma unroll
    for (int i = 0; i < RB; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * ROW_BYTES), (lptr_t)(lb + (i * NW + wid) * 1024),
                                       16, 0, 0);
  };

  // scale_a: image q holds K-tiles 4 q .. 4 q + 3 of the tile's rows; lane l of round i fetches row
  // (i NW + wid) 16 + l / 4, K-tile 4 q + l % 4 (the last K-tile where that is past the end)
  const float* srow[RS];
#pragma unroll
  for (int i = 0; i < RS; ++i)
    srow[i] = sa + static_cast<int64_t>(row0 + (i * NW + wid) * 16 + (lane >> 2)) * sa_stride;
  auto stage_scales = [&](int q) {
    char* img = lds + 2 * (TA + TB) + (q & 1) * SIMG;
    const int g = q * FB_SQ + (lane & 3);
    const int gc = g < nk ? g : nk - 1;
#pragma unroll
    for (int i = 0; i < RS; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(srow[i] + gc), (lptr_t)(img + (i * NW + wid) * 256), 4, 0, 0);
  };
  // scale_b: one value per wave and K-tile
  const float* sbw = sb + static_cast<size_t>((col0 + wc * WTN) / 128) * nk;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const auto fold = [&](f32x4& c, const f32x4& p, float s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = __builtin_fmaf(p[j], s, c[j]);
  };
  // the last FB_LAG fragments of the K-tile before and their scale; zeros fold to nothing in front of K-tile 0
  f32x4 carry[FB_LAG];
#pragma unroll
  for (int i = 0; i < FB_LAG; ++i) carry[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float scarry = 0.f;

  stage_scales(0);
  stage(0, 0);
  float sb_next = sbw[0];
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const float sbk = sb_next;
    if (kt + 1 < nk) {
      if (((kt + 1) & (FB_SQ - 1)) == 0) stage_scales((kt + 1) / FB_SQ);
      stage(kt + 1, buf ^ 1);
      sb_next = sbw[kt + 1];
    }
    const char* la = lds + buf * (TA + TB);
    const char* lb = la + TA;
    const char* img = lds + 2 * (TA + TB) + ((kt / FB_SQ) & 1) * SIMG + (kt & (FB_SQ - 1)) * 4;
    frag bfr[NR][2];
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        bfr[n][c] = *reinterpret_cast<const frag*>(lb + swz(wc * WTN + n * 16 + fr, c * 4 + fq));
    float s[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
      s[m] = *reinterpret_cast<const float*>(img + (wr * WTM + m * 16 + fr) * FB_SROW) * sbk;

    f32x4 p[F];
    frag af[2];
    static_for<F>([&](auto f) {
      constexpr int m = f / NR, n = f % NR;
      if constexpr (n == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
          af[c] = *reinterpret_cast<const frag*>(la + swz(wr * WTM + m * 16 + fr, c * 4 + fq));
      }
      p[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      OP::mma(p[f], bfr[n], af);  // B first: register j is column 4 fq + j, the lane's row of A is fr
      if constexpr (f < FB_LAG) {
        fold(acc[MR - 1][NR - FB_LAG + f], carry[f], scarry);
      } else {
        fold(acc[(f - FB_LAG) / NR][(f - FB_LAG) % NR], p[f - FB_LAG], s[(f - FB_LAG) / NR]);
      }
    });
#pragma unroll
    for (int i = 0; i < FB_LAG; ++i) carry[i] = p[F - FB_LAG + i];
    scarry = s[MR - 1];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < FB_LAG; ++i) fold(acc[MR - 1][NR - FB_LAG + i], carry[i], scarry);

  // Epilogue through LDS, in a region private to the wave: a WTM x 64 bf16 tile whose rows are 8 chunks of 16 B,
  // chunk c of row r at position c ^ (r & 7) (the 16 lanes of a write hold 16 rows of one column).
  char* ct = lds + wid * (WTM * WTN * 2);
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int r = m * 16 + fr, c = n * 2 + (fq >> 1);
      i32x2 v;
      v[0] = static_cast<int>(f2bf(acc[m][n][0]) | (static_cast<uint32_t>(f2bf(acc[m][n][1])) << 16));
      v[1] = static_cast<int>(f2bf(acc[m][n][2]) | (static_cast<uint32_t>(f2bf(acc[m][n][3])) << 16));
      *reinterpret_cast<i32x2*>(ct + r * (WTN * 2) + ((c ^ (r & 7)) << 4) + (fq & 1) * 8) = v;
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  uint16_t* Cw = C + static_cast<size_t>(row0 + wr * WTM) * N + col0 + wc * WTN;
#pragma unroll
  for (int i = 0; i < WTM / 8; ++i) {  // 8 rows per store instruction, 8 lanes per row
    const int r = i * 8 + (lane >> 3), c = lane & 7;
    const i32x4 v = *reinterpret_cast<const i32x4*>(ct + r * (WTN * 2) + ((c ^ (r & 7)) << 4));
    *reinterpret_cast<i32x4*>(Cw + static_cast<size_t>(r) * N + c * 8) = v;
  }
}

// ---------------------------------------------------------------------------
// The quantiser: a 16-lane team per group of 128 elements, 16 groups per workgroup.
// ---------------------------------------------------------------------------
constexpr int QB_THREADS = 256;
constexpr int QB_GROUPS = QB_THREADS / 16;

__global__ __launch_bounds__(QB_THREADS) void quant_fp8_block_kernel(const uint16_t* __restrict__ X, int64_t x_stride,
                                                                    uint8_t* __restrict__ Q, int64_t q_stride,
                                                                    float* __restrict__ S, int64_t s_stride,
                                                                    int64_t groups, int gpr) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * QB_GROUPS + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  const bool live = gid < groups;  // uniform over a team
  const int64_t row = live ? gid / gpr : 0;
  const int64_t col = (live ? gid % gpr : 0) * 128 + 8 * l;
  float x[8];
  float am = 0.f;
  if (live) {
    na_to_f32(*reinterpret_cast<const i32x4*>(X + row * x_stride + col), x);
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(x[e]));
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
  if (!live) return;
  const bool zero = am == 0.f;
  const float inv = zero ? 0.f : 448.f / am;
  if (l == 0) S[row * s_stride + col / 128] = zero ? 1.0f : am / 448.f;
  *reinterpret_cast<i32x2*>(Q + row * q_stride + col) = zero ? i32x2{0, 0} : na_to_e4m3(x, inv);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

static int fb_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

static bool fb_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bbytes && y < x + abytes;
}

// What the scales, the pointers and C's place add to launch()'s checks; nothing touches the device before both passed.
static int fb_validate(const char* who, int bm, int bn, const void* A, const void* B, const void* C, int M, int N,
                       int K, const float* sa, int64_t sa_stride, const float* sb) {
  if (!A || !B || !C || !sa || !sb) return fb_refuse(who, "A, B, C, scale_a and scale_b must not be NULL");
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) % 16)
    return fb_refuse(who, "operands must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) % 4)
    return fb_refuse(who, "scale_a and scale_b must be 4-B aligned");
  char msg[160];
  if (M <= 0 || N <= 0 || K <= 0 || M % bm || N % bn || K % 128) {
    std::snprintf(msg, sizeof(msg), "%s: need M%%%d==0, N%%%d==0, K%%128==0", who, bm, bn);
    return fail_arg(msg);
  }
  // launch()'s limit, ahead of the spans below: they are computed from K
  if (static_cast<int64_t>((bm > bn ? bm : bn) - 1) * K + (ROW_BYTES - CHUNK) > INT32_MAX) {
    std::snprintf(msg, sizeof(msg), "%s: K too large: %d rows of K elements must stay below 2^31", who,
                  bm > bn ? bm : bn);
    return fail_arg(msg);
  }
  const uint64_t m = M, n = N, k = K, g = k / 128;
  if (sa_stride < static_cast<int64_t>(g)) return fb_refuse(who, "need sa_stride >= K/128");
  const uint64_t cbytes = m * n * 2, sabytes = ((m - 1) * static_cast<uint64_t>(sa_stride) + g) * 4;
  if (fb_overlap(C, cbytes, A, m * k) || fb_overlap(C, cbytes, B, n * k) || fb_overlap(C, cbytes, sa, sabytes) ||
      fb_overlap(C, cbytes, sb, n / 128 * g * 4))
    return fb_refuse(who, "C must not overlap A, B, scale_a or scale_b");
  return 0;
}

struct Fp8BlockCfg {
  const char* name;
  int bm, bn;
  int (*launch)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                const float* sa, int64_t sa_stride, const float* sb);
};
template <int BM, int BN, int WM, int WN, int GM>
constexpr Fp8BlockCfg fb_cfg(const char* name) {
  constexpr auto kernel = &gemm_fp8_block_kernel<BM, BN, WM, WN, GM>;
  return {name, BM, BN,
          &launch<kernel, uint8_t, WM * WN * 64, fb_lds_bytes<BM, BN>(), BM, BN, 1, const float*, int64_t,
                  const float*>};
}

constexpr Fp8BlockCfg kFp8BlockCfgs[] = {
    fb_cfg<128, 128, 2, 2, 8>("128x128/4w"),
    fb_cfg<256, 128, 4, 2, 4>("256x128/8w"),
    fb_cfg<256, 256, 2, 4, 4>("256x256/8w"),
};
constexpr int kNumFp8BlockCfgs = sizeof(kFp8BlockCfgs) / sizeof(kFp8BlockCfgs[0]);
// the rows gsx_gemm_fp8_block_nt dispatches to
constexpr int kFb128 = 0, kFb256 = 2;

static const Fp8BlockCfg* fb_row(int cfg) {
  return cfg >= 0 && cfg < kNumFp8BlockCfgs ? &kFp8BlockCfgs[cfg] : nullptr;
}

static int fb_run(const char* who, void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                  const float* sa, int64_t sa_stride, const float* sb) {
  const Fp8BlockCfg& c = kFp8BlockCfgs[(M > 0 && N > 0 && M % 256 == 0 && N % 256 == 0) ? kFb256 : kFb128];
  if (int rc = fb_validate(who, c.bm, c.bn, A, B, C, M, N, K, sa, sa_stride, sb)) return rc;
  return c.launch(who, S(stream), A, B, C, M, N, K, sa, sa_stride, sb);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_gemm_fp8_block_cfg_name(int cfg) { return fb_row(cfg) ? fb_row(cfg)->name : nullptr; }

int gsx_gemm_fp8_block_cfg_tile(int cfg, int* bm, int* bn) {
  const Fp8BlockCfg* c = fb_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  return 0;
}

int gsx_gemm_fp8_block_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                     const float* scale_a, int64_t sa_stride, const float* scale_b, int cfg) {
  const char* who = "gsx_gemm_fp8_block_nt_launch_cfg";
  const Fp8BlockCfg* c = fb_row(cfg);
  if (!c) return fb_refuse(who, "unknown config");
  if (int rc = fb_validate(who, c->bm, c->bn, A, B, C, M, N, K, scale_a, sa_stride, scale_b)) return rc;
  return c->launch(who, S(stream), A, B, C, M, N, K, scale_a, sa_stride, scale_b);
}

int gsx_gemm_fp8_block_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                          const float* scale_a, int64_t sa_stride, const float* scale_b) {
  return fb_run("gsx_gemm_fp8_block_nt", stream, A, B, C, M, N, K, scale_a, sa_stride, scale_b);
}

int gsx_event_time_gemm_fp8_block(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                  const float* scale_a, int64_t sa_stride, const float* scale_b, int iters,
                                  float* ms) {
  return event_time(stream, iters, ms, [&] {
    return fb_run("gsx_gemm_fp8_block_nt", stream, A, B, C, M, N, K, scale_a, sa_stride, scale_b);
  });
}

int gsx_quant_fp8_block(void* stream, const void* X, int64_t x_stride, void* Q, int64_t q_stride, float* S_out,
                        int64_t s_stride, int R, int K) {
  const char* who = "gsx_quant_fp8_block";
  if (!X || !Q || !S_out) return fb_refuse(who, "X, Q and S must not be NULL");
  if (R < 1 || K < 128 || K % 128) return fb_refuse(who, "need R >= 1, K >= 128 and K % 128 == 0");
  if (x_stride < K || x_stride % 8) return fb_refuse(who, "need x_stride >= K and x_stride % 8 == 0");
  if (q_stride < K || q_stride % 8) return fb_refuse(who, "need q_stride >= K and q_stride % 8 == 0");
  if (s_stride < K / 128) return fb_refuse(who, "need s_stride >= K/128");
  if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Q)) % 16)
    return fb_refuse(who, "X and Q must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(S_out) % 4) return fb_refuse(who, "S must be 4-B aligned");
  const uint64_t r = R, k = K;
  const uint64_t xb = ((r - 1) * x_stride + k) * 2, qb = (r - 1) * q_stride + k, sb = ((r - 1) * s_stride + k / 128) * 4;
  if (fb_overlap(Q, qb, X, xb) || fb_overlap(S_out, sb, X, xb) || fb_overlap(S_out, sb, Q, qb))
    return fb_refuse(who, "X, Q and S must not overlap");
  const int64_t groups = static_cast<int64_t>(R) * (K / 128);
  const int64_t blocks = (groups + QB_GROUPS - 1) / QB_GROUPS;
  if (blocks > INT32_MAX) return fb_refuse(who, "R * K/128 too large for one launch");
  hipLaunchKernelGGL(quant_fp8_block_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(QB_THREADS), 0, S(stream),
                     static_cast<const uint16_t*>(X), x_stride, static_cast<uint8_t*>(Q), q_stride, S_out, s_stride,
                     groups, K / 128);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

}  // extern "C"
