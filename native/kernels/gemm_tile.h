// Device code and the host launcher shared by the GEMM translation units (gemm.hip: bf16, gemm_fp8.hip: fp8 e4m3,
// gemm_mxfp4.hip: e2m1 with e8m0 block scales).  Internal, like gsx_internal.h.
//
// A K-tile is 128 B per row whatever the operand type: 64 bf16, 128 fp8 or 256 fp4 values.  So the global -> LDS
// staging, the LDS swizzle and the ds_read_b128 pattern are the same for all; an operand kind (below) says what the
// element is and how the 16-B chunks a lane has read turn into MFMAs.  The two K-loop schedules, gemm_kernel (one
// __syncthreads per K-tile) and gemm_phased_kernel (prefetch in flight across barriers), exist once and take the kind
// as a parameter.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>

#include "gsx_internal.h"

namespace gsxgemm {

using namespace gsx;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef long i64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;

constexpr int ROW_BYTES = 128;  // one row of a K-tile
constexpr int CHUNK = 16;       // what one lane stages and reads at a time

// Operand kinds.  `elem` is the storage unit of A and B and EPU the elements one unit holds (2 for packed fp4): all
// addressing is in units, a row of K elements being K / EPU of them.  BK is the K-tile in elements, `frag` one 16-B
// chunk as the MFMA builtin wants it; MX says that the kind takes e8m0 block scales (MxScales below).  Lane (fr, fq)
// of a 16x16 fragment reads chunks fq and 4 + fq of its row; CH says how many of the two one call of mma() consumes.
// A and B take the same chunks, so the k positions of a product agree
// whatever k order the instruction gives the bytes of a lane.
struct Bf16 {  // v_mfma_f32_16x16x32_bf16: chunk fq is k 8 fq .. 8 fq + 7 of the first k-step, 4 + fq of the second
  using elem = uint16_t;
  using frag = bf16x8;
  static constexpr int EPU = 1, BK = ROW_BYTES / 2, CH = 1;
  static constexpr bool MX = false;
  static __device__ __forceinline__ void mma(f32x4& acc, const frag* a, const frag* b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  }
};
// OCP e4m3 on v_mfma_f32_16x16x128_f8f6f4: both chunks are the lane's 32-B operand, one MFMA per K-tile.  Format
// selects 0 / 0 are fp8 (e4m3) for A and B; scale arguments of 0 select the instruction's unscaled form.
struct Fp8K128 {
  using elem = uint8_t;
  using frag = i32x4;
  static constexpr int EPU = 1, BK = ROW_BYTES, CH = 2;
  static constexpr bool MX = false;
  static __device__ __forceinline__ void mma(f32x4& acc, const frag* a, const frag* b) {
    const i32x8 av = __builtin_shufflevector(a[0], a[1], 0, 1, 2, 3, 4, 5, 6, 7);
    const i32x8 bv = __builtin_shufflevector(b[0], b[1], 0, 1, 2, 3, 4, 5, 6, 7);
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 0, 0, 0, 0, 0, 0);
  }
};
// OCP e4m3 on v_mfma_f32_16x16x32_fp8_fp8 (8-B operands, the bf16 rate): each chunk feeds two MFMAs.
struct Fp8K32 {
  using elem = uint8_t;
  using frag = i64x2;
  static constexpr int EPU = 1, BK = ROW_BYTES, CH = 1;
  static constexpr bool MX = false;
  static __device__ __forceinline__ void mma(f32x4& acc, const frag* a, const frag* b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[0][0], b[0][0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[0][1], b[0][1], acc, 0, 0, 0);
  }
};
// OCP e2m1, two per byte (torch.float4_e2m1fn_x2), on the same instruction with format selects 4 / 4.  One 16-B chunk
// is 32 elements: the lane's whole operand of one MFMA and exactly one scale block, so chunk fq is block fq of the
// tile's first 128 k and chunk 4 + fq block fq of its second 128: two MFMAs per K-tile and fragment.  `sa` and `sb`
// are VGPRs of four e8m0 codes each (MxScales); SA and SB, immediates, say which byte this MFMA takes.  With e2m1
// selected the instruction reads the low four of the eight operand registers; the high four are left undefined.
// FIXED: every scale is code 127 (2^0) whatever sa and sb hold, the ablation of the scale path.
template <bool FIXED>
struct Mxfp4T {
  using elem = uint8_t;
  using frag = i32x4;
  static constexpr int EPU = 2, BK = 2 * ROW_BYTES, CH = 1;
  static constexpr bool MX = !FIXED;
  template <int SA, int SB>
  static __device__ __forceinline__ void mma(f32x4& acc, const frag* a, const frag* b, int sa, int sb) {
    const i32x8 av = __builtin_shufflevector(a[0], a[0], 0, 1, 2, 3, -1, -1, -1, -1);
    const i32x8 bv = __builtin_shufflevector(b[0], b[0], 0, 1, 2, 3, -1, -1, -1, -1);
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 4, 4, SA, sa, SB, sb);
  }
  static __device__ __forceinline__ void mma(f32x4& acc, const frag* a, const frag* b) {
    mma<0, 0>(acc, a, b, 127, 127);
  }
};
using Mxfp4 = Mxfp4T<false>;
using Mxfp4Unit = Mxfp4T<true>;

// The e8m0 block scales of an MX kind, staged through LDS next to the operand tiles.  S[rows][K / 32] is row-major,
// so the eight codes of one row and one K-tile are 8 consecutive, 8-B aligned bytes, and the LDS image of an operand
// tile's scales is [row][8 codes], 8 B per row.  mx_stage() is the writer: one global_load_lds of 4 B per lane, wave
// w fetching rows 32 w .. 32 w + 31 (lane l: row 32 w + l / 2, codes 4 (l & 1) .. + 3), which land lane-linear, that
// is in this very layout.  read() and pack() are the reader.  The MFMA takes the scale of lane (fr, fq) from a byte of
// a VGPR of that lane, and which byte is an immediate: the code of (row fr of the fragment, block fq) must sit at the
// same byte position in all 64 lanes.  So for each of its N fragments (16 rows apart) a lane reads the 8 codes of its
// row fr (one ds_read_b64, four lanes per address) and moves byte fq (first MFMA of the K-tile) and byte 4 + fq
// (second) of four fragments into bytes 0 .. 3 of one VGPR with v_perm_b32: pk[kk][g] serves MFMA kk of fragments
// 4 g .. 4 g + 3, fragment 4 g + i with byte select i.
constexpr int MX_ROW = 8;  // bytes of scales per row and K-tile
// s: the codes of the tile's row 0 (K-tile 0); ld = K / 32, the bytes of a row; img: the LDS image
__device__ __forceinline__ void mx_stage(const uint8_t* s, int ld, int kt, char* img, int wid, int lane) {
  const uint8_t* src = s + static_cast<size_t>(wid * 32 + (lane >> 1)) * ld + (kt * MX_ROW + (lane & 1) * 4);
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(img + wid * 256), 4, 0, 0);
}
template <int N>
struct MxScales {
  static_assert(N % 4 == 0, "fragments are packed by fours");
  i32x2 raw[N];
  int pk[2][N / 4];
  // row: the lane's row of fragment 0 in the image.  Read as plain vectors, like the operand fragments: through a
  // struct type (uint2) the compiler takes the read for one that may alias the staging loads in flight and puts
  // s_waitcnt vmcnt(0) in front of it.
  __device__ __forceinline__ void read(const char* img, int row) {
#pragma unroll
    for (int f = 0; f < N; ++f) raw[f] = *reinterpret_cast<const i32x2*>(img + (row + f * 16) * MX_ROW);
  }
  __device__ __forceinline__ void pack(int fq) {
    const int sel = 0x0c0c0000 | ((4 + fq) << 8) | fq;  // byte fq of both sources into bytes 0 and 1
#pragma unroll
    for (int g = 0; g < N / 4; ++g) {
      const i32x2* r = raw + g * 4;
      pk[0][g] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(r[3].x, r[2].x, sel),
                                       __builtin_amdgcn_perm(r[1].x, r[0].x, sel), 0x05040100);
      pk[1][g] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(r[3].y, r[2].y, sel),
                                       __builtin_amdgcn_perm(r[1].y, r[0].y, sel), 0x05040100);
    }
  }
};
struct NoScales {};

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index can be an immediate
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// The LDS swizzle, both halves.  A K-tile row is 128 B = 8 chunks of 16 B, and the LDS image of a tile is
// lane-linear: load slot p (lane p of a round of global_load_lds) lands at byte 16 p, i.e. row p >> 3, chunk
// position p & 7.  Invariant: chunk c of row r sits at position c ^ ((r >> 1) & 7).  glds_col() is the writer's half
// (slot p fetches, from whichever global row its LDS row holds, the chunk that belongs at its position), swz() the
// reader's.  The XOR is its own inverse, so both apply the same term; change one and the other must follow.
template <typename T>
__device__ __forceinline__ int glds_col(int p) {  // in units of T, from the first unit of the slot's global row
  const int row = p >> 3, slot = p & 7;
  return (slot ^ ((row >> 1) & 7)) * (CHUNK / static_cast<int>(sizeof(T)));
}
__device__ __forceinline__ uint32_t swz(int row, int chunk) {  // in bytes, from the tile's LDS base
  return static_cast<uint32_t>(row * ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4));
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

// What happens to the 16x16 accumulator fragments of a wave tile before they are converted to bf16.  (row0, col0)
// is the wave tile's origin in C.
struct Unscaled {
  template <int MR, int NR>
  __device__ __forceinline__ void operator()(f32x4 (&)[MR][NR], int, int, int, int) const {}
};
// c = (acc * sa[row]) * sb[col]: two fp32 multiplies in this order.  `stride` is 1 for one scale per row of A and
// of B, 0 for one per tensor (every lane reads element 0); sa == nullptr leaves the accumulator alone.
struct Scaled {
  const float* sa;
  const float* sb;
  int stride;
  template <int MR, int NR>
  __device__ __forceinline__ void operator()(f32x4 (&acc)[MR][NR], int row0, int col0, int fr, int fq) const {
    if (sa == nullptr) return;
    float b[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) b[n] = sb[static_cast<size_t>(col0 + n * 16 + fr) * stride];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = sa[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * stride];
#pragma unroll
        for (int n = 0; n < NR; ++n) acc[m][n][j] = (acc[m][n][j] * a) * b[n];
      }
  }
};

// The kernels take Scaled's members as arguments after K, or nothing there.
template <typename... EP>
using epilogue_t = std::conditional_t<sizeof...(EP) == 0, Unscaled, Scaled>;
// An MX kind's kernels take scale_a and scale_b (e8m0 codes, [rows][K / 32]) there instead and have no epilogue.
struct MxArgs {
  const uint8_t* sa;
  const uint8_t* sb;
};
template <class OP, typename... EP>
using kernel_epilogue_t = std::conditional_t<OP::MX, Unscaled, epilogue_t<EP...>>;
template <class S, bool TAKES, typename... EP>
__device__ __forceinline__ S from_args(EP... ep) {
  if constexpr (TAKES) {
    return S{ep...};
  } else {
    return S{};
  }
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

// ---------------------------------------------------------------------------
// One __syncthreads per K-tile: BM x BN block tile, WM x WN waves, two LDS buffers (tile k+1 in flight while the
// MFMAs consume tile k).
// ---------------------------------------------------------------------------
template <class OP, int BM, int BN, int WM, int WN, int GROUP_M, typename... EP>
__global__ __launch_bounds__(WM * WN * 64) void gemm_kernel(const typename OP::elem* __restrict__ A,
                                                           const typename OP::elem* __restrict__ B,
                                                           uint16_t* __restrict__ C, int M, int N, int K, EP... ep) {
  const auto epi = from_args<kernel_epilogue_t<OP, EP...>, !OP::MX>(ep...);
  using T = typename OP::elem;
  using frag = typename OP::frag;
  constexpr int BK = OP::BK, CH = OP::CH;
  constexpr int BKU = BK / OP::EPU;  // a K-tile and a row of K elements in units of T
  const int ld = K / OP::EPU;
  constexpr int NW = WM * WN;
  constexpr int TA = BM * ROW_BYTES, TB = BN * ROW_BYTES;  // bytes per operand tile
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
    off[i] = (p >> 3) * ld + glds_col<T>(p);
  }
  const T* Ab = A + static_cast<size_t>(row0) * ld;
  const T* Bb = B + static_cast<size_t>(col0) * ld;

  auto stage = [&](int kt, int buf) {
    char* la = lds + buf * (TA + TB);
    char* lb = la + TA;
#pragma unroll
    for (int i = 0; i < RA; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Ab + off[i] + kt * BKU), (lptr_t)(la + (i * NW + wid) * 1024), 16,
                                       0, 0);
#pragma unroll
    for (int i = 0; i < RB; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(Bb + off[i] + kt * BKU), (lptr_t)(lb + (i * NW + wid) * 1024), 16,
                                       0, 0);
  };

  f32x4 acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  // MX: the scales of a K-tile are staged with its operands, into images behind the operand buffers
  constexpr bool MX = OP::MX;
  static_assert(!MX || (MR == 4 && NR == 4 && BM == NW * 32 && BN == NW * 32),
                "the scale path packs four fragments and stages 32 rows per wave");
  constexpr int SCALES = 2 * (TA + TB);  // [buf][A|B] images of BM and BN rows
  [[maybe_unused]] std::conditional_t<MX, MxScales<4>, NoScales> sca, scb;
  [[maybe_unused]] const auto stage_scales = [&](int kt, int buf) {
    if constexpr (MX) {
      const auto mx = from_args<MxArgs, MX>(ep...);
      char* img = lds + SCALES + buf * (BM + BN) * MX_ROW;
      mx_stage(mx.sa + static_cast<size_t>(row0) * (K / 32), K / 32, kt, img, wid, lane);
      mx_stage(mx.sb + static_cast<size_t>(col0) * (K / 32), K / 32, kt, img + BM * MX_ROW, wid, lane);
    }
  };
  stage_scales(0, 0);
  stage(0, 0);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if constexpr (MX) {
      const char* img = lds + SCALES + buf * (BM + BN) * MX_ROW;
      sca.read(img, wr * WTM + fr);
      scb.read(img + BM * MX_ROW, wc * WTN + fr);
      sca.pack(fq);
      scb.pack(fq);
      if (kt + 1 < nk) stage_scales(kt + 1, buf ^ 1);
    }
    if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
    const char* la = lds + buf * (TA + TB);
    const char* lb = la + TA;
#pragma unroll
    for (int kk = 0; kk < 2 / CH; ++kk) {
      frag bfr[NR][CH];
#pragma unroll
      for (int n = 0; n < NR; ++n)
#pragma unroll
        for (int c = 0; c < CH; ++c)
          bfr[n][c] = *reinterpret_cast<const frag*>(lb + swz(wc * WTN + n * 16 + fr, (kk * CH + c) * 4 + fq));
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        frag af[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c)
          af[c] = *reinterpret_cast<const frag*>(la + swz(wr * WTM + m * 16 + fr, (kk * CH + c) * 4 + fq));
        __builtin_amdgcn_s_setprio(1);
        if constexpr (MX) {
          static_for<NR>([&](auto n) {
            static_for<4>([&](auto sel) {  // m as an immediate
              if (sel == m) OP::template mma<sel, n>(acc[m][n], af, bfr[n], sca.pk[kk][0], scb.pk[kk][0]);
            });
          });
        } else {
#pragma unroll
          for (int n = 0; n < NR; ++n) OP::mma(acc[m][n], af, bfr[n]);
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
  }
  epi(acc, row0 + wr * WTM, col0 + wc * WTN, fr, fq);
  uint16_t* ct = reinterpret_cast<uint16_t*>(lds + wid * (WTM * WTN * 2));
  scatter16<WTN>(ct, acc, fr, fq);
  store_wave_tile<WTM, WTN>(ct, C, N, row0 + wr * WTM, col0, wc * WTN, lane);
}

// ---------------------------------------------------------------------------
// Phased 256x256 schedule: the prefetch stays in flight across barriers.
//
// gemm_kernel ends every K-tile with __syncthreads(), which hipcc lowers
// to `s_waitcnt vmcnt(0); s_barrier`: the next tile's loads are drained every
// K-tile, and at one 512-thread block per CU nothing hides that.  Here a K-tile
// is four phases; each phase MFMAs one quadrant of the wave's 128x64 C tile
// (16 bf16 MFMAs) and issues one *half-tile* (16 KiB: 128 rows x 128 B of A or B)
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
//
// An MX kind adds the block scales (MxScales): per K-tile an image of A's and one of B's, 2 KiB each, behind the
// operand buffers, [tile & 1][A|B]; staging both is "half S", two global_load_lds per wave.  They are vector-memory
// loads like the other stages, counted by the same vmcnt and completing in issue order, so where they are issued
// decides what a count means.  Half S travels with half 0, issued just before it:
//   p0: read S (8 + 4 ds_read_b64), A0, B2; stage t+1 half 3; vmcnt(10): half 3 of t has landed, in flight at most
//       t half 1 | t+1 halves S, 0, 2, 3; after the barrier S is packed into 6 registers
//   p1: stage t+1 half 1; vmcnt(10): half 1 of t has landed, in flight t+1 halves S, 0, 2, 3, 1
//   p2: stage t+2 halves S, 0; no wait
//   p3: stage t+2 half 2; vmcnt(10): t+1 halves S, 0, 2 have landed, in flight t+1 halves 3, 1 | t+2 halves S, 0, 2
// So every count is the old 8 plus the 2 loads of one half S, and the same four operand half-tiles stay in flight.
// Half S is read in p0 and restaged in p2 like half 0 (WAR), and p3's wait and barrier come before its first read in
// the next p0 (RAW).  A tile past the end is clamped for the scales as for the operands, so the loads stay inside
// the scale arrays.
// ---------------------------------------------------------------------------
constexpr int PH_HALF = 128 * ROW_BYTES;  // 16 KiB

__device__ __forceinline__ void ph_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// M32 (bf16 only): the same schedule on v_mfma_f32_32x32x16_bf16 (per quadrant 2 x 1 blocks of 32x32 over 4 k-steps:
// 8 MFMAs of twice the work instead of 16), for the A/B the MFMA-shape rule asks for (the chip may hold a different
// clock on the other shape; same LDS bytes, same registers).
template <class OP, int GROUP_M, bool M32, typename... EP>
__global__ __launch_bounds__(512) void gemm_phased_kernel(const typename OP::elem* __restrict__ A,
                                                         const typename OP::elem* __restrict__ B,
                                                         uint16_t* __restrict__ C, int M, int N, int K, EP... ep) {
  const auto epi = from_args<kernel_epilogue_t<OP, EP...>, !OP::MX>(ep...);
  using T = typename OP::elem;
  using frag = typename OP::frag;
  static_assert(!M32 || std::is_same_v<OP, Bf16>, "the 32x32 shape is a bf16 ablation");
  constexpr int BK = OP::BK, CH = OP::CH;
  constexpr int BKU = BK / OP::EPU;  // a K-tile and a row of K elements in units of T
  const int ld = K / OP::EPU;
  constexpr bool MX = OP::MX;
  constexpr int VM = 8 + (MX ? 2 : 0);  // the vmcnt of the phases: four half-tiles, and one half S
  constexpr int BM = 256, BN = 256, WTM = 128, WTN = 64;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;

  int tm, tn;
  tile_of<BM, BN, GROUP_M>(blockIdx.x, gridDim.x, M, N, tm, tn);
  const T* Ab = A + static_cast<size_t>(tm * BM) * ld;
  const T* Bb = B + static_cast<size_t>(tn * BN) * ld;

  // per-lane source offsets of the two 8-KiB rounds of each half
  int off[4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = (i * 8 + wid) * 64 + lane;
    const int lr = p >> 3;
    const int sw = glds_col<T>(p);
    off[0][i] = ((lr >> 6) * 128 + (lr & 63)) * ld + sw;
    off[1][i] = ((lr >> 6) * 128 + 64 + (lr & 63)) * ld + sw;
    off[2][i] = ((lr >> 5) * 64 + (lr & 31)) * ld + sw;
    off[3][i] = ((lr >> 5) * 64 + 32 + (lr & 31)) * ld + sw;
  }
  const int nk = K / BK;
  auto stage = [&](int tile, int half) {
    const int kt = tile < nk ? tile : nk - 1;
    const T* src = (half < 2 ? Ab : Bb) + kt * BKU;
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
  frag af[4][2], bf[2][2][2];  // A: [m][chunk]; B: [nh][n][chunk]  (M32: A [b][kk], B [nh][kk], k-steps of 16)

  // MX: sca.pk[kk][mh] holds the scales of A fragments 4 mh .. 4 mh + 3, scb.pk[kk][0] those of the 4 B fragments
  [[maybe_unused]] std::conditional_t<MX, MxScales<8>, NoScales> sca;
  [[maybe_unused]] std::conditional_t<MX, MxScales<4>, NoScales> scb;
  [[maybe_unused]] const auto stage_scales = [&](int tile) {
    if constexpr (MX) {
      const auto mx = from_args<MxArgs, MX>(ep...);
      const int kt = tile < nk ? tile : nk - 1;
      char* img = lds + 8 * PH_HALF + (tile & 1) * (BM + BN) * MX_ROW;
      mx_stage(mx.sa + static_cast<size_t>(tm * BM) * (K / 32), K / 32, kt, img, wid, lane);
      mx_stage(mx.sb + static_cast<size_t>(tn * BN) * (K / 32), K / 32, kt, img + BM * MX_ROW, wid, lane);
    }
  };

  auto read_a = [&](const char* base, int mh) {
    const char* h = base + mh * PH_HALF;
    if constexpr (M32) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          af[b * 2 + (kk >> 1)][kk & 1] =
              *reinterpret_cast<const frag*>(h + swz(wr * 64 + b * 32 + r32, kk * 2 + h32));
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          af[m][kk] = *reinterpret_cast<const frag*>(h + swz(wr * 64 + m * 16 + fr, kk * 4 + fq));
    }
  };
  auto read_b = [&](const char* base, int nh) {
    const char* h = base + (2 + nh) * PH_HALF;
    if constexpr (M32) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        bf[nh][kk >> 1][kk & 1] = *reinterpret_cast<const frag*>(h + swz(wc * 32 + r32, kk * 2 + h32));
    } else {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          bf[nh][n][kk] = *reinterpret_cast<const frag*>(h + swz(wc * 32 + n * 16 + fr, kk * 4 + fq));
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
      for (int kk = 0; kk < 2 / CH; ++kk) {
        if constexpr (MX) {
          static_for<4>([&](auto m) {
            static_for<4>([&](auto nn) {  // nh * 2 + n as an immediate
              if (nn >> 1 == nh)
                OP::template mma<m, nn>(acc[mh * 4 + m][nn], &af[m][kk], &bf[nn >> 1][nn & 1][kk], sca.pk[kk][mh],
                                        scb.pk[kk][0]);
            });
          });
        } else {
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
              OP::mma(acc[mh * 4 + m][nh * 2 + n], &af[m][kk * CH], &bf[nh][n][kk * CH]);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: what the steady state has issued before tile 0, phase 0
  stage_scales(0);
  stage(0, 0);
  stage(0, 2);
  stage(0, 3);
  stage(0, 1);
  stage_scales(1);
  stage(1, 0);
  stage(1, 2);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
  ph_barrier();
  if (wr == 1) ph_barrier();  // stagger the groups by one barrier

  for (int t = 0; t < nk; ++t) {
    const char* base = lds + (t & 1) * 4 * PH_HALF;
    // p0
    if constexpr (MX) {
      const char* img = lds + 8 * PH_HALF + (t & 1) * (BM + BN) * MX_ROW;
      sca.read(img, wr * WTM + fr);
      scb.read(img + BM * MX_ROW, wc * WTN + fr);
    }
    read_a(base, 0);
    read_b(base, 0);
    stage(t + 1, 3);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
    ph_barrier();
    if constexpr (MX) {  // after the barrier: the reads' latency passes while the wave waits there
      sca.pack(fq);
      scb.pack(fq);
    }
    mma(0, 0);
    ph_barrier();
    // p1
    read_b(base, 1);
    stage(t + 1, 1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
    ph_barrier();
    mma(0, 1);
    ph_barrier();
    // p2
    read_a(base, 1);
    stage_scales(t + 2);
    stage(t + 2, 0);
    ph_barrier();
    mma(1, 1);
    ph_barrier();
    // p3
    stage(t + 2, 2);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
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
    epi(acc, tm * BM + wr * WTM, tn * BN + wc * WTN, fr, fq);
    scatter16<WTN>(ct, acc, fr, fq);
  }
  store_wave_tile<WTM, WTN>(ct, C, N, tm * BM + wr * WTM, tn * BN + wc * WTN, 0, lane);
}

// ---------------------------------------------------------------------------
// Host side: one launcher.
// ---------------------------------------------------------------------------

// Validates once for every kernel, then launches; a failure's text begins with `who`, the C entry point.  T is the
// operands' storage unit and EPU the elements in one (the kind's); `extra` are the kernel's arguments after K.
template <auto KERNEL, typename T, int THREADS, int LDS, int BM, int BN, int EPU = 1, typename... Extra>
int launch(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
           Extra... extra) {
  constexpr int BKU = ROW_BYTES / sizeof(T), BK = BKU * EPU;  // a K-tile in units and in elements
  char msg[160];
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK) {
    std::snprintf(msg, sizeof(msg), "%s: need M%%%d==0, N%%%d==0, K%%%d==0", who, BM, BN, BK);
    return fail_arg(msg);
  }
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) % 16) {
    std::snprintf(msg, sizeof(msg), "%s: operands must be 16-B aligned", who);
    return fail_arg(msg);
  }
  // The kernels keep a lane's source offset inside an operand tile in an int, in units: row * (K / EPU) + column,
  // with row < max(BM, BN) and column <= a K-tile minus one 16-B chunk (off[] of the kernels).  Everything else that
  // grows with the problem is added to the pointer in 64 bits.
  constexpr int SIDE = BM > BN ? BM : BN;
  if (static_cast<int64_t>(SIDE - 1) * (K / EPU) + (BKU - CHUNK / static_cast<int>(sizeof(T))) > INT32_MAX) {
    std::snprintf(msg, sizeof(msg), "%s: K too large: %d rows of K elements%s must stay below 2^31", who, SIDE,
                  EPU == 1 ? "" : ", packed two to the byte,");
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
  hipLaunchKernelGGL(KERNEL, dim3((M / BM) * (N / BN)), dim3(THREADS), LDS, s, static_cast<const T*>(A),
                     static_cast<const T*>(B), static_cast<uint16_t*>(C), M, N, K, extra...);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

// elapsed milliseconds of `iters` calls of `step` (each launches on `stream`), by hip events
template <class STEP>
int event_time(void* stream, int iters, float* ms, STEP step) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto timed = [&]() -> int {
    GSX_CHECK(hipEventCreate(&e0));
    GSX_CHECK(hipEventCreate(&e1));
    GSX_CHECK(hipEventRecord(e0, S(stream)));
    for (int i = 0; i < iters; ++i) {
      if (int rc = step()) return rc;
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

}  // namespace gsxgemm
