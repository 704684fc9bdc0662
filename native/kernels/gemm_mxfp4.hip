// MXFP4 MFMA GEMM family for the pod workload, and the quantiser that makes its operands.  C ABI and the operand
// format in gsx_kernels.h.
//
//   C[M][N] (bf16) = sum over blocks g of 32 k: 2^(sa[i][g] - 127) 2^(sb[j][g] - 127) sum_k A[i][k] B[j][k]
//
// A and B are OCP e2m1, two per byte; sa and sb are e8m0 codes, one per row and block, row-major.  The schedules, the
// tile map, the swizzle and the store of C are gemm_tile.h's, the ones the bf16 and fp8 families run: a row of a
// K-tile is 128 B there and here (256 fp4), so staging and LDS reads are the same instructions.  What differs is the
// MFMA burst (v_mfma_scale_f32_16x16x128_f8f6f4 with format selects 4 / 4: two per K-tile and fragment) and the
// path of the block scales into it, which is gemm_tile.h's MxScales: staged through LDS next to the operand tiles,
// in the plain layout, and moved to the byte positions the instruction wants by the reader.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

// The scale pointers are checked here, the rest by launch(); nothing touches the device before both have passed.
// TAKES: the kernel has the scale pointers as arguments (the ablation row has not, and ignores them).
template <auto KERNEL, bool TAKES, int THREADS, int LDS, int BM, int BN>
int launch_mxfp4(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                 const void* sa, const void* sb) {
  char msg[160];
  if (!sa || !sb) {
    std::snprintf(msg, sizeof(msg), "%s: scale_a and scale_b must not be NULL", who);
    return fail_arg(msg);
  }
  if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) % 16) {
    std::snprintf(msg, sizeof(msg), "%s: scale_a and scale_b must be 16-B aligned", who);
    return fail_arg(msg);
  }
  if constexpr (TAKES) {
    return launch<KERNEL, uint8_t, THREADS, LDS, BM, BN, 2>(who, s, A, B, C, M, N, K, static_cast<const uint8_t*>(sa),
                                                            static_cast<const uint8_t*>(sb));
  } else {
    return launch<KERNEL, uint8_t, THREADS, LDS, BM, BN, 2>(who, s, A, B, C, M, N, K);
  }
}

struct Mxfp4Cfg {
  const char* name;
  int bm, bn;
  int (*launch)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                const void* sa, const void* sb);
};
template <int BM, int BN, int WM, int WN, int GM>
constexpr Mxfp4Cfg plain(const char* name) {
  constexpr auto kernel = &gemm_kernel<Mxfp4, BM, BN, WM, WN, GM, const uint8_t*, const uint8_t*>;
  return {name, BM, BN,
          &launch_mxfp4<kernel, true, WM * WN * 64, 2 * (BM + BN) * (ROW_BYTES + MX_ROW), BM, BN>};
}
template <int GM>
constexpr Mxfp4Cfg phased(const char* name) {
  constexpr auto kernel = &gemm_phased_kernel<Mxfp4, GM, false, const uint8_t*, const uint8_t*>;
  return {name, 256, 256, &launch_mxfp4<kernel, true, 512, 8 * PH_HALF + 2 * (256 + 256) * MX_ROW, 256, 256>};
}
template <int GM>
constexpr Mxfp4Cfg phased_unit(const char* name) {
  constexpr auto kernel = &gemm_phased_kernel<Mxfp4Unit, GM, false>;
  return {name, 256, 256, &launch_mxfp4<kernel, false, 512, 8 * PH_HALF, 256, 256>};
}

constexpr Mxfp4Cfg kMxfp4Cfgs[] = {
    plain<128, 128, 2, 2, 8>("128x128/4w"),
    phased<4>("256x256/8w-phased-g4"),
    phased_unit<4>("256x256/8w-phased-g4-unit"),  // ablation: every scale fixed at 127, no scale staging
};
constexpr int kNumMxfp4Cfgs = sizeof(kMxfp4Cfgs) / sizeof(kMxfp4Cfgs[0]);
// the two rows gsx_gemm_mxfp4_nt dispatches to
constexpr int kMxfp4Grouped128 = 0, kMxfp4Phased = 1;

static const Mxfp4Cfg* mxfp4_row(int cfg) { return cfg >= 0 && cfg < kNumMxfp4Cfgs ? &kMxfp4Cfgs[cfg] : nullptr; }

// ---------------------------------------------------------------------------
// The quantiser: bf16 X[R][K] -> e2m1 Q[R][K / 2] and e8m0 S[R][K / 32], OCP MX v1.0.  One thread per block of 32:
// it reads 64 B, writes 16 B and one byte.  With E the biased exponent of the block's largest magnitude the code is
// clamp(E - 2, 1, 254): floor(log2(max)) - 2 + 127, where everything at or below the lower clamp (subnormals
// included) needs no logarithm.  The elements are x * 2^(127 - code), exact in fp32 or far below the grid's first
// midpoint, rounded to nearest even onto {0, .5, 1, 1.5, 2, 3, 4, 6} by comparing with the seven midpoints: a tie goes
// to the even code, so the midpoints below odd codes count when reached and those below even codes when passed.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t e2m1_of(uint32_t bf, float inv) {
  const float a = __uint_as_float((bf & 0x7fffu) << 16) * inv;
  const uint32_t code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return code | ((bf >> 12) & 8u);
}

__global__ __launch_bounds__(256) void quant_mxfp4_kernel(const uint16_t* __restrict__ X, uint8_t* __restrict__ Q,
                                                          uint8_t* __restrict__ S, size_t blocks) {
  const size_t g = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (g >= blocks) return;
  uint4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = reinterpret_cast<const uint4*>(X + g * 32)[i];
  const uint32_t* w = reinterpret_cast<const uint32_t*>(v);  // 16 words of two bf16 each
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t lo = w[i] & 0x7fffu, hi = (w[i] >> 16) & 0x7fffu;
    mx = mx > lo ? mx : lo;
    mx = mx > hi ? mx : hi;
  }
  const int e = static_cast<int>(mx >> 7);
  int code = e - 2 < 1 ? 1 : e - 2;
  if (mx == 0) code = 127;
  if (e == 255) code = 255;  // inf or NaN in the block: the elements are unspecified
  const float inv = __uint_as_float(static_cast<uint32_t>(254 - (code == 255 ? 127 : code)) << 23);
  uint32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = w[i * 4 + j];
      r |= (e2m1_of(p & 0xffffu, inv) | (e2m1_of(p >> 16, inv) << 4)) << (8 * j);
    }
    q[i] = r;
  }
  reinterpret_cast<uint4*>(Q)[g] = uint4{q[0], q[1], q[2], q[3]};
  S[g] = static_cast<uint8_t>(code);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_gemm_mxfp4_cfg_name(int cfg) { return mxfp4_row(cfg) ? mxfp4_row(cfg)->name : nullptr; }

int gsx_gemm_mxfp4_cfg_tile(int cfg, int* bm, int* bn) {
  const Mxfp4Cfg* c = mxfp4_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  return 0;
}

int gsx_gemm_mxfp4_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                 const void* scale_a, const void* scale_b, int cfg) {
  const Mxfp4Cfg* c = mxfp4_row(cfg);
  if (!c) return fail_arg("gsx_gemm_mxfp4_nt_launch_cfg: unknown config");
  return c->launch("gsx_gemm_mxfp4_nt_launch_cfg", S(stream), A, B, C, M, N, K, scale_a, scale_b);
}

int gsx_gemm_mxfp4_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K, const void* scale_a,
                      const void* scale_b) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % 256)
    return fail_arg("gsx_gemm_mxfp4_nt: need M%128==0, N%128==0, K%256==0");
  const Mxfp4Cfg& c = kMxfp4Cfgs[(M % 256 == 0 && N % 256 == 0) ? kMxfp4Phased : kMxfp4Grouped128];
  return c.launch("gsx_gemm_mxfp4_nt", S(stream), A, B, C, M, N, K, scale_a, scale_b);
}

int gsx_event_time_gemm_mxfp4(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                              const void* scale_a, const void* scale_b, int iters, float* ms) {
  return event_time(stream, iters, ms,
                    [&] { return gsx_gemm_mxfp4_nt(stream, A, B, C, M, N, K, scale_a, scale_b); });
}

int gsx_quant_mxfp4(void* stream, const void* X, void* Q, void* S_, int R, int K) {
  if (R <= 0 || K <= 0 || K % 32) return fail_arg("gsx_quant_mxfp4: need R > 0, K > 0, K%32==0");
  if (!X || !Q || !S_) return fail_arg("gsx_quant_mxfp4: X, Q and S must not be NULL");
  if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Q)) % 16)
    return fail_arg("gsx_quant_mxfp4: X and Q must be 16-B aligned");
  const size_t blocks = static_cast<size_t>(R) * (K / 32);
  if ((blocks + 255) / 256 > static_cast<size_t>(INT32_MAX)) return fail_arg("gsx_quant_mxfp4: R * K too large");
  hipLaunchKernelGGL(quant_mxfp4_kernel, dim3(static_cast<unsigned>((blocks + 255) / 256)), dim3(256), 0, S(stream),
                     static_cast<const uint16_t*>(X), static_cast<uint8_t*>(Q), static_cast<uint8_t*>(S_), blocks);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, "gsx_quant_mxfp4");
}

}  // extern "C"
