// Fused residual add + RMSNorm, and SwiGLU, for the pod workload: the glue between the projections of a decoder layer
// (gemm_decode.hip).  Both write bf16, or OCP e4m3 with one scale per row, which is the A / scale_a the fp8 decode
// GEMM takes with GSX_GEMM_SCALE_ROW.  With a few rows they are a decode step's launches, with thousands a prefill
// chunk's, where they are bound by HBM bandwidth.  C ABI and numeric contract in gsx_kernels.h.
//
// A row is cut into chunks of 16 B = 8 bf16.  In the row kernels a workgroup of 256 threads owns one row and thread t
// owns chunks t, t + 256, ..: U of them, U a template parameter picked from the row length, all held in registers,
// so the row is read from memory once.  The loads of a thread's chunks are issued before the first is used.
//   * add_rmsnorm_kernel: h = bf16(x + r) (a raw copy of x without R_in), R_out = h, then the sum of squares in a
//     fixed order: a thread adds the 8 squares of a chunk in order, its chunks in order (n_chain = 8 U); a wave
//     combines by xor shuffles over 32, 16, .., 1 (6 levels); the four waves' sums s0..s3 go through LDS and every
//     thread forms (s0 + s1) + (s2 + s3) (2 levels).  The square of a bf16 value is exact in fp32, so an FMA gives
//     what multiply and add give.  The mean, the square root and the reciprocal are one correctly rounded operation
//     each; y32 = (h * rinv) * w.
//   * silu_mul_row_kernel (e4m3 output): y32 of the whole row in registers, in groups of 4 chunks whose loads are in
//     flight together.
//   * silu_mul_kernel (bf16 output): no row reduction, so a 2-D grid of rows by runs of 512 chunks.
//   * silu: e = v_exp_f32(fl(g * -log2 e)), y32 = fl(fl(g * v_rcp_f32(fl(1 + e))) * u).
//   * e4m3: amax over the row by the same shuffle-and-LDS tree (a max does not depend on order), scale = amax / 448,
//     and fl(y32 * fl(448 / amax)) is clamped to +-448 (v_med3_f32; a NaN stays a NaN) in front of v_cvt_pk_fp8_f32,
//     the idiom of kv_append.hip.
// No atomics and nothing between workgroups; row offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int NA_THREADS = 256;
constexpr int NA_WAVES = NA_THREADS / 64;
constexpr int NORM_MAX_H = 16384;        // 8 chunks a thread
constexpr int SILU_MAX_ROW_I = 32768;    // 16 chunks a thread
constexpr int SILU_GRID_U = 2;           // chunks a thread of the bf16 SwiGLU takes
constexpr int SILU_MAX_GRID_ROWS = 65535;

// 8 bf16 (one 16-B chunk) as fp32: exact
__device__ __forceinline__ void na_to_f32(const i32x4& v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(static_cast<uint32_t>(v[i]) << 16);
    f[2 * i + 1] = __uint_as_float(static_cast<uint32_t>(v[i]) & 0xffff0000u);
  }
}

// 8 fp32 as 8 bf16, round to nearest even
__device__ __forceinline__ i32x4 na_to_bf16(const float* f) {
  i32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] = static_cast<int>(f2bf(f[2 * i]) | (static_cast<uint32_t>(f2bf(f[2 * i + 1])) << 16));
  return v;
}

// fl(x * inv) onto OCP e4m3fn, round to nearest even, saturating; a NaN passes the clamp and becomes a NaN code
__device__ __forceinline__ float na_e4m3_clamp(float x, float inv) {
  const float y = x * inv;
  const float c = __builtin_amdgcn_fmed3f(y, -448.f, 448.f);
  return y != y ? y : c;
}
__device__ __forceinline__ i32x2 na_to_e4m3(const float* f, float inv) {
  i32x2 v;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(na_e4m3_clamp(f[4 * i], inv), na_e4m3_clamp(f[4 * i + 1], inv), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(na_e4m3_clamp(f[4 * i + 2], inv), na_e4m3_clamp(f[4 * i + 3], inv), w, true);
    v[i] = w;
  }
  return v;
}

// The fixed tree over the workgroup: xor shuffles over 32 .. 1 inside a wave, then (s0 + s1) + (s2 + s3) of the four
// waves' results through `lds` (NA_WAVES floats of its own per reduction).  Every thread gets the same value.
template <bool MAX>
__device__ __forceinline__ float na_block_reduce(float v, float* lds) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float t = __shfl_xor(v, o);
    v = MAX ? fmaxf(v, t) : v + t;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const float a = lds[0], b = lds[1], c = lds[2], d = lds[3];
  return MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
}

// A row's y32, U chunks a thread, to Y: rounded to bf16, or quantised with the row's own scale.
template <int U, bool FP8>
__device__ __forceinline__ void na_store_row(const float (&y)[U][8], int nchunks, void* yrow, float* scale_slot,
                                             float* lds) {
  const int t = threadIdx.x;
  if constexpr (!FP8) {
    static_for<U>([&](auto u) {
      const int c = t + NA_THREADS * u;
      if (c < nchunks) *reinterpret_cast<i32x4*>(static_cast<uint16_t*>(yrow) + 8 * c) = na_to_bf16(y[u]);
    });
  } else {
    float am = 0.f;
    static_for<U>([&](auto u) {
      if (t + NA_THREADS * u < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(y[u][e]));
      }
    });
    am = na_block_reduce<true>(am, lds);
    const bool zero = am == 0.f;  // uniform over the workgroup
    const float inv = zero ? 0.f : 448.f / am;
    if (t == 0) *scale_slot = zero ? 1.0f : am / 448.f;
    static_for<U>([&](auto u) {
      const int c = t + NA_THREADS * u;
      if (c < nchunks)
        *reinterpret_cast<i32x2*>(static_cast<uint8_t*>(yrow) + 8 * c) = zero ? i32x2{0, 0} : na_to_e4m3(y[u], inv);
    });
  }
}

template <int U, bool FP8>
__global__ __launch_bounds__(NA_THREADS) void add_rmsnorm_kernel(
    const uint16_t* __restrict__ X, int64_t x_stride, const uint16_t* R_in, uint16_t* R_out, int64_t r_stride,
    const uint16_t* __restrict__ W, void* __restrict__ Y, int64_t y_stride, float* __restrict__ scale_out, int H,
    float eps) {
  __shared__ float lds[2][NA_WAVES];
  const int64_t m = blockIdx.x;
  const int t = threadIdx.x;
  const int nchunks = H >> 3;
  const uint16_t* const xrow = X + m * x_stride;
  const uint16_t* const rrow = R_in ? R_in + m * r_stride : nullptr;
  i32x4 xv[U], rv[U], wv[U];
  static_for<U>([&](auto u) {
    const int c = t + NA_THREADS * u;
    if (c < nchunks) {
      xv[u] = *reinterpret_cast<const i32x4*>(xrow + 8 * c);
      if (rrow) rv[u] = *reinterpret_cast<const i32x4*>(rrow + 8 * c);
      wv[u] = *reinterpret_cast<const i32x4*>(W + 8 * c);
    }
  });
  float h[U][8];
  float ss = 0.f;
  static_for<U>([&](auto u) {
    const int c = t + NA_THREADS * u;
    if (c >= nchunks) return;
    i32x4 hv = xv[u];
    na_to_f32(xv[u], h[u]);
    if (rrow) {
      float r[8];
      na_to_f32(rv[u], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) h[u][e] += r[e];
      hv = na_to_bf16(h[u]);
      na_to_f32(hv, h[u]);
    }
    if (R_out) *reinterpret_cast<i32x4*>(R_out + m * r_stride + 8 * c) = hv;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += h[u][e] * h[u][e];
  });
  ss = na_block_reduce<false>(ss, lds[0]);
  const float rinv = 1.0f / sqrtf(ss / static_cast<float>(H) + eps);
  static_for<U>([&](auto u) {
    if (t + NA_THREADS * u >= nchunks) return;
    float w[8];
    na_to_f32(wv[u], w);
#pragma unroll
    for (int e = 0; e < 8; ++e) h[u][e] = (h[u][e] * rinv) * w[e];
  });
  const int64_t yoff = m * y_stride;
  na_store_row<U, FP8>(h, nchunks,
                       FP8 ? static_cast<void*>(static_cast<uint8_t*>(Y) + yoff)
                           : static_cast<void*>(static_cast<uint16_t*>(Y) + yoff),
                       FP8 ? scale_out + m : nullptr, lds[1]);
}

// silu(g) * u: v_exp_f32 of fl(g * -log2 e), v_rcp_f32 of fl(1 + e), two multiplies
__device__ __forceinline__ float na_silu_mul(float g, float u) {
  const float e = __builtin_amdgcn_exp2f(g * -1.44269504088896341f);
  return (g * __builtin_amdgcn_rcpf(1.0f + e)) * u;
}

__device__ __forceinline__ void na_silu_mul8(const i32x4& gv, const i32x4& uv, float* y) {
  float g[8], u[8];
  na_to_f32(gv, g);
  na_to_f32(uv, u);
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = na_silu_mul(g[e], u[e]);
}

template <int U>
__global__ __launch_bounds__(NA_THREADS) void silu_mul_row_kernel(const uint16_t* __restrict__ GU, int64_t gu_stride,
                                                                  uint8_t* __restrict__ Y, int64_t y_stride,
                                                                  float* __restrict__ scale_out, int I) {
  constexpr int G = U < 4 ? U : 4;  // chunks of gate and of up whose loads are in flight together
  __shared__ float lds[NA_WAVES];
  const int64_t m = blockIdx.x;
  const int t = threadIdx.x;
  const int nchunks = I >> 3;
  const uint16_t* const grow = GU + m * gu_stride;
  const uint16_t* const urow = grow + I;
  float y[U][8];
  static_for<U / G>([&](auto q) {
    i32x4 gv[G], uv[G];
    static_for<G>([&](auto j) {
      const int c = t + NA_THREADS * (q * G + j);
      if (c < nchunks) {
        gv[j] = *reinterpret_cast<const i32x4*>(grow + 8 * c);
        uv[j] = *reinterpret_cast<const i32x4*>(urow + 8 * c);
      }
    });
    static_for<G>([&](auto j) {
      if (t + NA_THREADS * (q * G + j) < nchunks) na_silu_mul8(gv[j], uv[j], y[q * G + j]);
    });
  });
  na_store_row<U, true>(y, nchunks, Y + m * y_stride, scale_out + m, lds);
}

__global__ __launch_bounds__(NA_THREADS) void silu_mul_kernel(const uint16_t* __restrict__ GU, int64_t gu_stride,
                                                              uint16_t* __restrict__ Y, int64_t y_stride, int M,
                                                              int I) {
  const int nchunks = I >> 3;
  const int c0 = blockIdx.x * (NA_THREADS * SILU_GRID_U) + threadIdx.x;
  for (int64_t m = blockIdx.y; m < M; m += gridDim.y) {
    const uint16_t* const grow = GU + m * gu_stride;
    const uint16_t* const urow = grow + I;
    i32x4 gv[SILU_GRID_U], uv[SILU_GRID_U];
    static_for<SILU_GRID_U>([&](auto j) {
      const int c = c0 + NA_THREADS * j;
      if (c < nchunks) {
        gv[j] = *reinterpret_cast<const i32x4*>(grow + 8 * static_cast<int64_t>(c));
        uv[j] = *reinterpret_cast<const i32x4*>(urow + 8 * static_cast<int64_t>(c));
      }
    });
    static_for<SILU_GRID_U>([&](auto j) {
      const int c = c0 + NA_THREADS * j;
      if (c >= nchunks) return;
      float y[8];
      na_silu_mul8(gv[j], uv[j], y);
      *reinterpret_cast<i32x4*>(Y + m * y_stride + 8 * static_cast<int64_t>(c)) = na_to_bf16(y);
    });
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct NaSpan {  // [p, p + bytes); p == nullptr: nothing
  const void* p;
  uint64_t bytes;
};

static NaSpan na_rows(const void* p, int M, int64_t stride, int64_t row, int esize) {
  return {p, p ? (static_cast<uint64_t>(M - 1) * static_cast<uint64_t>(stride) + static_cast<uint64_t>(row)) * esize
               : 0};
}

static bool na_overlap(const NaSpan& a, const NaSpan& b) {
  if (!a.p || !b.p) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

static int na_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

// What both entry points refuse about the output kind, M and scale_out.
static int na_validate_out(const char* who, int out_kind, int M, const void* Y, const float* scale_out) {
  if (out_kind != GSX_ACT_OUT_BF16 && out_kind != GSX_ACT_OUT_FP8_ROW) {
    char msg[96];
    std::snprintf(msg, sizeof(msg), "%s: unknown out_kind %d", who, out_kind);
    return fail_arg(msg);
  }
  if (M < 1) return na_refuse(who, "need M >= 1");
  if ((out_kind == GSX_ACT_OUT_BF16) != (scale_out == nullptr))
    return na_refuse(who, "scale_out must be NULL with GSX_ACT_OUT_BF16 and non-NULL with GSX_ACT_OUT_FP8_ROW");
  return 0;
}

struct NormArgs {
  int out_kind;
  const void* X;
  int64_t x_stride;
  const void* R_in;
  void* R_out;
  int64_t r_stride;
  const void* W;
  void* Y;
  int64_t y_stride;
  float* scale_out;
  int M, H;
  float eps;
};

static int norm_validate(const char* who, const NormArgs& a) {
  if (int rc = na_validate_out(who, a.out_kind, a.M, a.Y, a.scale_out)) return rc;
  if (a.H < 8 || a.H > NORM_MAX_H || a.H % 8) return na_refuse(who, "need 8 <= H <= 16384 and H % 8 == 0");
  if (a.x_stride < a.H || a.x_stride % 8) return na_refuse(who, "need x_stride >= H and x_stride % 8 == 0");
  if ((a.R_in || a.R_out) && (a.r_stride < a.H || a.r_stride % 8))
    return na_refuse(who, "need r_stride >= H and r_stride % 8 == 0");
  if (a.y_stride < a.H || a.y_stride % 8) return na_refuse(who, "need y_stride >= H and y_stride % 8 == 0");
  if (!a.X || !a.W || !a.Y) return na_refuse(who, "X, W and Y must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.R_in) | reinterpret_cast<uintptr_t>(a.R_out) |
       reinterpret_cast<uintptr_t>(a.W) | reinterpret_cast<uintptr_t>(a.Y)) % 16)
    return na_refuse(who, "X, R_in, R_out, W and Y must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(a.scale_out) % 4) return na_refuse(who, "scale_out must be 4-B aligned");
  const bool fp8 = a.out_kind == GSX_ACT_OUT_FP8_ROW;
  const NaSpan x = na_rows(a.X, a.M, a.x_stride, a.H, 2), ri = na_rows(a.R_in, a.M, a.r_stride, a.H, 2),
             ro = na_rows(a.R_out, a.M, a.r_stride, a.H, 2), w = na_rows(a.W, 1, 0, a.H, 2),
             y = na_rows(a.Y, a.M, a.y_stride, a.H, fp8 ? 1 : 2), sc = na_rows(a.scale_out, 1, 0, a.M, 4);
  if (na_overlap(y, x) || na_overlap(y, ri) || na_overlap(y, w)) return na_refuse(who, "Y must not overlap X, R_in or W");
  if (na_overlap(ro, x) || na_overlap(ro, w) || na_overlap(ro, y) || na_overlap(ro, sc) ||
      (a.R_out != a.R_in && na_overlap(ro, ri)))
    return na_refuse(who, "R_out must not overlap X, W, Y or scale_out, nor R_in unless it is R_in");
  if (na_overlap(sc, x) || na_overlap(sc, ri) || na_overlap(sc, w) || na_overlap(sc, y))
    return na_refuse(who, "scale_out must not overlap X, R_in, W or Y");
  if (!std::isfinite(a.eps) || !(a.eps >= 0.f)) return na_refuse(who, "eps must be finite and >= 0");
  return 0;
}

template <int U, bool FP8>
static void norm_launch_u(hipStream_t s, const NormArgs& a) {
  hipLaunchKernelGGL((add_rmsnorm_kernel<U, FP8>), dim3(a.M), dim3(NA_THREADS), 0, s,
                     static_cast<const uint16_t*>(a.X), a.x_stride, static_cast<const uint16_t*>(a.R_in),
                     static_cast<uint16_t*>(a.R_out), a.r_stride, static_cast<const uint16_t*>(a.W), a.Y, a.y_stride,
                     a.scale_out, a.H, a.eps);
}

// chunks a thread holds: the power of two that covers the row
static int na_pick_u(int nchunks) {
  int u = 1;
  while (u * NA_THREADS < nchunks) u *= 2;
  return u;
}

template <bool FP8>
static int norm_launch(const char* who, hipStream_t s, const NormArgs& a) {
  switch (na_pick_u(a.H / 8)) {
    case 1: norm_launch_u<1, FP8>(s, a); break;
    case 2: norm_launch_u<2, FP8>(s, a); break;
    case 4: norm_launch_u<4, FP8>(s, a); break;
    default: norm_launch_u<8, FP8>(s, a); break;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

static int norm_run(const char* who, void* stream, const NormArgs& a) {
  return a.out_kind == GSX_ACT_OUT_FP8_ROW ? norm_launch<true>(who, S(stream), a)
                                           : norm_launch<false>(who, S(stream), a);
}

struct SiluArgs {
  int out_kind;
  const void* GU;
  int64_t gu_stride;
  void* Y;
  int64_t y_stride;
  float* scale_out;
  int M, I;
};

static int silu_validate(const char* who, const SiluArgs& a) {
  if (int rc = na_validate_out(who, a.out_kind, a.M, a.Y, a.scale_out)) return rc;
  const bool fp8 = a.out_kind == GSX_ACT_OUT_FP8_ROW;
  if (a.I < 8 || a.I % 8) return na_refuse(who, "need I >= 8 and I % 8 == 0");
  if (fp8 && a.I > SILU_MAX_ROW_I) return na_refuse(who, "need I <= 32768 with GSX_ACT_OUT_FP8_ROW");
  if (a.gu_stride < 2 * static_cast<int64_t>(a.I) || a.gu_stride % 8)
    return na_refuse(who, "need gu_stride >= 2 I and gu_stride % 8 == 0");
  if (a.y_stride < a.I || a.y_stride % 8) return na_refuse(who, "need y_stride >= I and y_stride % 8 == 0");
  if (!a.GU || !a.Y) return na_refuse(who, "GU and Y must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.GU) | reinterpret_cast<uintptr_t>(a.Y)) % 16)
    return na_refuse(who, "GU and Y must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(a.scale_out) % 4) return na_refuse(who, "scale_out must be 4-B aligned");
  const NaSpan gu = na_rows(a.GU, a.M, a.gu_stride, 2 * static_cast<int64_t>(a.I), 2),
             y = na_rows(a.Y, a.M, a.y_stride, a.I, fp8 ? 1 : 2), sc = na_rows(a.scale_out, 1, 0, a.M, 4);
  if (na_overlap(y, gu)) return na_refuse(who, "Y must not overlap GU");
  if (na_overlap(sc, gu) || na_overlap(sc, y)) return na_refuse(who, "scale_out must not overlap GU or Y");
  return 0;
}

template <int U>
static void silu_launch_row(hipStream_t s, const SiluArgs& a) {
  hipLaunchKernelGGL((silu_mul_row_kernel<U>), dim3(a.M), dim3(NA_THREADS), 0, s, static_cast<const uint16_t*>(a.GU),
                     a.gu_stride, static_cast<uint8_t*>(a.Y), a.y_stride, a.scale_out, a.I);
}

static int silu_run(const char* who, void* stream, const SiluArgs& a) {
  hipStream_t s = S(stream);
  const int nchunks = a.I / 8;
  if (a.out_kind == GSX_ACT_OUT_FP8_ROW) {
    switch (na_pick_u(nchunks)) {
      case 1: silu_launch_row<1>(s, a); break;
      case 2: silu_launch_row<2>(s, a); break;
      case 4: silu_launch_row<4>(s, a); break;
      case 8: silu_launch_row<8>(s, a); break;
      default: silu_launch_row<16>(s, a); break;
    }
  } else {
    constexpr int PER = NA_THREADS * SILU_GRID_U;
    const dim3 grid((nchunks + PER - 1) / PER, a.M < SILU_MAX_GRID_ROWS ? a.M : SILU_MAX_GRID_ROWS);
    hipLaunchKernelGGL(silu_mul_kernel, grid, dim3(NA_THREADS), 0, s, static_cast<const uint16_t*>(a.GU), a.gu_stride,
                       static_cast<uint16_t*>(a.Y), a.y_stride, a.M, a.I);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

int gsx_add_rmsnorm(void* stream, int out_kind, const void* X, int64_t x_stride, const void* R_in, void* R_out,
                    int64_t r_stride, const void* W, void* Y, int64_t y_stride, float* scale_out, int M, int H,
                    float eps) {
  const NormArgs a{out_kind, X, x_stride, R_in, R_out, r_stride, W, Y, y_stride, scale_out, M, H, eps};
  if (int rc = norm_validate("gsx_add_rmsnorm", a)) return rc;
  return norm_run("gsx_add_rmsnorm", stream, a);
}

int gsx_event_time_add_rmsnorm(void* stream, int out_kind, const void* X, int64_t x_stride, const void* R_in,
                               void* R_out, int64_t r_stride, const void* W, void* Y, int64_t y_stride,
                               float* scale_out, int M, int H, float eps, int iters, float* ms) {
  const NormArgs a{out_kind, X, x_stride, R_in, R_out, r_stride, W, Y, y_stride, scale_out, M, H, eps};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = norm_validate("gsx_add_rmsnorm", a)) return rc;
  return event_time(stream, iters, ms, [&] { return norm_run("gsx_add_rmsnorm", stream, a); });
}

int gsx_silu_mul(void* stream, int out_kind, const void* GU, int64_t gu_stride, void* Y, int64_t y_stride,
                 float* scale_out, int M, int I) {
  const SiluArgs a{out_kind, GU, gu_stride, Y, y_stride, scale_out, M, I};
  if (int rc = silu_validate("gsx_silu_mul", a)) return rc;
  return silu_run("gsx_silu_mul", stream, a);
}

int gsx_event_time_silu_mul(void* stream, int out_kind, const void* GU, int64_t gu_stride, void* Y, int64_t y_stride,
                            float* scale_out, int M, int I, int iters, float* ms) {
  const SiluArgs a{out_kind, GU, gu_stride, Y, y_stride, scale_out, M, I};
  if (int rc = silu_validate("gsx_silu_mul", a)) return rc;
  return event_time(stream, iters, ms, [&] { return silu_run("gsx_silu_mul", stream, a); });
}

}  // extern "C"
