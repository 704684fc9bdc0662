// bf16 <-> fp32 and fp32 -> OCP e4m3 on one 16-B chunk of 8 elements: what norm_act.hip's e4m3 outputs and the block
// quantiser of gemm_fp8_block.hip share.  Internal, like gemm_tile.h.
#pragma once

#include "gemm_tile.h"

namespace gsxgemm {

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

}  // namespace gsxgemm
