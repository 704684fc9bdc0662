// What the decode attention kernels over the paged KV cache share (attn_decode.hip, attn_decode_multi.hip): the
// geometry of a tile of 32 tokens and of a wave's V image in LDS, the exact e4m3 -> bf16 conversion, and the weight
// of a partial in a merge.
#pragma once

#include <hip/hip_runtime.h>

#include "gemm_tile.h"

namespace gsxgemm {

typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) i16x4* lds_i16x4_t;

constexpr int AT_D = 128;           // head dimension
constexpr int AT_TILE = 32;         // tokens per tile: the k of one PV MFMA
constexpr int AT_VROW = 288;        // bytes of a row of the V image in LDS: 256 + 32 of padding
constexpr int AT_WAVE_LDS = AT_TILE * AT_VROW;  // 9216: a wave's V image, later its (acc, m, l)
constexpr int AT_MAX_SPLITS = 64;

// two e4m3 bytes of `w` (the low pair, or the high pair) as two bf16 in one dword; the conversion is exact
__device__ __forceinline__ int fp8x2_to_bf16x2(int w, bool hi) {
  const auto f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true) : __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  return static_cast<int>((__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u));
}
// 8 e4m3 bytes (two dwords) as 8 bf16
__device__ __forceinline__ i32x4 fp8x8_to_bf16x8(int lo, int hi) {
  return i32x4{fp8x2_to_bf16x2(lo, false), fp8x2_to_bf16x2(lo, true), fp8x2_to_bf16x2(hi, false),
               fp8x2_to_bf16x2(hi, true)};
}

// The weight of a partial (m, l, acc) in a merge whose maximum is M: a partial without a token has m = -inf and
// weight 0, also when M is -inf too.
__device__ __forceinline__ float merge_weight(float m, float M) {
  return m == -__builtin_inff() ? 0.f : __builtin_amdgcn_exp2f(m - M);
}

}  // namespace gsxgemm
