// The 16-bit key that orders bf16 codes, shared by the sampler (sample.hip) and the MoE router (moe.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsxgemm {

// -0 is +0, every NaN is 0, below -inf (0x007f).
__device__ __forceinline__ uint32_t sm_key(uint32_t b) {
  if ((b & 0x7fffu) > 0x7f80u) return 0u;
  if (b == 0x8000u) return 0x8000u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

}  // namespace gsxgemm
