// The counter-based generator of the memory test's RANDOM pattern and of the compute test's operands and signatures,
// for kernels and host code.  NumPy twin: ops/memtest.py (_mix64, _GOLDEN).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsx {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// splitmix64's output function: two multiply-xorshift rounds (bijective; mix64(0) is 0)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// what a seed adds to every counter; never 0
__host__ __device__ __forceinline__ uint64_t seed_key(uint32_t seed) {
  return (static_cast<uint64_t>(seed) + 1ull) * kGolden;
}

// RANDOM: 64-bit half `half` (0 or 1) of 16-byte word W
__host__ __device__ __forceinline__ uint64_t random_half(uint64_t W, uint32_t half, uint64_t key) {
  return mix64(2ull * W + half + key);
}

}  // namespace gsx
