// Compute pre-flight for MI355X (gfx950): a known-answer test of every CU's matrix cores, vector ALU and LDS.
// C ABI at the end of gsx_kernels.h; NumPy twin in ops/cutest.py.
//
// One kernel.  A workgroup is 4 waves and declares all 160 KiB of LDS, so a CU holds one workgroup at a time and a
// grid a few times the CU count spreads over every CU the stream's mask allows.  Every wave reads HW_ID / XCC_ID
// as cuprobe_kernel does, runs the units of the table in gsx_kernels.h and writes one record from lane 0 with
// plain stores.  No scratch, no atomics.
//
// What makes the answer known:
//  * operands are a function of (seed, unit, round, matrix coordinates), never of lane or register: elem().  The
//    kernel places them by the lane maps of the matrix instructions; the twins compute a plain integer A @ B;
//  * every result is an exact integer whatever the summation order: sum |a| |b| over a chain stays below 2^24
//    (f32 accumulators) or 2^31 (MFMA_I8); rounds per unit in kUnits;
//  * a signature is sum over (i, j) of mix64(bits32(D[i][j]) ^ (i * N + j + 1) * odd): position-dependent and
//    order-free, so the lanes reduce in any order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <chrono>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "hwid.h"
#include "mix64.h"

using namespace gsx;

namespace {

#define GSX_HD __host__ __device__ __forceinline__

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kUnitCount = GSX_CUTEST_UNITS;
constexpr int kMatrixUnits = 7;
constexpr uint32_t kIntSteps = 256;                  // VALU_INT: steps of a lane's chain
constexpr uint32_t kLdsBytes = 163840;               // all of a CU's LDS
constexpr uint32_t kLdsWords = kLdsBytes / 16;       // 16-B words
constexpr uint32_t kQuarterWords = kLdsWords / 4;    // a wave fills and checks a quarter
constexpr uint32_t kQuarterDwords = 4 * kQuarterWords;
static_assert(kQuarterWords % 128 == 0, "a quarter's halves are whole 64-lane sweeps");

// The matrix units: a chain of `rounds` M x N x K products of integers in [-span/2, span/2 - 1]; `gen` is the unit
// whose operands it multiplies (VALU_F32 takes MFMA_F32's).  64 rounds keep the 16-bit, fp8 and i8 chains exact
// (64 * 32 * 8 * 8 = 2^17, 64 * 64 * 128 * 128 = 2^26 < 2^31), 32 rounds the f32 ones (32 * 4 * 2^16 = 2^23 < 2^24).
struct Unit {
  const char* name;
  int m, n, k, rounds, span, gen;
  bool integer;
};
constexpr Unit kUnits[kMatrixUnits] = {
    {"MFMA_BF16_16", 16, 16, 32, 64, 16, GSX_CUTEST_MFMA_BF16_16, false},
    {"MFMA_BF16_32", 32, 32, 16, 64, 16, GSX_CUTEST_MFMA_BF16_32, false},
    {"MFMA_F16", 16, 16, 32, 64, 16, GSX_CUTEST_MFMA_F16, false},
    {"MFMA_FP8", 16, 16, 32, 64, 16, GSX_CUTEST_MFMA_FP8, false},
    {"MFMA_I8", 16, 16, 64, 64, 256, GSX_CUTEST_MFMA_I8, true},
    {"MFMA_F32", 16, 16, 4, 32, 512, GSX_CUTEST_MFMA_F32, false},
    {"VALU_F32", 16, 16, 4, 32, 512, GSX_CUTEST_MFMA_F32, false},
};
constexpr const char* kOtherNames[kUnitCount - kMatrixUnits] = {"VALU_INT", "LDS"};
constexpr uint32_t kSeeds[] = {8, 256};  // by level: QUICK, FULL

// ------------------------------------------------------------------ what the kernel and the host twin share

// mix64 and seed_key: mix64.h, as the memory test's generator

// A[i][k] (which 0) or B[k][j] (which 1, with j in the place of i) of unit u in round r
GSX_HD int elem(uint64_t key, uint32_t u, uint32_t r, uint32_t which, uint32_t i, uint32_t k, uint32_t span) {
  const uint64_t ctr = (static_cast<uint64_t>(u) << 32) | (r << 24) | (which << 16) | (i << 8) | k;
  return static_cast<int>(static_cast<uint32_t>(mix64(key + ctr) >> 32) & (span - 1u)) - static_cast<int>(span / 2u);
}

// one term of a signature: the value at position n (counted from 1)
GSX_HD uint64_t fold(uint64_t v, uint64_t n) { return mix64(v ^ (n * kGolden)); }

// VALU_INT: one lane's chain
GSX_HD void int_chain(uint64_t key, uint32_t lane, uint32_t* xo, uint64_t* yo) {
  uint64_t y = mix64(key + (static_cast<uint64_t>(GSX_CUTEST_VALU_INT) << 32) + lane);
  uint32_t x = static_cast<uint32_t>(y >> 32);
  for (uint32_t s = 0; s < kIntSteps; ++s) {
    const uint32_t c = static_cast<uint32_t>(y) | 1u;
    const uint32_t lo = x * 0x9E3779B1u;                                                // v_mul_lo_u32
    const uint32_t hi = static_cast<uint32_t>((static_cast<uint64_t>(x) * c) >> 32);    // v_mul_hi_u32
    y = y * 0xD1342543DE82EF95ull + ((static_cast<uint64_t>(hi) << 32) | lo);           // 64-bit multiply-add
    const uint32_t r = __builtin_rotateleft32(lo ^ hi, static_cast<uint32_t>(y >> 59));
    const uint32_t p = static_cast<uint32_t>(__builtin_popcountll(y));
    x = r > static_cast<uint32_t>(y >> 32) ? r + p : r ^ (p * 0x01010101u);             // compare-select
  }
  *xo = x;
  *yo = y;
}
GSX_HD uint64_t int_fold(uint32_t x, uint64_t y, uint32_t lane) { return fold(y, lane + 1) + fold(x, lane + 65); }

// LDS: dword d of the memory test's RANDOM words (word d / 4, half (d / 2) & 1, as gen_word in memtest.hip)
GSX_HD uint32_t lds_dword(uint64_t key, uint32_t d, uint32_t inv) {
  const uint64_t z = random_half(d >> 2, (d >> 1) & 1u, key);
  return static_cast<uint32_t>(d & 1u ? z >> 32 : z) ^ inv;
}

// ------------------------------------------------------------------ device

__device__ __forceinline__ uint64_t wave_sum(uint64_t s) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(static_cast<unsigned long long>(s), o, 64);
  return s;
}

// C/D of every 16x16 instruction: col = lane & 15, row = 4 * (lane >> 4) + reg
__device__ __forceinline__ uint64_t fold_16x16(const uint32_t (&bits)[4], int lane, uint32_t inj) {
  uint64_t s = 0;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const uint32_t row = 4 * (lane >> 4) + reg, col = lane & 15;
    const uint32_t b = bits[reg] ^ (reg == 0 && lane == 0 ? inj : 0u);  // element (0, 0)
    s += fold(b, row * 16 + col + 1);
  }
  return wave_sum(s);
}

// 8 integers in [-8, 7] as one operand of a 16x16x32 / 32x32x16 instruction
__device__ __forceinline__ bf16x8 pack_bf16(const int (&v)[8]) {
  s16x8 s;
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = static_cast<short>(__float_as_uint(static_cast<float>(v[j])) >> 16);
  return __builtin_bit_cast(bf16x8, s);
}
__device__ __forceinline__ f16x8 pack_f16(const int (&v)[8]) {
  f16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = static_cast<_Float16>(static_cast<float>(v[j]));
  return h;
}
// OCP e4m3: sign, 4 exponent bits (bias 7), 3 mantissa bits; every integer in [-8, 8] is exact
__device__ __forceinline__ long pack_fp8(const int (&v)[8]) {
  uint64_t q = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t f = __float_as_uint(static_cast<float>(v[j]));
    const uint32_t b = v[j] == 0 ? 0u : ((((f >> 20) & 0x7FFu) - (120u << 3)) | ((f >> 24) & 0x80u));
    q |= static_cast<uint64_t>(b & 0xFFu) << (8 * j);
  }
  return static_cast<long>(q);
}

// MFMA_BF16_16, MFMA_F16, MFMA_FP8: lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15]
template <int U>
__device__ __forceinline__ uint64_t unit_16x16x32(uint64_t key, int lane, uint32_t inj) {
  const uint32_t rc = lane & 15, kb = 8 * (lane >> 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t r = 0; r < static_cast<uint32_t>(kUnits[U].rounds); ++r) {
    int a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = elem(key, U, r, 0, rc, kb + j, 16);
      b[j] = elem(key, U, r, 1, rc, kb + j, 16);
    }
    if constexpr (U == GSX_CUTEST_MFMA_BF16_16) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pack_bf16(a), pack_bf16(b), acc, 0, 0, 0);
    } else if constexpr (U == GSX_CUTEST_MFMA_F16) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(pack_f16(a), pack_f16(b), acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack_fp8(a), pack_fp8(b), acc, 0, 0, 0);
    }
  }
  const uint32_t bits[4] = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]),
                            __float_as_uint(acc[3])};
  return fold_16x16(bits, lane, inj);
}

// MFMA_BF16_32: lane l holds A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31]; C/D col = l & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
__device__ __forceinline__ uint64_t unit_32x32x16(uint64_t key, int lane, uint32_t inj) {
  constexpr int U = GSX_CUTEST_MFMA_BF16_32;
  const uint32_t rc = lane & 31, kb = 8 * (lane >> 5);
  f32x16 acc;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
  for (uint32_t r = 0; r < static_cast<uint32_t>(kUnits[U].rounds); ++r) {
    int a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = elem(key, U, r, 0, rc, kb + j, 16);
      b[j] = elem(key, U, r, 1, rc, kb + j, 16);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pack_bf16(a), pack_bf16(b), acc, 0, 0, 0);
  }
  uint64_t s = 0;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const uint32_t row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = lane & 31;
    const uint32_t b = __float_as_uint(acc[reg]) ^ (reg == 0 && lane == 0 ? inj : 0u);
    s += fold(b, row * 32 + col + 1);
  }
  return wave_sum(s);
}

// MFMA_I8: lane l holds A[l & 15][16 (l >> 4) + j] and B[16 (l >> 4) + j][l & 15], j = 0 .. 15, one byte each
__device__ __forceinline__ uint64_t unit_i8(uint64_t key, int lane, uint32_t inj) {
  constexpr int U = GSX_CUTEST_MFMA_I8;
  const uint32_t rc = lane & 15, kb = 16 * (lane >> 4);
  i32x4 acc = {0, 0, 0, 0};
  for (uint32_t r = 0; r < static_cast<uint32_t>(kUnits[U].rounds); ++r) {
    i32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      a[j >> 2] |= (elem(key, U, r, 0, rc, kb + j, 256) & 0xFF) << (8 * (j & 3));
      b[j >> 2] |= (elem(key, U, r, 1, rc, kb + j, 256) & 0xFF) << (8 * (j & 3));
    }
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
  }
  const uint32_t bits[4] = {static_cast<uint32_t>(acc[0]), static_cast<uint32_t>(acc[1]),
                            static_cast<uint32_t>(acc[2]), static_cast<uint32_t>(acc[3])};
  return fold_16x16(bits, lane, inj);
}

// MFMA_F32: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]
__device__ __forceinline__ uint64_t unit_f32(uint64_t key, int lane, uint32_t inj) {
  constexpr int U = GSX_CUTEST_MFMA_F32;
  const uint32_t rc = lane & 15, k = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t r = 0; r < static_cast<uint32_t>(kUnits[U].rounds); ++r) {
    const float a = static_cast<float>(elem(key, U, r, 0, rc, k, 512));
    const float b = static_cast<float>(elem(key, U, r, 1, rc, k, 512));
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const uint32_t bits[4] = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]),
                            __float_as_uint(acc[3])};
  return fold_16x16(bits, lane, inj);
}

// VALU_F32: the product of MFMA_F32, every lane computing the four elements the C/D map gives it with v_fma_f32
__device__ __forceinline__ uint64_t unit_valu_f32(uint64_t key, int lane, uint32_t inj) {
  constexpr int U = GSX_CUTEST_MFMA_F32;
  const uint32_t col = lane & 15, row0 = 4 * (lane >> 4);
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t r = 0; r < static_cast<uint32_t>(kUnits[U].rounds); ++r) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const float b = static_cast<float>(elem(key, U, r, 1, col, k, 512));
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        out[reg] = __builtin_fmaf(static_cast<float>(elem(key, U, r, 0, row0 + reg, k, 512)), b, out[reg]);
    }
  }
  const uint32_t bits[4] = {__float_as_uint(out[0]), __float_as_uint(out[1]), __float_as_uint(out[2]),
                            __float_as_uint(out[3])};
  return fold_16x16(bits, lane, inj);
}

__device__ __forceinline__ uint64_t unit_valu_int(uint64_t key, int lane, uint32_t inj) {
  uint32_t x;
  uint64_t y;
  int_chain(key, lane, &x, &y);
  if (lane == 0) x ^= inj;
  return wave_sum(int_fold(x, y, lane));
}

// LDS, two passes (the RANDOM words, then their complement).  Wave w fills quarter w with the words of the
// ABSOLUTE dword index; after the barrier it reads quarter (w + 1) & 3, which another wave wrote, the first half
// as 16-B words (ds_read_b128) and the second as dwords (ds_read_b32), and compares: what it folds is
// read ^ expected(absolute index) ^ expected(index in the quarter) -- the word of the index in the quarter when the
// LDS returned what was written, so every wave of a healthy CU ends in the same signature, while a dword that
// reads back wrong, or comes from another address, does not.
__device__ __forceinline__ uint64_t unit_lds(uint4* lds, uint64_t key, int wave, int lane, uint32_t inj) {
  const uint32_t mine = wave * kQuarterWords, theirs = ((wave + 1) & 3) * kQuarterWords;
  const uint32_t* lds32 = reinterpret_cast<const uint32_t*>(lds);
  uint64_t s = 0;
  for (uint32_t p = 0; p < 2; ++p) {
    const uint32_t inv = p ? 0xFFFFFFFFu : 0u;
    const uint32_t at = p * kQuarterDwords + 1;  // a pass's positions follow the pass before
    for (uint32_t w = lane; w < kQuarterWords; w += 64) {
      const uint32_t d = 4 * (mine + w);
      lds[mine + w] = make_uint4(lds_dword(key, d, inv), lds_dword(key, d + 1, inv), lds_dword(key, d + 2, inv),
                                 lds_dword(key, d + 3, inv));
    }
    __syncthreads();
    for (uint32_t w = lane; w < kQuarterWords / 2; w += 64) {
      const uint4 got = lds[theirs + w];
      const uint32_t g[4] = {got.x, got.y, got.z, got.w};
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        uint32_t v = g[c] ^ lds_dword(key, 4 * (theirs + w) + c, inv) ^ lds_dword(key, 4 * w + c, inv);
        if (p == 0 && w == 0 && c == 0) v ^= inj;  // dword 0 of the quarter (w == 0 is lane 0's first word)
        s += fold(v, at + 4 * w + c);
      }
    }
    for (uint32_t d = kQuarterDwords / 2 + lane; d < kQuarterDwords; d += 64) {
      const uint32_t v = lds32[4 * theirs + d] ^ lds_dword(key, 4 * theirs + d, inv) ^ lds_dword(key, d, inv);
      s += fold(v, at + d);
    }
    __syncthreads();  // nobody refills a quarter that is still being read
  }
  return wave_sum(s);
}

struct Expected {
  uint64_t sig[kUnitCount];
};

__global__ __launch_bounds__(256) void cutest_kernel(gsx_cutest_record* __restrict__ out, uint32_t seed, Expected want,
                                                     gsx_cutest_inject inj) {
  __shared__ uint4 lds[kLdsWords];
  uint32_t hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t key = seed_key(seed);
  const HwId at{hw, xcc};
  const bool hit = inj.xor_mask != 0 && static_cast<int>(at.xcc()) == inj.xcc &&
                   static_cast<int>(at.se()) == inj.se && static_cast<int>(at.sh()) == inj.sh &&
                   static_cast<int>(at.cu()) == inj.cu && (inj.simd < 0 || static_cast<int>(at.simd()) == inj.simd);
  const int iu = hit ? inj.unit : -1;
  const uint32_t m = inj.xor_mask;
  uint64_t sig[kUnitCount];
  sig[0] = unit_16x16x32<GSX_CUTEST_MFMA_BF16_16>(key, lane, iu == 0 ? m : 0u);
  sig[1] = unit_32x32x16(key, lane, iu == 1 ? m : 0u);
  sig[2] = unit_16x16x32<GSX_CUTEST_MFMA_F16>(key, lane, iu == 2 ? m : 0u);
  sig[3] = unit_16x16x32<GSX_CUTEST_MFMA_FP8>(key, lane, iu == 3 ? m : 0u);
  sig[4] = unit_i8(key, lane, iu == 4 ? m : 0u);
  sig[5] = unit_f32(key, lane, iu == 5 ? m : 0u);
  sig[6] = unit_valu_f32(key, lane, iu == 6 ? m : 0u);
  sig[7] = unit_valu_int(key, lane, iu == 7 ? m : 0u);
  sig[8] = unit_lds(lds, key, wave, lane, iu == 8 ? m : 0u);
  if (lane == 0) {
    uint32_t fail = 0;
#pragma unroll
    for (int u = 0; u < kUnitCount; ++u) fail |= (sig[u] != want.sig[u] ? 1u : 0u) << u;
    gsx_cutest_record* rec = out + (blockIdx.x * 4u + wave);
    rec->hw_id = hw;
    rec->xcc_id = xcc;
    rec->fail_mask = fail;
    rec->seed = seed;
#pragma unroll
    for (int u = 0; u < kUnitCount; ++u) rec->sig[u] = sig[u];
  }
}

// ------------------------------------------------------------------ host

uint64_t matrix_expected(int unit, uint32_t seed) {
  const Unit& t = kUnits[unit];
  const uint64_t key = seed_key(seed);
  std::vector<int64_t> d(static_cast<size_t>(t.m) * t.n, 0);
  std::vector<int> a(static_cast<size_t>(t.m) * t.k), b(static_cast<size_t>(t.n) * t.k);
  for (int r = 0; r < t.rounds; ++r) {
    for (int i = 0; i < t.m; ++i)
      for (int k = 0; k < t.k; ++k) a[i * t.k + k] = elem(key, t.gen, r, 0, i, k, t.span);
    for (int j = 0; j < t.n; ++j)
      for (int k = 0; k < t.k; ++k) b[j * t.k + k] = elem(key, t.gen, r, 1, j, k, t.span);
    for (int i = 0; i < t.m; ++i)
      for (int j = 0; j < t.n; ++j) {
        int64_t s = 0;
        for (int k = 0; k < t.k; ++k) s += static_cast<int64_t>(a[i * t.k + k]) * b[j * t.k + k];
        d[i * t.n + j] += s;
      }
  }
  uint64_t sig = 0;
  for (int i = 0; i < t.m; ++i)
    for (int j = 0; j < t.n; ++j) {
      uint32_t bits;
      if (t.integer) {
        bits = static_cast<uint32_t>(static_cast<int32_t>(d[i * t.n + j]));
      } else {
        const float f = static_cast<float>(d[i * t.n + j]);  // exact: |d| < 2^24
        std::memcpy(&bits, &f, 4);
      }
      sig += fold(bits, static_cast<uint64_t>(i) * t.n + j + 1);
    }
  return sig;
}

uint64_t int_expected(uint32_t seed) {
  const uint64_t key = seed_key(seed);
  uint64_t sig = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    uint32_t x;
    uint64_t y;
    int_chain(key, lane, &x, &y);
    sig += int_fold(x, y, lane);
  }
  return sig;
}

uint64_t lds_expected(uint32_t seed) {
  const uint64_t key = seed_key(seed);
  uint64_t sig = 0;
  for (uint32_t p = 0; p < 2; ++p)
    for (uint32_t d = 0; d < kQuarterDwords; ++d)
      sig += fold(lds_dword(key, d, p ? 0xFFFFFFFFu : 0u), p * kQuarterDwords + 1 + d);
  return sig;
}

uint64_t unit_expected(int unit, uint32_t seed) {
  if (unit < kMatrixUnits) return matrix_expected(unit, seed);
  return unit == GSX_CUTEST_VALU_INT ? int_expected(seed) : lds_expected(seed);
}

// every unit's expected signature for a seed; the levels' seeds are few and come back at every run
std::mutex g_mu;
std::unordered_map<uint32_t, Expected> g_expected;

Expected expected_for(uint32_t seed) {
  {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_expected.find(seed);
    if (it != g_expected.end()) return it->second;
  }
  Expected e;
  for (int u = 0; u < kUnitCount; ++u) e.sig[u] = unit_expected(u, seed);
  std::lock_guard<std::mutex> g(g_mu);
  if (g_expected.size() >= 1024) g_expected.clear();
  g_expected[seed] = e;
  return e;
}

int device_cus(uint32_t* cus) {
  int dev = 0, n = 0;
  if (int rc = current_device("gsx_cutest", &dev)) return rc;
  GSX_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  *cus = n > 0 ? static_cast<uint32_t>(n) : 1u;
  return 0;
}

}  // namespace

extern "C" {

const char* gsx_cutest_unit_name(int unit) {
  if (unit < 0 || unit >= kUnitCount) return nullptr;
  return unit < kMatrixUnits ? kUnits[unit].name : kOtherNames[unit - kMatrixUnits];
}

int gsx_cutest_unit_shape(int unit, int* m, int* n, int* k, int* rounds, int* span) {
  if (unit < 0 || unit >= kMatrixUnits) return 1;
  const Unit& t = kUnits[unit];
  *m = t.m, *n = t.n, *k = t.k, *rounds = t.rounds, *span = t.span;
  return 0;
}

uint32_t gsx_cutest_seeds(int level) {
  return level == GSX_CUTEST_QUICK || level == GSX_CUTEST_FULL ? kSeeds[level] : 0;
}

int gsx_cutest_expected(int unit, uint32_t seed, uint64_t* sig) {
  if (unit < 0 || unit >= kUnitCount || !sig) return fail_arg("gsx_cutest_expected: unknown unit");
  *sig = unit_expected(unit, seed);
  return 0;
}

int gsx_cutest_launch(void* stream, uint32_t seed, int blocks, const gsx_cutest_inject* inject,
                      gsx_cutest_record* records_out, uint32_t n) {
  if (blocks <= 0 || blocks > GSX_CUTEST_MAX_BLOCKS) return fail_arg("gsx_cutest_launch: bad block count");
  const uint32_t waves = 4u * static_cast<uint32_t>(blocks);
  if (!records_out || n < waves) return fail_arg("gsx_cutest_launch: records_out holds fewer than 4 * blocks");
  gsx_cutest_inject inj{};
  if (inject) {
    if (inject->unit < 0 || inject->unit >= kUnitCount) return fail_arg("gsx_cutest_launch: unknown unit to inject");
    inj = *inject;
  }
  const Expected want = expected_for(seed);
  hipStream_t st = S(stream);
  gsx_cutest_record* d = nullptr;
  const size_t bytes = sizeof(gsx_cutest_record) * waves;
  GSX_CHECK(hipMallocAsync(reinterpret_cast<void**>(&d), bytes, st));
  hipLaunchKernelGGL(cutest_kernel, dim3(blocks), dim3(256), 0, st, d, seed, want, inj);
  GSX_CHECK(hipGetLastError());
  GSX_CHECK(hipMemcpyAsync(records_out, d, bytes, hipMemcpyDeviceToHost, st));
  GSX_CHECK(hipFreeAsync(d, st));
  GSX_CHECK(hipStreamSynchronize(st));
  return 0;
}

int gsx_cutest_aggregate(const gsx_cutest_record* records, uint32_t n, gsx_cutest_report* rep) {
  if (!rep || (n && !records)) return fail_arg("gsx_cutest_aggregate: no records or no report");
  for (uint32_t w = 0; w < n; ++w) {
    const gsx_cutest_record& r = records[w];
    const HwId at{r.hw_id, r.xcc_id};
    const uint32_t xcc = at.xcc(), se = at.se(), sh = at.sh(), cu = at.cu(), simd = 1u << at.simd();
    gsx_cutest_cu& c = rep->cu[cu_slot(at)];
    if (!c.waves) ++rep->cus_seen;
    if (!(c.simds & simd)) {
      ++rep->simds_seen;
      c.simds |= simd;
      if (c.simds == 0xF) ++rep->cus_covered;
    }
    ++c.waves;
    ++rep->waves;
    const uint32_t fail = r.fail_mask & ((1u << kUnitCount) - 1u);
    if (!fail) continue;
    ++c.bad_waves;
    ++rep->bad_waves;
    if (!c.fail_mask) {
      ++rep->bad_cus;
      if (rep->n_bad < GSX_CUTEST_MAX_BAD) {
        gsx_cutest_bad& b = rep->bad[rep->n_bad++];
        std::memset(&b, 0, sizeof b);
        b.xcc = xcc, b.se = se, b.sh = sh, b.cu = cu;
        b.unit = static_cast<uint8_t>(__builtin_ctz(fail));
        b.seed = r.seed;
        b.expected = unit_expected(b.unit, r.seed);
        b.got = r.sig[b.unit];
      }
    }
    c.fail_mask |= fail;
    c.bad_simds |= simd;
    for (uint32_t k = 0; k < rep->n_bad; ++k) {
      gsx_cutest_bad& b = rep->bad[k];
      if (b.xcc == xcc && b.se == se && b.sh == sh && b.cu == cu) b.simds = c.bad_simds, b.units = c.fail_mask;
    }
  }
  return 0;
}

int gsx_cutest_stream_cus(void* stream, uint32_t* cus) {
  if (!cus) return fail_arg("gsx_cutest_stream_cus: no result");
  uint32_t dev = 0;
  if (int rc = device_cus(&dev)) return rc;
  uint32_t mask[8] = {0};
  uint32_t bits = 0;
  if (stream && hipExtStreamGetCUMask(S(stream), 8, mask) == hipSuccess) {
    for (uint32_t w : mask) bits += static_cast<uint32_t>(__builtin_popcount(w));
  } else {
    (void)hipGetLastError();
  }
  *cus = bits && bits < dev ? bits : dev;
  return 0;
}

int gsx_cutest_run(void* stream, int level, uint32_t expect_cus, gsx_cutest_report* rep, double* seconds_out) {
  bool truncated = false;
  return cutest_run(stream, level, expect_cus, CutestOpts{}, rep, seconds_out, &truncated);
}

}  // extern "C"

namespace gsx __attribute__((visibility("hidden"))) {

int cutest_run(void* stream, int level, uint32_t expect_cus, const CutestOpts& opts, gsx_cutest_report* rep,
               double* seconds, bool* truncated) {
  const uint32_t seeds = gsx_cutest_seeds(level);
  if (!seeds) return fail_arg("gsx_cutest_run: unknown level");
  if (!rep) return fail_arg("gsx_cutest_run: no report");
  const auto t0 = std::chrono::steady_clock::now();
  const auto since = [t0] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
  if (!expect_cus)
    if (int rc = gsx_cutest_stream_cus(stream, &expect_cus)) return rc;
  const uint64_t want = 4ull * expect_cus;
  const int blocks = static_cast<int>(want < GSX_CUTEST_MAX_BLOCKS ? want : GSX_CUTEST_MAX_BLOCKS);
  std::vector<gsx_cutest_record> recs(4u * static_cast<size_t>(blocks));
  int rc = 0;
  // the level's seeds, then further ones while a CU still has a SIMD no wave ran on
  for (uint32_t k = 0; !rc && (k < seeds || (rep->cus_covered < expect_cus && k < seeds + GSX_CUTEST_EXTRA_LAUNCHES));
       ++k) {
    if (opts.max_seconds > 0 && since() >= opts.max_seconds) {
      *truncated = true;
      break;
    }
    rc = gsx_cutest_launch(stream, k, blocks, opts.inject, recs.data(), static_cast<uint32_t>(recs.size()));
    if (!rc) rc = gsx_cutest_aggregate(recs.data(), static_cast<uint32_t>(recs.size()), rep);
    if (!rc) ++rep->launches;
  }
  rep->cus_expected = expect_cus;
  rep->covered = rep->cus_covered >= expect_cus;
  if (seconds) *seconds = since();
  return rc;
}

}  // namespace gsx
