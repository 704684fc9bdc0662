// RoPE and KV-cache append for the pod workload: the glue between the fused QKV projection (gemm_decode.hip) and the
// decode attention (attn_decode.hip).  Row n of QKV holds token n's Hq query heads, Hkv key heads and Hkv value heads
// of D = 128; the kernel rotates Q and K by the token's position (half-split pairing, tables supplied by the caller),
// writes Q to Q_out and the token's K and V into its slot of the paged caches, quantised for an e4m3 cache.  With
// T = 1 it is a decode step's cache write, with many tokens per sequence that of a prefill chunk, where it is bound by
// HBM bandwidth.  C ABI and numeric contract in gsx_kernels.h.
//
// kv_append_kernel: a workgroup of 256 threads owns one token and nothing passes between workgroups.
//   * A head row is 256 B = 16 chunks of 16 B.  Eight lanes share a head row: lane j loads chunk j and chunk j + 8,
//     which hold the two halves (x[i], x[i + 64]) of its 8 rotation pairs, rotates in registers and stores both
//     halves.  A wave covers 8 head rows per pass and the workgroup 32; a lane has the loads of KVA_U = 4 passes
//     in flight before it touches the first.
//   * The token's cos / sin chunks (8 floats each, the lane's 8 pairs) are loaded once and serve all Hq + Hkv rotated
//     heads.  V heads go straight through: a raw copy for a bf16 cache.
//   * Every fp32 multiply, add and subtract of the rotation is rounded on its own: rope_pair() switches contraction
//     into an FMA off for them.
//   * e4m3: the scaled value is clamped to +-448 (v_med3_f32; a NaN stays a NaN) in front of v_cvt_pk_fp8_f32, so the
//     conversion never sees a value out of range.
//   * No LDS, no atomics.  Everything that decides whether a token is live (its sequence's length, its page index) is
//     uniform over the workgroup.  A token that is not live writes zeros to its Q_out row and nothing else: a bad page
//     index is dropped, never clamped.  lens_out[b] is written by the workgroup of the sequence's token 0.
// Offsets into the caches, QKV and Q_out are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

constexpr int KVA_D = 128;        // head dimension
constexpr int KVA_THREADS = 256;  // 32 head rows per pass
constexpr int KVA_U = 4;          // passes whose loads a lane has in flight

// 8 bf16 (one 16-B chunk) as fp32: exact
__device__ __forceinline__ void bf16x8_to_f32(const i32x4& v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(static_cast<uint32_t>(v[i]) << 16);
    f[2 * i + 1] = __uint_as_float(static_cast<uint32_t>(v[i]) & 0xffff0000u);
  }
}

// 8 fp32 as 8 bf16, round to nearest even
__device__ __forceinline__ i32x4 f32_to_bf16x8(const float* f) {
  i32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] = static_cast<int>(f2bf(f[2 * i]) | (static_cast<uint32_t>(f2bf(f[2 * i + 1])) << 16));
  return v;
}

// One rotation pair: x1' = fl(fl(x1 c) - fl(x2 s)), x2' = fl(fl(x2 c) + fl(x1 s)).  The contract rounds every
// operation on its own.  hipcc contracts by default (-ffp-contract=fast-honor-pragmas), and it does so through
// __fmul_rn and __fsub_rn as well: they are plain operators inlined from a header, outside the reach of a pragma
// here.  So the operators stand here themselves, under the pragma, and the kernel's code holds v_pk_mul_f32,
// v_sub_f32 and v_add_f32 and no v_fma (tests/test_gpu_kv_append.py's cancellation case fails on an FMA).
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& y1, float& y2) {
#pragma clang fp contract(off)
  const float p1 = x1 * c, p2 = x2 * s, p3 = x2 * c, p4 = x1 * s;
  y1 = p1 - p2;
  y2 = p3 + p4;
}

// fl(x * inv) onto OCP e4m3fn, round to nearest even, saturating: every finite value beyond +-448 and +-inf give
// +-448; a NaN passes the clamp as it is and the conversion makes a NaN code of it.
__device__ __forceinline__ float e4m3_clamp(float x, float inv) {
  const float y = __fmul_rn(x, inv);
  const float c = __builtin_amdgcn_fmed3f(y, -448.f, 448.f);
  return y != y ? y : c;
}
__device__ __forceinline__ i32x2 f32_to_e4m3x8(const float* f, float inv) {
  i32x2 v;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(e4m3_clamp(f[4 * i], inv), e4m3_clamp(f[4 * i + 1], inv), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(e4m3_clamp(f[4 * i + 2], inv), e4m3_clamp(f[4 * i + 3], inv), w, true);
    v[i] = w;
  }
  return v;
}

template <bool FP8>
__global__ __launch_bounds__(KVA_THREADS) void kv_append_kernel(
    const uint16_t* __restrict__ QKV, int64_t qkv_stride, uint16_t* __restrict__ Q_out, uint8_t* __restrict__ Kc,
    uint8_t* __restrict__ Vc, const int32_t* __restrict__ block_table, const int32_t* __restrict__ seq_lens,
    int32_t* __restrict__ lens_out, const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, int T,
    int Hq, int Hkv, int page, int num_pages, int table_stride, int max_seq_len, float k_inv, float v_inv) {
  constexpr int ROWB = FP8 ? KVA_D : 2 * KVA_D;  // bytes of a token's row in the cache
  const int n = blockIdx.x;                      // the token: sequence n / T, its new token number n % T
  const int b = n / T, t = n - b * T;
  int base = seq_lens[b];
  base = base < 0 ? 0 : base > max_seq_len ? max_seq_len : base;
  if (t == 0 && threadIdx.x == 0 && lens_out) {
    const int64_t after = static_cast<int64_t>(base) + T;
    lens_out[b] = after < max_seq_len ? static_cast<int32_t>(after) : max_seq_len;
  }
  const int64_t pos = static_cast<int64_t>(base) + t;
  bool live = pos < max_seq_len;
  int pp = 0;
  if (live) {  // pos / page < table_stride: max_seq_len <= table_stride * page
    pp = block_table[static_cast<size_t>(b) * table_stride + static_cast<int>(pos) / page];
    live = static_cast<uint32_t>(pp) < static_cast<uint32_t>(num_pages);
  }
  uint16_t* const qrow = Q_out + static_cast<size_t>(n) * Hq * KVA_D;
  if (!live) {  // uniform over the workgroup
    for (int c = threadIdx.x; c < Hq * (KVA_D / 8); c += KVA_THREADS)
      *reinterpret_cast<i32x4*>(qrow + c * 8) = i32x4{0, 0, 0, 0};
    return;
  }

  const int j = threadIdx.x & 7;     // the lane's pairs: d = 8 j .. 8 j + 7 with d + 64
  const int grp = threadIdx.x >> 3;  // the lane's head row of a pass
  float cs[8], sn[8];
  {
    const float* cp = rope_cos + static_cast<size_t>(pos) * (KVA_D / 2) + 8 * j;
    const float* sp = rope_sin + static_cast<size_t>(pos) * (KVA_D / 2) + 8 * j;
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cs[e] = c0[e];
      cs[e + 4] = c1[e];
      sn[e] = s0[e];
      sn[e + 4] = s1[e];
    }
  }
  const int R = Hq + 2 * Hkv;  // head rows of the token
  const uint16_t* const src = QKV + static_cast<size_t>(n) * qkv_stride + 8 * j;
  const int slot = static_cast<int>(pos) - (static_cast<int>(pos) / page) * page;
  // the token's row of KV head 0 in a cache, in rows; KV head h is h * page rows on
  const size_t row0 = static_cast<size_t>(pp) * Hkv * page + slot;

  for (int r0 = grp; r0 < R; r0 += 32 * KVA_U) {
    i32x4 x1[KVA_U], x2[KVA_U];
    static_for<KVA_U>([&](auto u) {
      const int r = r0 + 32 * u;
      if (r < R) {
        x1[u] = *reinterpret_cast<const i32x4*>(src + r * KVA_D);
        x2[u] = *reinterpret_cast<const i32x4*>(src + r * KVA_D + KVA_D / 2);
      }
    });
    static_for<KVA_U>([&](auto u) {
      const int r = r0 + 32 * u;
      if (r >= R) return;
      if (r < Hq + Hkv) {
        float a[8], c[8], y1[8], y2[8];
        bf16x8_to_f32(x1[u], a);
        bf16x8_to_f32(x2[u], c);
#pragma unroll
        for (int e = 0; e < 8; ++e) rope_pair(a[e], c[e], cs[e], sn[e], y1[e], y2[e]);
        if (r < Hq) {
          uint16_t* const dst = qrow + r * KVA_D + 8 * j;
          *reinterpret_cast<i32x4*>(dst) = f32_to_bf16x8(y1);
          *reinterpret_cast<i32x4*>(dst + KVA_D / 2) = f32_to_bf16x8(y2);
        } else {
          uint8_t* const dst = Kc + (row0 + static_cast<size_t>(r - Hq) * page) * ROWB;
          if constexpr (FP8) {
            *reinterpret_cast<i32x2*>(dst + 8 * j) = f32_to_e4m3x8(y1, k_inv);
            *reinterpret_cast<i32x2*>(dst + KVA_D / 2 + 8 * j) = f32_to_e4m3x8(y2, k_inv);
          } else {
            *reinterpret_cast<i32x4*>(dst + 16 * j) = f32_to_bf16x8(y1);
            *reinterpret_cast<i32x4*>(dst + KVA_D + 16 * j) = f32_to_bf16x8(y2);
          }
        }
      } else {
        uint8_t* const dst = Vc + (row0 + static_cast<size_t>(r - Hq - Hkv) * page) * ROWB;
        if constexpr (FP8) {
          float a[8], c[8];
          bf16x8_to_f32(x1[u], a);
          bf16x8_to_f32(x2[u], c);
          *reinterpret_cast<i32x2*>(dst + 8 * j) = f32_to_e4m3x8(a, v_inv);
          *reinterpret_cast<i32x2*>(dst + KVA_D / 2 + 8 * j) = f32_to_e4m3x8(c, v_inv);
        } else {
          *reinterpret_cast<i32x4*>(dst + 16 * j) = x1[u];
          *reinterpret_cast<i32x4*>(dst + KVA_D + 16 * j) = x2[u];
        }
      }
    });
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct KvAppendArgs {
  int kind;
  const void* QKV;
  int64_t qkv_stride;
  void *Q_out, *K, *V;
  const void *block_table, *seq_lens;
  void* lens_out;
  const float *rope_cos, *rope_sin;
  int rope_len, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len;
  float k_inv_scale, v_inv_scale;
};

static bool kva_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + b_bytes && y < x + a_bytes;
}

// Everything the entry points refuse, before the first device call.
static int kva_validate(const char* who, const KvAppendArgs& a) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind != GSX_ATTN_KV_BF16 && a.kind != GSX_ATTN_KV_FP8) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (a.D != KVA_D) return refuse("need D == 128");
  if (a.Hq < 1 || a.Hq > 4096) return refuse("need 1 <= Hq <= 4096");
  if (a.Hkv < 1 || a.Hq % a.Hkv || a.Hq / a.Hkv > 16) return refuse("need Hq % Hkv == 0 and Hq / Hkv <= 16");
  if (a.page < 16 || a.page > 256 || a.page % 16) return refuse("need page % 16 == 0 and 16 <= page <= 256");
  if (a.B < 1 || a.T < 1) return refuse("need B >= 1 and T >= 1");
  if (static_cast<int64_t>(a.B) * a.T > INT32_MAX) return refuse("B * T must stay below 2^31");
  if (a.num_pages < 1) return refuse("need num_pages >= 1");
  if (a.table_stride < 1) return refuse("need table_stride >= 1");
  if (a.max_seq_len < 1) return refuse("need max_seq_len >= 1");
  if (static_cast<int64_t>(a.max_seq_len) > static_cast<int64_t>(a.table_stride) * a.page)
    return refuse("need max_seq_len <= table_stride * page");
  if (a.rope_len < a.max_seq_len) return refuse("need rope_len >= max_seq_len");
  const int64_t row = static_cast<int64_t>(a.Hq + 2 * a.Hkv) * KVA_D;
  if (a.qkv_stride < row || a.qkv_stride % 8)
    return refuse("need qkv_stride >= (Hq + 2 Hkv) * D and qkv_stride % 8 == 0");
  if (!a.QKV || !a.Q_out || !a.K || !a.V || !a.block_table || !a.seq_lens || !a.rope_cos || !a.rope_sin)
    return refuse("QKV, Q_out, K_cache, V_cache, block_table, seq_lens, rope_cos and rope_sin must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.QKV) | reinterpret_cast<uintptr_t>(a.Q_out) | reinterpret_cast<uintptr_t>(a.K) |
       reinterpret_cast<uintptr_t>(a.V) | reinterpret_cast<uintptr_t>(a.rope_cos) |
       reinterpret_cast<uintptr_t>(a.rope_sin)) % 16)
    return refuse("QKV, Q_out, K_cache, V_cache, rope_cos and rope_sin must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.block_table) | reinterpret_cast<uintptr_t>(a.seq_lens) |
       reinterpret_cast<uintptr_t>(a.lens_out)) % 4)
    return refuse("block_table, seq_lens and lens_out must be 4-B aligned");
  const uint64_t tokens = static_cast<uint64_t>(a.B) * a.T;
  if (kva_overlap(a.QKV, ((tokens - 1) * static_cast<uint64_t>(a.qkv_stride) + row) * 2, a.Q_out,
                  tokens * a.Hq * KVA_D * 2))
    return refuse("Q_out must not overlap QKV");
  if (a.lens_out && kva_overlap(a.lens_out, static_cast<uint64_t>(a.B) * 4, a.seq_lens, static_cast<uint64_t>(a.B) * 4))
    return refuse("lens_out must not overlap seq_lens");
  if (a.kind == GSX_ATTN_KV_BF16) {
    if (a.k_inv_scale != 1.0f || a.v_inv_scale != 1.0f)
      return refuse("a bf16 cache takes no scales: k_inv_scale and v_inv_scale must be 1.0");
  } else if (!std::isfinite(a.k_inv_scale) || !std::isfinite(a.v_inv_scale) || !(a.k_inv_scale > 0.f) ||
             !(a.v_inv_scale > 0.f)) {
    return refuse("k_inv_scale and v_inv_scale must be finite and > 0");
  }
  return 0;
}

template <bool FP8>
static int kva_launch(const char* who, hipStream_t s, const KvAppendArgs& a) {
  hipLaunchKernelGGL((kv_append_kernel<FP8>), dim3(a.B * a.T), dim3(KVA_THREADS), 0, s,
                     static_cast<const uint16_t*>(a.QKV), a.qkv_stride, static_cast<uint16_t*>(a.Q_out),
                     static_cast<uint8_t*>(a.K), static_cast<uint8_t*>(a.V),
                     static_cast<const int32_t*>(a.block_table), static_cast<const int32_t*>(a.seq_lens),
                     static_cast<int32_t*>(a.lens_out), a.rope_cos, a.rope_sin, a.T, a.Hq, a.Hkv, a.page, a.num_pages,
                     a.table_stride, a.max_seq_len, a.k_inv_scale, a.v_inv_scale);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

static int kva_run(const char* who, void* stream, const KvAppendArgs& a) {
  return a.kind == GSX_ATTN_KV_FP8 ? kva_launch<true>(who, S(stream), a) : kva_launch<false>(who, S(stream), a);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

int gsx_kv_append(void* stream, int kind, const void* QKV, int64_t qkv_stride, void* Q_out, void* K_cache,
                  void* V_cache, const void* block_table, const void* seq_lens, void* lens_out, const float* rope_cos,
                  const float* rope_sin, int rope_len, int B, int T, int Hq, int Hkv, int D, int page, int num_pages,
                  int table_stride, int max_seq_len, float k_inv_scale, float v_inv_scale) {
  const KvAppendArgs a{kind, QKV, qkv_stride, Q_out, K_cache, V_cache, block_table, seq_lens, lens_out, rope_cos,
                       rope_sin, rope_len, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len, k_inv_scale,
                       v_inv_scale};
  if (int rc = kva_validate("gsx_kv_append", a)) return rc;
  return kva_run("gsx_kv_append", stream, a);
}

int gsx_event_time_kv_append(void* stream, int kind, const void* QKV, int64_t qkv_stride, void* Q_out, void* K_cache,
                             void* V_cache, const void* block_table, const void* seq_lens, void* lens_out,
                             const float* rope_cos, const float* rope_sin, int rope_len, int B, int T, int Hq, int Hkv,
                             int D, int page, int num_pages, int table_stride, int max_seq_len, float k_inv_scale,
                             float v_inv_scale, int iters, float* ms) {
  const KvAppendArgs a{kind, QKV, qkv_stride, Q_out, K_cache, V_cache, block_table, seq_lens, lens_out, rope_cos,
                       rope_sin, rope_len, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len, k_inv_scale,
                       v_inv_scale};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = kva_validate("gsx_kv_append", a)) return rc;
  return event_time(stream, iters, ms, [&] { return kva_run("gsx_kv_append", stream, a); });
}

}  // extern "C"
