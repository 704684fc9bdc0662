// Decode attention for the pod workload: one new token per sequence, grouped-query attention (Hq query heads share
// Hkv KV heads in groups of G = Hq / Hkv <= 16) over a paged KV cache in bf16 or OCP e4m3, D = 128.  It is the other
// half of an inference server's decode step next to gemm_decode.hip: bound by HBM bandwidth, but reading 4 KiB-ish
// pages scattered through the pod's share and reached through a block table.  C ABI and numeric contract in
// gsx_kernels.h.
//
// attn_kernel: a workgroup owns one (sequence, KV head, split) and nothing passes between workgroups.
//   * The sequence's tokens are cut into tiles of 32; a split owns a contiguous run of tiles and the workgroup's W
//     waves take that run interleaved (wave w: tiles w, w + W, ...), so the workgroup walks its pages front to back.
//   * Both products are computed TRANSPOSED on v_mfma_f32_16x16x32_bf16, with the G query rows as the 16 COLUMNS:
//       S^T[t][g] = K[t][:] . Q[g][:]     A = K (a lane's row is a token, its 16-B chunk 8 consecutive d), B = Q
//       O^T[d][g] = V^T[d][:] . P^T[:][g] A = V^T, B = P^T
//     The result of the first lands in lane (fr, fq) as tokens 4 fq .. 4 fq + 3 of each 16-token half for query row
//     g = fr.  These 8 values are exactly the 8 k-slots of lane (fr, fq) of the second product's B operand once k-slot
//     (fq, e) is DEFINED as token 4 fq + e (e < 4) or 16 + 4 fq + e - 4: the order of a sum is free, so P needs no
//     move between lanes, only its rounding to bf16.  The softmax state (m, l) and the 32 accumulators of a lane all
//     belong to the one query row g = fr: the running maximum is two lane exchanges (xor 16, xor 32) per tile.
//     Rows G..15 of Q are zeros from a bounds-checked buffer load whose range is exactly the group's G rows.
//   * K goes from global memory to VGPRs in fragment shape with 16-B loads and never touches LDS.
//   * The V transposition.  V is token-major in memory and the PV product needs, per lane, 8 TOKENS of one d.  Of the
//     three ways (an in-register 8 x 8 transpose of 16-bit values over 8 lanes, three exchange rounds with byte
//     permutes per 16-B chunk; an operand order in which it is free, which does not exist for 16-B loads: a lane's
//     load holds one token, and the MFMA sums over what a lane holds; an LDS round trip) this file takes the LDS round
//     trip with ds_read_b64_tr_b16: V is loaded to VGPRs with 16-B loads, whole 256-B rows per 16 lanes, in the same
//     register ring as K, so the wait for HBM is the ring's; just before its MFMAs the wave writes the tile (e4m3
//     converted to bf16, slots at or past seq_len as zeros) into a wave-private [32][288 B] image and reads it back
//     transposed, 16 reads of 8 B per lane.  Rows are padded from 256 to 288 B: the 8 rows a 32-lane half reads
//     then start 8 banks apart and cover the 64 banks once.  No barrier: LDS executes one wave's instructions in
//     order; fences at wavefront scope keep the compiler from reordering them.  The transposed read needs EXEC all
//     ones: every branch around it is wave-uniform.
//   * A wave keeps F tiles in flight in a register ring (bf16: 64 VGPRs per tile; e4m3: 32) behind counted vmcnt
//     waits, structured as decode_kernel's ring.
//   * The waves' (m, l, acc) meet in LDS (the V images, reused) and are merged in wave order; with splits == 1 the
//     workgroup writes O, otherwise the triple goes to the workspace in fp32 and attn_merge_kernel, one small second
//     launch on the same stream, merges the splits in split order.
// Resources (hipcc -O3, gfx950; profiles/attn_decode/README.md has the table): no scratch in any instantiation, no
// atomics; LDS W * 9216 B (36864 B for 4 waves, 73728 B for 8).
// Offsets into the caches are 64-bit.  A page index is clamped into [0, num_pages) and a length to max_seq_len, so
// no content of block_table or seq_lens makes the kernel read outside the caches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) i16x4* lds_i16x4_t;

constexpr int AT_D = 128;           // head dimension
constexpr int AT_TILE = 32;         // tokens per tile: the k of one PV MFMA
constexpr int AT_VROW = 288;        // bytes of a row of the V image in LDS: 256 + 32 of padding
constexpr int AT_WAVE_LDS = AT_TILE * AT_VROW;  // 9216: a wave's V image, later its (acc, m, l)
constexpr int AT_NF = AT_D / 16;    // output fragments of 16 d
constexpr int AT_MAX_SPLITS = 64;

// A raw buffer over `bytes` bytes at `base`: a load at or past the end returns zeros and touches nothing.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t attn_rows_buffer(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, static_cast<int>(bytes), 0x00020000);
}

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

template <bool FP8, int W, int F>
__global__ __launch_bounds__(W * 64) void attn_kernel(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kc,
                                                     const uint8_t* __restrict__ Vc,
                                                     const int32_t* __restrict__ block_table,
                                                     const int32_t* __restrict__ seq_lens, uint16_t* __restrict__ O,
                                                     float* __restrict__ ws_acc, float* __restrict__ ws_ml, int Hq,
                                                     int Hkv, int page, int num_pages, int table_stride,
                                                     int max_seq_len, int splits, float qk_scale, float v_scale) {
  constexpr int ROWB = FP8 ? AT_D : 2 * AT_D;  // bytes of a token's row in the cache
  constexpr int NCK = ROWB / 64;               // 16-B chunks of K a lane loads per 16-token half
  constexpr int NV = ROWB / 32;                // 16-B chunks of V a lane loads per tile
  constexpr int VLPR = ROWB / 16;              // lanes that share a row of V in one load
  constexpr int VROWS = 64 / VLPR;             // rows of V one load instruction covers
  constexpr float NEG_INF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[W * AT_WAVE_LDS];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int G = Hq / Hkv;
  const int split = blockIdx.x % splits;
  const int pair = blockIdx.x / splits;
  const int kvh = pair % Hkv, b = pair / Hkv;

  int len = seq_lens[b];
  len = len < 0 ? 0 : len > max_seq_len ? max_seq_len : len;
  const int nt = (len + AT_TILE - 1) / AT_TILE;
  const int tps = (nt + splits - 1) / splits;  // tiles per split
  const int t0 = split * tps;
  const int t1 = t0 + tps < nt ? t0 + tps : nt;
  const int mine = t0 + wid < t1 ? (t1 - t0 - wid + W - 1) / W : 0;  // tiles t0 + wid, t0 + wid + W, ...
  const int32_t* bt = block_table + static_cast<size_t>(b) * table_stride;

  // Q: row g of the group is the lane's column fr.  k-step s of the first product covers, per lane, the 8 d of
  // chunk 4 s + fq (bf16), or of the half (s & 1) of the cache's 16-B chunk 4 (s >> 1) + fq (e4m3, 16 d per chunk)
  bf16x8 qf[4];
  {
    const __amdgpu_buffer_rsrc_t qbuf =
        attn_rows_buffer(Q + (static_cast<size_t>(b) * Hq + static_cast<size_t>(kvh) * G) * AT_D, G * AT_D * 2);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d0 = FP8 ? 16 * (4 * (s >> 1) + fq) + 8 * (s & 1) : 8 * (4 * s + fq);
      qf[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(qbuf, fr * AT_D * 2 + d0 * 2, 0, 0));
    }
  }

  // the ring: slot i holds one tile's chunks of K (two halves of 16 tokens) and of V
  i32x4 rk[F][2][NCK], rv[F][NV];

  auto load = [&](auto slot, int j) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + wid + j * W) * AT_TILE;
    // The first row of each half, in rows of the cache.  A half lies in one page (page % 16 == 0).  The second half
    // of the sequence's last tile can lie wholly past seq_len, where the block table need not have an entry: it
    // then reads what the first half reads, and is masked.
    size_t row[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tok0 = tb + 16 * h < len ? tb + 16 * h : tb;
      const int lp = tok0 / page;
      uint32_t pp = static_cast<uint32_t>(bt[lp]);
      pp = pp < static_cast<uint32_t>(num_pages - 1) ? pp : static_cast<uint32_t>(num_pages - 1);
      row[h] = (static_cast<size_t>(pp) * Hkv + kvh) * page + (tok0 - lp * page);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < NCK; ++c)
        rk[i][h][c] = *reinterpret_cast<const i32x4*>(Kc + (row[h] + fr) * ROWB + (4 * c + fq) * CHUNK);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int r = c * VROWS + lane / VLPR;  // the row of the tile
      rv[i][c] = *reinterpret_cast<const i32x4*>(Vc + (row[r >> 4] + (r & 15)) * ROWB + (lane % VLPR) * CHUNK);
    }
  };

  float m = NEG_INF, l = 0.f;  // l: the lane's part, the sum over its own 8 tokens of every tile
  f32x4 acc[AT_NF];
#pragma unroll
  for (int n = 0; n < AT_NF; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  char* const vl = lds + wid * AT_WAVE_LDS;
  // the transposed read: lane 4 q + p of a group of 16 names row q, columns 4 p .. 4 p + 3 of a 4 x 16 block and
  // lane i receives column i of the 4 rows.  Group fq reads rows (tokens) 4 fq .. 4 fq + 3 and, 16 rows on, the same
  // of the second half; the block's 16 columns are d = 16 n .. 16 n + 15
  const char* const vtr = vl + (4 * fq + (fr >> 2)) * AT_VROW + (fr & 3) * 8;

  auto compute = [&](auto slot, int j) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + wid + j * W) * AT_TILE;

    // S^T = K Q^T for both halves
    f32x4 s[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        bf16x8 kf;
        if constexpr (FP8) {
          const i32x4 raw = rk[i][h][st >> 1];
          kf = __builtin_bit_cast(bf16x8, (st & 1) ? fp8x8_to_bf16x8(raw[2], raw[3]) : fp8x8_to_bf16x8(raw[0], raw[1]));
        } else {
          kf = __builtin_bit_cast(bf16x8, rk[i][h][st]);
        }
        s[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[st], s[h], 0, 0, 0);
      }
    }

    // the lane's 8 tokens of query row fr: x, masked by select (a NaN from a slot past seq_len goes with it)
    float x[8];
    float mx = NEG_INF;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int tok = tb + 16 * (e >> 2) + 4 * fq + (e & 3);
      x[e] = tok < len ? s[e >> 2][e & 3] * qk_scale : NEG_INF;
      mx = fmaxf(mx, x[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float ms = mn == NEG_INF ? 0.f : mn;  // every x at -inf: p = exp2(-inf) = 0, not exp2(-inf + inf)
    const float alpha = __builtin_amdgcn_exp2f(m - ms);
    m = mn;
    float p[8], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = __builtin_amdgcn_exp2f(x[e] - ms);
      ps += p[e];
    }
    l = l * alpha + ps;
    bf16x8 pf;
#pragma unroll
    for (int e = 0; e < 8; ++e) pf[e] = static_cast<__bf16>(p[e]);  // round to nearest even
#pragma unroll
    for (int n = 0; n < AT_NF; ++n)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[n][jj] *= alpha;

    // V into the wave's image: zeros for a slot at or past seq_len (0 * NaN in the MFMA would be NaN)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // behind the previous tile's reads
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int r = c * VROWS + lane / VLPR;
      const bool ok = tb + r < len;
      const i32x4 raw = ok ? rv[i][c] : i32x4{0, 0, 0, 0};
      char* const dst = vl + r * AT_VROW + (lane % VLPR) * (FP8 ? 2 * CHUNK : CHUNK);
      if constexpr (FP8) {
        *reinterpret_cast<i32x4*>(dst) = fp8x8_to_bf16x8(raw[0], raw[1]);
        *reinterpret_cast<i32x4*>(dst + CHUNK) = fp8x8_to_bf16x8(raw[2], raw[3]);
      } else {
        *reinterpret_cast<i32x4*>(dst) = raw;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int n = 0; n < AT_NF; ++n) {
      const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + n * 32));
      const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + 16 * AT_VROW + n * 32));
      const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[n], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  // The ring of decode_kernel: slot i holds tile t + i until it is consumed, then tile t + i + F.  The steady loop
  // has no condition inside and is entered behind an unconditional prologue; the last 2 F - 1 tiles or fewer drain
  // in two conditional passes.  Every condition is wave-uniform.
  int t = 0;
  if (mine >= 2 * F) {
    static_for<F>([&](auto i) {
      load(i, i);
      __builtin_amdgcn_sched_barrier(0);
    });
    do {
      static_for<F>([&](auto i) {
        compute(i, t + i);
        load(i, t + i + F);
        __builtin_amdgcn_sched_barrier(0);
      });
      t += F;
    } while (t + 2 * F <= mine);
  } else {
    static_for<F>([&](auto i) {
      if (i < mine) load(i, i);
    });
  }
  static_for<F>([&](auto i) {
    if (t + i < mine) {
      compute(i, t + i);
      if (t + i + F < mine) load(i, t + i + F);
    }
  });
  static_for<F>([&](auto i) {
    if (t + F + i < mine) compute(i, t + F + i);
  });

  // The waves' partials meet in LDS, each in its own image: acc as [n][j][lane], then m and the lane's part of l.
  // A wave without a tile contributes m = -inf, l = 0 and zeros.
  {
    float* const mine_f = reinterpret_cast<float*>(vl);
#pragma unroll
    for (int n = 0; n < AT_NF; ++n)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) mine_f[(n * 4 + jj) * 64 + lane] = acc[n][jj];
    mine_f[32 * 64 + lane] = m;
    mine_f[33 * 64 + lane] = l;
  }
  __syncthreads();

  // every wave merges, in wave order, the output fragments n = wid, wid + W, ...; all of them compute M and L
  float mw[W], M = NEG_INF;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    mw[w] = reinterpret_cast<const float*>(lds + w * AT_WAVE_LDS)[32 * 64 + lane];
    M = fmaxf(M, mw[w]);
  }
  float L = 0.f, aw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const float* lw = reinterpret_cast<const float*>(lds + w * AT_WAVE_LDS) + 33 * 64;
    const float lsum = ((lw[fr] + lw[16 + fr]) + lw[32 + fr]) + lw[48 + fr];
    aw[w] = merge_weight(mw[w], M);
    L += aw[w] * lsum;
  }
  const bool grow = fr < G;
  const size_t hq = static_cast<size_t>(b) * Hq + static_cast<size_t>(kvh) * G + fr;  // the lane's row of Q and O
  for (int n = wid; n < AT_NF; n += W) {
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const float* aw_f = reinterpret_cast<const float*>(lds + w * AT_WAVE_LDS);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) o[jj] += aw[w] * aw_f[(n * 4 + jj) * 64 + lane];
    }
    if (!grow) continue;
    const int d0 = 16 * n + 4 * fq;  // O^T map: row (d) 4 fq + j, column (g) fr
    if (splits == 1) {
      uint16_t r[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) r[jj] = L > 0.f || L != L ? f2bf((o[jj] / L) * v_scale) : uint16_t{0};
      *reinterpret_cast<i32x2*>(O + hq * AT_D + d0) =
          i32x2{static_cast<int>(r[0] | (static_cast<uint32_t>(r[1]) << 16)),
                static_cast<int>(r[2] | (static_cast<uint32_t>(r[3]) << 16))};
    } else {
      const size_t at = hq * splits + split;
      *reinterpret_cast<f32x4*>(ws_acc + at * AT_D + d0) = o;
      if (n == 0 && fq == 0) {
        ws_ml[at * 2] = M;
        ws_ml[at * 2 + 1] = L;
      }
    }
  }
}

// One workgroup of 128 threads per (sequence, query head): thread d merges the splits' partials in split order.
__global__ __launch_bounds__(AT_D) void attn_merge_kernel(const float* __restrict__ ws_acc,
                                                          const float* __restrict__ ws_ml, uint16_t* __restrict__ O,
                                                          int splits, float v_scale) {
  const size_t at = static_cast<size_t>(blockIdx.x) * splits;
  const int d = threadIdx.x;
  float M = -__builtin_inff();
  for (int s = 0; s < splits; ++s) M = fmaxf(M, ws_ml[(at + s) * 2]);
  float L = 0.f, o = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float a = merge_weight(ws_ml[(at + s) * 2], M);
    L += a * ws_ml[(at + s) * 2 + 1];
    o += a * ws_acc[(at + s) * AT_D + d];
  }
  O[static_cast<size_t>(blockIdx.x) * AT_D + d] = L > 0.f || L != L ? f2bf((o / L) * v_scale) : uint16_t{0};
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

constexpr int kAttnKinds = 2;

struct AttnArgs {
  int kind;
  const void *Q, *K, *V, *block_table, *seq_lens;
  void* O;
  int B, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len;
  float scale, k_scale, v_scale;
  void* workspace;
  uint64_t workspace_bytes;
};

// fp32 partials of `splits` splits: acc[B][Hq][splits][128], then (m, l)[B][Hq][splits]
static uint64_t attn_ws_bytes(int B, int Hq, int splits) {
  return splits <= 1 ? 0 : static_cast<uint64_t>(B) * Hq * splits * (AT_D + 2) * sizeof(float);
}

// What the shape arguments alone can get wrong (no pointers): shared by the launchers and the workspace query.
static int attn_validate_shape(const char* who, int B, int Hq, int D, int page, int max_seq_len) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (D != AT_D) return refuse("need D == 128");
  if (B < 1 || B > (1 << 20)) return refuse("need 1 <= B <= 2^20");
  if (Hq < 1 || Hq > 4096) return refuse("need 1 <= Hq <= 4096");
  if (static_cast<int64_t>(B) * Hq > INT32_MAX) return refuse("B * Hq must stay below 2^31");  // the merge's grid
  if (page < 16 || page > 256 || page % 16) return refuse("need page % 16 == 0 and 16 <= page <= 256");
  if (max_seq_len < 1) return refuse("need max_seq_len >= 1");
  return 0;
}

// Everything the entry points refuse, before the first device call.
static int attn_validate(const char* who, const AttnArgs& a, int splits) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind < 0 || a.kind >= kAttnKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (int rc = attn_validate_shape(who, a.B, a.Hq, a.D, a.page, a.max_seq_len)) return rc;
  if (a.Hkv < 1 || a.Hq % a.Hkv || a.Hq / a.Hkv > 16) return refuse("need Hq % Hkv == 0 and Hq / Hkv <= 16");
  if (a.num_pages < 1) return refuse("need num_pages >= 1");
  if (a.table_stride < 1) return refuse("need table_stride >= 1");
  if (static_cast<int64_t>(a.max_seq_len) > static_cast<int64_t>(a.table_stride) * a.page)
    return refuse("need max_seq_len <= table_stride * page");
  if (!a.Q || !a.K || !a.V || !a.O || !a.block_table || !a.seq_lens)
    return refuse("Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.Q) | reinterpret_cast<uintptr_t>(a.K) | reinterpret_cast<uintptr_t>(a.V) |
       reinterpret_cast<uintptr_t>(a.O)) % 16)
    return refuse("Q, K_cache, V_cache and O must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.block_table) | reinterpret_cast<uintptr_t>(a.seq_lens)) % 4)
    return refuse("block_table and seq_lens must be 4-B aligned");
  if (!std::isfinite(a.scale) || !std::isfinite(a.k_scale) || !std::isfinite(a.v_scale))
    return refuse("scale, k_scale and v_scale must be finite");
  if (a.kind == GSX_ATTN_KV_BF16 && (a.k_scale != 1.0f || a.v_scale != 1.0f))
    return refuse("a bf16 cache takes no scales: k_scale and v_scale must be 1.0");
  if (splits < 1 || splits > AT_MAX_SPLITS) return refuse("need 1 <= splits <= 64");
  if (static_cast<int64_t>(a.B) * a.Hkv * splits > INT32_MAX) return refuse("B * Hkv * splits must stay below 2^31");
  const uint64_t need = attn_ws_bytes(a.B, a.Hq, splits);
  if (need) {
    if (!a.workspace || a.workspace_bytes < need) {
      std::snprintf(msg, sizeof(msg), "%s: workspace too small: %d splits need %llu bytes", who, splits,
                    static_cast<unsigned long long>(need));
      return fail_arg(msg);
    }
    if (reinterpret_cast<uintptr_t>(a.workspace) % 16) return refuse("workspace must be 16-B aligned");
  }
  return 0;
}

using attn_launch_t = int (*)(const char* who, hipStream_t s, const AttnArgs& a, int splits);

template <bool FP8, int W, int F>
int attn_launch(const char* who, hipStream_t s, const AttnArgs& a, int splits) {
  float* ws_acc = static_cast<float*>(a.workspace);
  float* ws_ml = ws_acc ? ws_acc + static_cast<size_t>(a.B) * a.Hq * splits * AT_D : nullptr;
  if (splits == 1) ws_acc = ws_ml = nullptr;
  const float qk_scale = (a.scale * a.k_scale) * 1.4426950408889634f;
  hipLaunchKernelGGL((attn_kernel<FP8, W, F>), dim3(a.B * a.Hkv * splits), dim3(W * 64), 0, s,
                     static_cast<const uint16_t*>(a.Q), static_cast<const uint8_t*>(a.K),
                     static_cast<const uint8_t*>(a.V), static_cast<const int32_t*>(a.block_table),
                     static_cast<const int32_t*>(a.seq_lens), static_cast<uint16_t*>(a.O), ws_acc, ws_ml, a.Hq, a.Hkv,
                     a.page, a.num_pages, a.table_stride, a.max_seq_len, splits, qk_scale, a.v_scale);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, who);
  if (splits > 1) {
    hipLaunchKernelGGL(attn_merge_kernel, dim3(a.B * a.Hq), dim3(AT_D), 0, s, ws_acc, ws_ml,
                       static_cast<uint16_t*>(a.O), splits, a.v_scale);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e, who);
  }
  return 0;
}

struct AttnCfg {
  const char* name;
  int waves, inflight;
  attn_launch_t launch[kAttnKinds];  // indexed by GSX_ATTN_KV_*
};
template <int W, int F>
constexpr AttnCfg attn_cfg(const char* name) {
  return {name, W, F, {&attn_launch<false, W, F>, &attn_launch<true, W, F>}};
}

// name: waves per workgroup - tiles of 32 tokens a wave keeps in flight
constexpr AttnCfg kAttnCfgs[] = {
    attn_cfg<4, 1>("4w-f1"),
    attn_cfg<4, 2>("4w-f2"),
    attn_cfg<8, 1>("8w-f1"),
    attn_cfg<8, 2>("8w-f2"),
};
constexpr int kNumAttnCfgs = sizeof(kAttnCfgs) / sizeof(kAttnCfgs[0]);

static const AttnCfg* attn_row(int cfg) { return cfg >= 0 && cfg < kNumAttnCfgs ? &kAttnCfgs[cfg] : nullptr; }

// The dispatch rule, from the (sequence, KV head) pairs and max_seq_len alone (a stream's CU mask is not known here,
// and the lengths are in device memory):
//   configuration "8w-f1" for both cache types;
//   splits = ceil(256 / pairs), one workgroup of 8 waves for each of the 256 CUs, but no more than leave every wave
//   of a split 4 tiles (max_seq_len / 1024), and at most 64.
// Measured on one MI355X on a ring of per-layer caches of more than 1 GiB, pages of 16 tokens in random order, TB/s
// of KV bytes by splits (profiles/attn_decode/README.md has every configuration, torch and the read yardstick):
//                                  pairs  splits: 1     2     4     8     16    32    64    rule
//   bf16  B 1   x 32768, 64/8 heads     8         0.36  0.69  1.29  2.21  3.28  3.51  2.62  32
//   bf16  B 8   x 8192,  64/8          64         2.55  4.19  5.16  4.78  4.24  3.53  2.57   4
//   bf16  B 64  x 2048,  64/8         512         5.57  5.24  4.91  4.21  3.14  2.10         1
//   bf16  B 1   x 32768, 32/32         32         1.43  2.69  4.42  5.50  5.29  4.80  4.02   8
//   bf16  B 8   x 8192,  32/32        256         5.58  5.63  5.65  5.38  5.16  4.35  3.33   1
//   fp8   B 1   x 32768, 64/8           8         0.27  0.52  0.96  1.63  2.33  2.44  1.78  32
//   fp8   B 8   x 8192,  64/8          64         1.97  3.30  4.33  4.02  3.68  2.99  2.09   4
//   fp8   B 1   x 32768, 32/32         32         1.07  2.02  3.37  4.84  4.48  4.25  3.68   8
// Fewer workgroups than CUs leave CUs idle; more only add partials to write, read and merge.  In every row above
// ceil(256 / pairs) decides.  The cap of 4 tiles per wave decides for one short sequence, and there it is too tight
// (bench section attn_decode_short, 64/8 heads, "8w-f1"):
//   bf16  B 1   x 8192                      8         0.34  0.60  1.02  1.50  1.74  1.58  0.99   8  (14 % behind s16)
//   bf16  B 1   x 4096                      8         0.32  0.53  0.81  1.09  1.14  0.93  0.54   4  (29 % behind s16)
//   fp8   B 1   x 8192                      8         0.25  0.44  0.71  0.98  1.09  0.91  0.58   8  (10 % behind s16)
//   fp8   B 1   x 4096                      8         0.23  0.37  0.54  0.67  0.62  0.49  0.30   4  (19 % behind s8)
// A cap of 2 tiles per wave would have picked the best cell in three of these rows and 4 % less in the fourth and
// would change none of the rows further up; it has not been run through the tests on a GPU, so the rule stands as
// measured.  Among the
// configurations the spread at the best split count is a few per cent in bf16 ("8w-f2" ahead by 0 to 2 % at 64/8
// heads); for e4m3 "8w-f2" is 7 to 20 % behind at large batches (165 VGPRs against 121: a workgroup of 8 waves is 2
// waves per SIMD, so one workgroup per CU fits instead of two, 2 waves per SIMD instead of 4) and "8w-f1" is the best
// in 7 of 8 shapes (2 % behind in the eighth), so one rule serves both.
static void attn_pick(int64_t pairs, int max_seq_len, int* cfg, int* splits) {
  const int tiles = (max_seq_len + AT_TILE - 1) / AT_TILE;
  *cfg = 2;
  const int w = kAttnCfgs[*cfg].waves;
  int64_t want = (256 + pairs - 1) / pairs;
  const int most = tiles / (4 * w);
  if (want > most) want = most;
  if (want > AT_MAX_SPLITS) want = AT_MAX_SPLITS;
  *splits = want < 1 ? 1 : static_cast<int>(want);
}

static AttnArgs attn_args(int kind, const void* Q, const void* K, const void* V, const void* block_table,
                          const void* seq_lens, void* O, int B, int Hq, int Hkv, int D, int page, int num_pages,
                          int table_stride, int max_seq_len, float scale, float k_scale, float v_scale,
                          void* workspace, uint64_t workspace_bytes) {
  return {kind, Q, K, V, block_table, seq_lens, O, B, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len,
          scale, k_scale, v_scale, workspace, workspace_bytes};
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_decode_attn_cfg_name(int cfg) { return attn_row(cfg) ? attn_row(cfg)->name : nullptr; }

int gsx_decode_attn_cfg_shape(int cfg, int* waves, int* inflight) {
  const AttnCfg* c = attn_row(cfg);
  if (!c) return -1;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_decode_attn_workspace_bytes(int B, int Hq, int D, int page, int max_seq_len, uint64_t* bytes) {
  const char* who = "gsx_decode_attn_workspace_bytes";
  if (!bytes) return fail_arg("gsx_decode_attn_workspace_bytes: bytes must not be NULL");
  if (int rc = attn_validate_shape(who, B, Hq, D, page, max_seq_len)) return rc;
  // Hkv is not known here: the fewest KV heads Hq allows (groups of 16) give the fewest pairs and the most splits
  int cfg = 0, splits = 1;
  attn_pick(static_cast<int64_t>(B) * ((Hq + 15) / 16), max_seq_len, &cfg, &splits);
  *bytes = attn_ws_bytes(B, Hq, splits);
  return 0;
}

int gsx_decode_attn_launch_cfg(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                               const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D,
                               int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                               float v_scale, void* workspace, uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_decode_attn_launch_cfg";
  const AttnCfg* c = attn_row(cfg);
  if (!c) return fail_arg("gsx_decode_attn_launch_cfg: unknown config");
  const AttnArgs a = attn_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, Hq, Hkv, D, page, num_pages,
                               table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  if (int rc = attn_validate(who, a, splits)) return rc;
  return c->launch[kind](who, S(stream), a, splits);
}

// What the dispatching entry point will run, or why it refuses: no device call.
static int attn_plan(const char* who, const AttnArgs& a, int* cfg, int* splits) {
  if (int rc = attn_validate(who, a, 1)) return rc;  // everything but the workspace
  attn_pick(static_cast<int64_t>(a.B) * a.Hkv, a.max_seq_len, cfg, splits);
  return attn_validate(who, a, *splits);
}

static int attn_dispatch(const char* who, void* stream, const AttnArgs& a) {
  int cfg = 0, splits = 1;
  if (int rc = attn_plan(who, a, &cfg, &splits)) return rc;
  return kAttnCfgs[cfg].launch[a.kind](who, S(stream), a, splits);
}

int gsx_decode_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                    const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D, int page,
                    int num_pages, int table_stride, int max_seq_len, float scale, float k_scale, float v_scale,
                    void* workspace, uint64_t workspace_bytes) {
  const AttnArgs a = attn_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, Hq, Hkv, D, page, num_pages,
                               table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  return attn_dispatch("gsx_decode_attn", stream, a);
}

int gsx_event_time_decode_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                               const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D,
                               int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                               float v_scale, void* workspace, uint64_t workspace_bytes, int iters, float* ms) {
  const AttnArgs a = attn_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, Hq, Hkv, D, page, num_pages,
                               table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  // refused before the events are made, under the name of the entry point that is timed
  int cfg = 0, splits = 1;
  if (int rc = attn_plan("gsx_decode_attn", a, &cfg, &splits)) return rc;
  return event_time(stream, iters, ms, [&] { return attn_dispatch("gsx_decode_attn", stream, a); });
}

}  // extern "C"
