// Causal prefill attention for the pod workload: T new tokens per sequence attend over the paged KV cache that
// gsx_kv_append has just extended (bf16 or OCP e4m3, D = 128, grouped-query heads).  It is the compute-bound
// counterpart of attn_decode.hip.  C ABI and numeric contract in gsx_kernels.h.
//
// prefill_kernel: a workgroup of 8 waves owns one (sequence, query head, block of 256 query rows) and nothing passes
// between workgroups.  A wave owns 32 of the rows; the workgroup walks the sequence's tokens front to back in tiles
// of 64, up to the tile that holds the position of its last live row.
//   * Both products run on v_mfma_f32_32x32x16_bf16 with the wave's 32 query rows as the 32 COLUMNS:
//       S^T[tok][q] = K[tok][:] . Q[q][:]     A = K (a lane's row is a token, its 16-B chunk 8 consecutive d), B = Q
//       O^T[d][q]   = V^T[d][:] . P^T[:][q]   A = V^T, B = P^T
//     Lane (r, h) = (lane & 31, lane >> 5) then holds, for query row r, the scores of 16 of each 32 tokens (token
//     (i & 3) + 8 (i >> 2) + 4 h in register i), later all 128 d of that row's accumulator in halves by h, and the
//     row's m, l and rescale factor as plain scalars.  A row's maximum is 31 fmax and one v_permlane32_swap with the
//     lane that holds its other 16 tokens; its l is kept per lane and the two halves meet once, at the end.
//     Registers 8 s .. 8 s + 7 of a score tile, rounded to bf16, ARE the B fragment of k-step s of the second
//     product, with k-slot j of lane half h DEFINED as token 16 s + 8 (j >> 2) + 4 h + (j & 3): the order of a sum is
//     free, so P never moves between lanes.  The A fragment follows the same order: two transposed reads of V.
//   * Q stays in registers (8 fragments of 16 B per lane).
//   * K and V tiles are double-buffered in LDS and written from registers: the loads of tile j + 1 are issued before
//     the products of tile j and written to the other buffer after them, one barrier per tile.  e4m3 is converted to
//     bf16 on the way into LDS (exact).  A 16-token run of a tile lies in one page (page % 16 == 0); every thread
//     looks up the page of the run its row belongs to.
//   * K image: 256-B rows, chunk c of row t at position c ^ (t & 15): the 16 rows a ds_read_b128 serves at a time hit
//     16 different chunks.  V image: rows padded to 320 B, read back with ds_read_b64_tr_b16: the 4 rows of 64 B a
//     32-lane half reads start 16 banks apart and cover the 64 banks once.
//   * A wave skips the tiles wholly above its last live row, and applies the causal mask, a select, only on tiles
//     that reach above its first row.  V of tokens past the workgroup's last live row is written to LDS as zeros
//     (0 * NaN in the MFMA would be NaN).
//   * Late query blocks, which have the most tiles, get the lowest workgroup ids.
// Resources (hipcc -O3, gfx950; profiles/attn_prefill/README.md has the table): no scratch, no atomics, LDS 73728 B.
// Offsets into the caches are 64-bit.  A page index is clamped into [0, num_pages) and a length to max_seq_len, and
// block-table entries past the page of the workgroup's last live row are never read.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

// No fp32 multiply is fused with a following add or subtract in this file: x = s * c and x - m round separately, as
// the contract has them, in the masked and in the unmasked instantiation of a tile alike.  With contraction on, the
// compiler fused them in one and not in the other, and a row's bits depended on which rows shared its wave.
#pragma clang fp contract(off)

namespace gsxgemm {
namespace {

typedef short pf_i16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) pf_i16x4* pf_lds_i16x4_t;

constexpr int PF_D = 128;                        // head dimension
constexpr int PF_WAVES = 8;                      // waves per workgroup
constexpr int PF_WROWS = 32;                     // query rows per wave: the columns of one MFMA
constexpr int PF_QROWS = PF_WAVES * PF_WROWS;    // query rows per workgroup
constexpr int PF_KV = 64;                        // tokens per KV tile
constexpr int PF_THREADS = PF_WAVES * 64;
constexpr int PF_KROW = 2 * PF_D;                // bytes of a row of the K image
constexpr int PF_VROW = 2 * PF_D + 64;           // bytes of a row of the V image: 256 + 64 of padding
constexpr int PF_KBYTES = PF_KV * PF_KROW;       // 16384
constexpr int PF_VBYTES = PF_KV * PF_VROW;       // 20480
constexpr int PF_STAGE = PF_KBYTES + PF_VBYTES;  // one buffer: a K image, then a V image
constexpr int PF_LDS = 2 * PF_STAGE;             // 73728

// two e4m3 bytes of `w` (the low pair, or the high pair) as two bf16 in one dword; the conversion is exact
__device__ __forceinline__ int pf_fp8x2_to_bf16x2(int w, bool hi) {
  const auto f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true) : __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  return static_cast<int>((__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u));
}
// 8 e4m3 bytes (two dwords) as 8 bf16
__device__ __forceinline__ i32x4 pf_fp8x8_to_bf16x8(int lo, int hi) {
  return i32x4{pf_fp8x2_to_bf16x2(lo, false), pf_fp8x2_to_bf16x2(lo, true), pf_fp8x2_to_bf16x2(hi, false),
               pf_fp8x2_to_bf16x2(hi, true)};
}

// v of this lane and v of lane ^ 32, in an order that is the same for both lanes of a pair only up to exchange: use
// them in a commutative operation.  v_permlane32_swap exchanges the upper half of its first operand with the lower
// half of its second.
__device__ __forceinline__ void pf_pair(float v, float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

template <bool FP8>
__global__ __launch_bounds__(PF_THREADS) void prefill_kernel(
    const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kc, const uint8_t* __restrict__ Vc,
    const int32_t* __restrict__ block_table, const int32_t* __restrict__ seq_lens, uint16_t* __restrict__ O, int B,
    int T, int Hq, int Hkv, int page, int num_pages, int table_stride, int max_seq_len, int nqb, float qk_scale,
    float v_scale) {
  constexpr int ROWB = FP8 ? PF_D : 2 * PF_D;  // bytes of a token's row in the cache
  constexpr int LPR = ROWB / CHUNK;            // threads that share a row in one round of loads
  constexpr int RPR = PF_THREADS / LPR;        // rows one round of loads covers
  constexpr int NLD = PF_KV / RPR;             // rounds per tile: 16-B chunks of K, and of V, a thread stages
  constexpr float NEG_INF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[PF_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  // late query blocks first
  int bid = blockIdx.x;
  const int hq = bid % Hq;
  bid /= Hq;
  const int b = bid % B;
  const int qb = nqb - 1 - bid / B;
  const int kvh = hq / (Hq / Hkv);

  int base = seq_lens[b];
  base = base < 0 ? 0 : base > max_seq_len ? max_seq_len : base;
  const int32_t* bt = block_table + static_cast<size_t>(b) * table_stride;

  // the workgroup: rows t0 .. tl of the chunk; pmax is the position of its last live row
  const int t0 = qb * PF_QROWS;
  const int tl = (T - t0 < PF_QROWS ? T - t0 : PF_QROWS) - 1 + t0;
  const bool wg_any = static_cast<int64_t>(base) + t0 < max_seq_len;
  const int64_t plast = static_cast<int64_t>(base) + tl;
  const int pmax = plast < max_seq_len ? static_cast<int>(plast) : max_seq_len - 1;
  const int ntiles = wg_any ? pmax / PF_KV + 1 : 0;

  // the wave: rows tw0 .. tw0 + 31; positions pw_min .. pw_max of its live rows
  const int tw0 = t0 + wid * PF_WROWS;
  const bool wave_any = tw0 < T && static_cast<int64_t>(base) + tw0 < max_seq_len;
  const int twl = T - 1 < tw0 + PF_WROWS - 1 ? T - 1 : tw0 + PF_WROWS - 1;
  const int64_t pwl = static_cast<int64_t>(base) + twl;
  const int pw_max = pwl < max_seq_len ? static_cast<int>(pwl) : max_seq_len - 1;
  const int64_t pw_min = static_cast<int64_t>(base) + tw0;

  // the lane's query row: a row that is not live sees no token (pos = -1)
  const int t = tw0 + r;
  const bool row_ok = t < T;
  const bool live = row_ok && static_cast<int64_t>(base) + t < max_seq_len;
  const int pos = live ? base + t : -1;
  const size_t qrow = static_cast<size_t>(b) * T + (row_ok ? t : T - 1);  // a row past the chunk reads the last one

  // Q: k-step s of the first product covers, per lane, d = 16 s + 8 h .. + 7 of query row r
  bf16x8 qf[8];
  {
    const uint16_t* qp = Q + (qrow * Hq + hq) * PF_D + 8 * h;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
  }

  // the staging registers: round c holds chunk tid % LPR of row c * RPR + tid / LPR of the tile, of K and of V
  i32x4 rk[NLD], rv[NLD];
  const int ld_row = tid / LPR, ld_ch = tid % LPR;

  auto gload = [&](int j) {
#pragma unroll
    for (int c = 0; c < NLD; ++c) {
      const int row = c * RPR + ld_row;
      // The first token of the row's run of 16.  A run wholly past pmax, where the block table need not have an
      // entry, reads what the tile's first run reads, and is masked.
      int tok0 = j * PF_KV;
      if (pmax - tok0 >= (row & ~15)) tok0 += row & ~15;
      const int lp = tok0 / page;
      uint32_t pp = static_cast<uint32_t>(bt[lp]);
      pp = pp < static_cast<uint32_t>(num_pages - 1) ? pp : static_cast<uint32_t>(num_pages - 1);
      const size_t at =
          (((static_cast<size_t>(pp) * Hkv + kvh) * page + (tok0 - lp * page)) + (row & 15)) * ROWB + ld_ch * CHUNK;
      rk[c] = *reinterpret_cast<const i32x4*>(Kc + at);
      rv[c] = *reinterpret_cast<const i32x4*>(Vc + at);
    }
  };

  auto lstore = [&](int j, int buf) {
    char* const kb = lds + buf * PF_STAGE;
    char* const vb = kb + PF_KBYTES;
#pragma unroll
    for (int c = 0; c < NLD; ++c) {
      const int row = c * RPR + ld_row;
      const bool past = pmax - j * PF_KV < row;  // a token no row of the workgroup sees: V as zeros
      const i32x4 v = past ? i32x4{0, 0, 0, 0} : rv[c];
      char* const krow = kb + row * PF_KROW;
      char* const vrow = vb + row * PF_VROW;
      if constexpr (FP8) {
        *reinterpret_cast<i32x4*>(krow + (((2 * ld_ch) ^ (row & 15)) << 4)) = pf_fp8x8_to_bf16x8(rk[c][0], rk[c][1]);
        *reinterpret_cast<i32x4*>(krow + (((2 * ld_ch + 1) ^ (row & 15)) << 4)) =
            pf_fp8x8_to_bf16x8(rk[c][2], rk[c][3]);
        *reinterpret_cast<i32x4*>(vrow + 2 * ld_ch * CHUNK) = pf_fp8x8_to_bf16x8(v[0], v[1]);
        *reinterpret_cast<i32x4*>(vrow + (2 * ld_ch + 1) * CHUNK) = pf_fp8x8_to_bf16x8(v[2], v[3]);
      } else {
        *reinterpret_cast<i32x4*>(krow + ((ld_ch ^ (row & 15)) << 4)) = rk[c];
        *reinterpret_cast<i32x4*>(vrow + ld_ch * CHUNK) = v;
      }
    }
  };

  float m = NEG_INF, l = 0.f;  // l: the lane's part, the sum over its own 32 tokens of every tile
  f32x16 acc[4];               // O^T: fragment n holds d = 32 n + (i & 3) + 8 (i >> 2) + 4 h of query row r
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;

  // K row read: row 32 u + r, chunk 2 s + h, swizzled by the row's low 4 bits (r & 15 for both u)
  const int k_off = r * PF_KROW;
  const int k_sw = h ^ (r & 15);
  // The transposed read: lane 4 q + p of a group of 16 names row q, columns 4 p .. 4 p + 3 of a 4 x 16 block and
  // lane i receives column i of the 4 rows.  Lanes 16 g .. 16 g + 15 are the d columns 16 (g & 1) .. + 15 of a
  // fragment and lane half h = g >> 1: the block's rows are tokens 4 h .. 4 h + 3 of a run of 8.
  const int v_off = (4 * h + ((lane & 15) >> 2)) * PF_VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;

  auto compute = [&](auto masked_t, int j, int buf) {
    constexpr bool MASKED = decltype(masked_t)::value;
    const char* const kb = lds + buf * PF_STAGE;
    const char* const vb = kb + PF_KBYTES;

    // S^T = K Q^T for the two halves of 32 tokens
    f32x16 sc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[u][i] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16x8 kf =
            *reinterpret_cast<const bf16x8*>(kb + u * 32 * PF_KROW + k_off + (((2 * s) ^ k_sw) << 4));
        sc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sc[u], 0, 0, 0);
        if (s % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // four K fragments in registers at a time
      }
    }

    // the lane's 32 tokens of query row r: x, masked by select (a NaN from a slot the row may not see goes with it)
    const int rel = pos - j * PF_KV;  // the row sees the tile's tokens 0 .. rel
    float mx = NEG_INF;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lt = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * h;
        float x = sc[u][i] * qk_scale;
        if constexpr (MASKED) x = lt <= rel ? x : NEG_INF;
        sc[u][i] = x;
        mx = fmaxf(mx, x);
      }
    {
      float a, bb;
      pf_pair(mx, a, bb);
      mx = fmaxf(a, bb);
    }
    const float mn = fmaxf(m, mx);
    const float ms = mn == NEG_INF ? 0.f : mn;  // every x at -inf: p = exp2(-inf) = 0, not exp2(-inf + inf)
    const float alpha = __builtin_amdgcn_exp2f(m - ms);
    m = mn;
    float ps = 0.f;
    bf16x8 pf[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(sc[u][i] - ms);
        ps += p;
        pf[u][i >> 3][i & 7] = static_cast<__bf16>(p);  // round to nearest even
      }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] *= alpha;

    // O^T += V^T P^T
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const char* const vp = vb + v_off + (32 * u + 16 * s) * PF_VROW + 64 * n;
          const pf_i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_lds_i16x4_t)(vp));
          const pf_i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_lds_i16x4_t)(vp + 8 * PF_VROW));
          const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[u][s], acc[n], 0, 0, 0);
          if (u == 1 && s == 1) __builtin_amdgcn_sched_barrier(0);  // one fragment's V reads in registers at a time
        }
  };

  // Every condition below is uniform over the workgroup or over the wave: the transposed read needs EXEC all ones.
  if (ntiles > 0) {
    gload(0);
    lstore(0, 0);
  }
  __syncthreads();
  for (int j = 0; j < ntiles; ++j) {
    const int buf = j & 1;
    const bool more = j + 1 < ntiles;
    if (more) gload(j + 1);
    const int tok0 = j * PF_KV;  // <= pmax
    if (wave_any && tok0 <= pw_max) {
      if (pw_min - tok0 < PF_KV - 1)
        compute(std::true_type{}, j, buf);
      else
        compute(std::false_type{}, j, buf);
    }
    if (more) lstore(j + 1, buf ^ 1);  // the buffer every wave left at the previous barrier
    __syncthreads();
  }

  // the two halves of a row's l meet; O = bf16((acc / l) * v_scale), zeros for a row that is not live
  float L;
  {
    float a, bb;
    pf_pair(l, a, bb);
    L = a + bb;
  }
  if (row_ok) {
    uint16_t* const orow = O + ((static_cast<size_t>(b) * T + t) * Hq + hq) * PF_D;
    const bool some = live && (L > 0.f || L != L);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint16_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = some ? f2bf((acc[n][4 * g + e] / L) * v_scale) : uint16_t{0};
        *reinterpret_cast<i32x2*>(orow + 32 * n + 8 * g + 4 * h) =
            i32x2{static_cast<int>(o[0] | (static_cast<uint32_t>(o[1]) << 16)),
                  static_cast<int>(o[2] | (static_cast<uint32_t>(o[3]) << 16))};
      }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

constexpr int kPrefillKinds = 2;

struct PrefillArgs {
  int kind;
  const void *Q, *K, *V, *block_table, *seq_lens;
  void* O;
  int B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len;
  float scale, k_scale, v_scale;
};

bool pf_overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bytes && y < x + bytes;
}

int64_t pf_blocks(const PrefillArgs& a) { return (static_cast<int64_t>(a.T) + PF_QROWS - 1) / PF_QROWS; }

// Everything the entry points refuse, before the first device call.
int pf_validate(const char* who, const PrefillArgs& a) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind < 0 || a.kind >= kPrefillKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (a.D != PF_D) return refuse("need D == 128");
  if (a.Hq < 1 || a.Hq > 4096) return refuse("need 1 <= Hq <= 4096");
  if (a.Hkv < 1 || a.Hq % a.Hkv || a.Hq / a.Hkv > 16) return refuse("need Hq % Hkv == 0 and Hq / Hkv <= 16");
  if (a.page < 16 || a.page > 256 || a.page % 16) return refuse("need page % 16 == 0 and 16 <= page <= 256");
  if (a.B < 1 || a.T < 1) return refuse("need B >= 1 and T >= 1");
  if (static_cast<int64_t>(a.B) * a.T > INT32_MAX) return refuse("B * T must stay below 2^31");
  if (pf_blocks(a) * a.B * a.Hq > INT32_MAX) return refuse("ceil(T / 256) * B * Hq must stay below 2^31");  // the grid
  if (a.num_pages < 1) return refuse("need num_pages >= 1");
  if (a.table_stride < 1) return refuse("need table_stride >= 1");
  if (a.max_seq_len < 1) return refuse("need max_seq_len >= 1");
  if (static_cast<int64_t>(a.max_seq_len) > static_cast<int64_t>(a.table_stride) * a.page)
    return refuse("need max_seq_len <= table_stride * page");
  if (!a.Q || !a.K || !a.V || !a.O || !a.block_table || !a.seq_lens)
    return refuse("Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.Q) | reinterpret_cast<uintptr_t>(a.K) | reinterpret_cast<uintptr_t>(a.V) |
       reinterpret_cast<uintptr_t>(a.O)) % 16)
    return refuse("Q, K_cache, V_cache and O must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.block_table) | reinterpret_cast<uintptr_t>(a.seq_lens)) % 4)
    return refuse("block_table and seq_lens must be 4-B aligned");
  if (pf_overlap(a.Q, a.O, static_cast<uint64_t>(a.B) * a.T * a.Hq * PF_D * 2)) return refuse("O must not overlap Q");
  if (!std::isfinite(a.scale) || !std::isfinite(a.k_scale) || !std::isfinite(a.v_scale) || !(a.scale > 0.f) ||
      !(a.k_scale > 0.f) || !(a.v_scale > 0.f))
    return refuse("scale, k_scale and v_scale must be finite and > 0");
  if (a.kind == GSX_ATTN_KV_BF16 && (a.k_scale != 1.0f || a.v_scale != 1.0f))
    return refuse("a bf16 cache takes no scales: k_scale and v_scale must be 1.0");
  return 0;
}

using prefill_launch_t = int (*)(const char* who, hipStream_t s, const PrefillArgs& a);

template <bool FP8>
int pf_launch(const char* who, hipStream_t s, const PrefillArgs& a) {
  const int nqb = static_cast<int>(pf_blocks(a));
  const float qk_scale = (a.scale * a.k_scale) * 1.4426950408889634f;
  hipLaunchKernelGGL((prefill_kernel<FP8>), dim3(nqb * a.B * a.Hq), dim3(PF_THREADS), 0, s,
                     static_cast<const uint16_t*>(a.Q), static_cast<const uint8_t*>(a.K),
                     static_cast<const uint8_t*>(a.V), static_cast<const int32_t*>(a.block_table),
                     static_cast<const int32_t*>(a.seq_lens), static_cast<uint16_t*>(a.O), a.B, a.T, a.Hq, a.Hkv,
                     a.page, a.num_pages, a.table_stride, a.max_seq_len, nqb, qk_scale, a.v_scale);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct PrefillCfg {
  const char* name;
  int q_rows, kv_tile, waves;
  prefill_launch_t launch[kPrefillKinds];  // indexed by GSX_ATTN_KV_*
};

// name: waves per workgroup - query rows per workgroup - tokens per KV tile
constexpr PrefillCfg kPrefillCfgs[] = {
    {"8w-q256-k64", PF_QROWS, PF_KV, PF_WAVES, {&pf_launch<false>, &pf_launch<true>}},
};
constexpr int kNumPrefillCfgs = sizeof(kPrefillCfgs) / sizeof(kPrefillCfgs[0]);

const PrefillCfg* pf_row(int cfg) { return cfg >= 0 && cfg < kNumPrefillCfgs ? &kPrefillCfgs[cfg] : nullptr; }

PrefillArgs pf_args(int kind, const void* Q, const void* K, const void* V, const void* block_table,
                    const void* seq_lens, void* O, int B, int T, int Hq, int Hkv, int D, int page, int num_pages,
                    int table_stride, int max_seq_len, float scale, float k_scale, float v_scale) {
  return {kind, Q, K, V, block_table, seq_lens, O, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len,
          scale, k_scale, v_scale};
}

}  // namespace
}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_prefill_attn_cfg_name(int cfg) { return pf_row(cfg) ? pf_row(cfg)->name : nullptr; }

int gsx_prefill_attn_cfg_shape(int cfg, int* q_rows, int* kv_tile, int* waves) {
  const PrefillCfg* c = pf_row(cfg);
  if (!c) return -1;
  *q_rows = c->q_rows;
  *kv_tile = c->kv_tile;
  *waves = c->waves;
  return 0;
}

int gsx_prefill_attn_launch_cfg(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv,
                                int D, int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                float k_scale, float v_scale, int cfg) {
  const char* who = "gsx_prefill_attn_launch_cfg";
  const PrefillCfg* c = pf_row(cfg);
  if (!c) return fail_arg("gsx_prefill_attn_launch_cfg: unknown config");
  const PrefillArgs a = pf_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page,
                                num_pages, table_stride, max_seq_len, scale, k_scale, v_scale);
  if (int rc = pf_validate(who, a)) return rc;
  return c->launch[kind](who, S(stream), a);
}

int gsx_prefill_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                     const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv, int D,
                     int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                     float v_scale) {
  const PrefillArgs a = pf_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page,
                                num_pages, table_stride, max_seq_len, scale, k_scale, v_scale);
  if (int rc = pf_validate("gsx_prefill_attn", a)) return rc;
  return kPrefillCfgs[0].launch[kind]("gsx_prefill_attn", S(stream), a);
}

int gsx_event_time_prefill_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv,
                                int D, int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                float k_scale, float v_scale, int iters, float* ms) {
  const PrefillArgs a = pf_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page,
                                num_pages, table_stride, max_seq_len, scale, k_scale, v_scale);
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = pf_validate("gsx_prefill_attn", a)) return rc;
  return event_time(stream, iters, ms,
                    [&] { return kPrefillCfgs[0].launch[a.kind]("gsx_prefill_attn", S(stream), a); });
}

}  // extern "C"
