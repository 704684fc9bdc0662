// Multi-head latent attention (MLA) decode over a paged latent cache: the attention of DeepSeek-V2/V3/R1 and Kimi K2
// in its absorbed form.  One new token per sequence; every token of the cache is ONE row of 576 elements, 512 latent
// plus 64 rotated RoPE elements, shared by all 1 .. 128 query heads: all 576 are K, the first 512 are V as well.  C ABI
// and numeric contract in gsx_kernels.h.
//
// mla_kernel: a workgroup of four waves owns one (sequence, head block, split).
//   * Heads.  The heads of a block are the COLUMNS of the transposed products on v_mfma_f32_16x16x32_bf16, NF = 1 .. 4
//     fragments of 16 (the orientation of attn_multi_kernel).  Hq <= 64 is one block of ceil(Hq / 16) fragments; more
//     heads are two blocks of NF = ceil(Hq / 32) fragments each, so 65 heads are 48 + 17 and not 64 + 1.  Columns at or
//     past Hq read zeros from a bounds-checked buffer load and are never stored.  The block's Q lies in LDS in fragment
//     order, [fragment][k-step][lane] of 16 B (up to 72 KiB), written once.
//   * The tile.  32 tokens x 576 elements are staged in LDS ONCE, as bf16 whatever the cache holds (an e4m3 row is
//     widened on the way in, which is exact), in rows of 1152 + 32 B: all 256 threads fetch 16-B chunks of the rows
//     (consecutive threads, consecutive chunks) into a ring of F register sets, F tiles ahead, and store a set to the
//     image when its tile's turn comes.  A slot at or past seq_len is stored as zeros.  The image is read twice:
//     row-wise, ds_read_b128, as the K operand of the score product, and through ds_read_b64_tr_b16 over its first 512
//     columns as the transposed V operand of the output product.  The row pitch, 37 * 32 B, puts the 8 rows of a
//     half-wave's transposed read on disjoint banks.
//   * Scores: split by token half and by k.  Wave w takes the 16 tokens of half w & 1 and the 9 k-steps of k half
//     w >> 1, for all NF fragments: 9 NF MFMAs on 9 reads of K, the same count for every wave and every NF.  The fp32
//     partial S^T fragments meet in LDS (NF KiB per wave); after one barrier EVERY wave reads all four, adds the two k
//     halves of each token half (k half 0 + k half 1) and so holds the tile's 32 x 16 NF scores in the register shape
//     of attn_multi_kernel.  Each wave then runs the online softmax itself: mask by select (a slot at or past seq_len
//     has its x replaced by -inf), tile maximum, p = exp2(x - m), the lane's part of l, P rounded to bf16.  The four
//     waves compute the same m, l and P bit for bit, so neither P nor the maximum has to be exchanged: the one
//     exchange per tile is the 4 NF KiB of partial scores.
//   * Output: split by d.  Wave w owns output elements 128 w .. 128 w + 127 of every head: 8 transposed reads pairs of
//     V per tile, each feeding the NF fragments, 32 accumulator VGPRs per fragment.  No wave merge exists: at the end
//     wave w stores its quarter of the rows, O = bf16((acc / l) * kv_scale), or with splits > 1 its quarter of the fp32
//     partials; mla_merge_kernel then merges the splits in split order.
//   * Barriers: three per tile (image written / partial scores written / image and scores read), raw s_barrier behind
//     s_waitcnt lgkmcnt(0), so the ring's global loads stay in flight across them.  Every condition around a barrier
//     depends on (sequence, split) alone and is workgroup-uniform; every wave takes part in every exchange.
// LDS: NF * 18 KiB of Q + 37888 B of tile + NF * 4 KiB of scores: 60416 B (NF 1) to 128000 B (NF 4).  No scratch in any
// instantiation, no atomics (profiles/attn_mla/README.md has the resource table).
// Offsets into the cache are 64-bit.  A page index is clamped into [0, num_pages) and a length into [0, max_seq_len],
// so no content of block_table, seq_lens or the cache makes the kernel read outside the cache or write outside O and
// the workspace.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "attn_tile.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {
namespace {

typedef __attribute__((address_space(3))) const bf16x8* lds_bf16x8_t;

constexpr int ML_DK = 576;                  // elements of a cache row and of a query row: all of them are K
constexpr int ML_DV = 512;                  // the first of them are V, and a row of O
constexpr int ML_KS = ML_DK / 32;           // k-steps of the score product
constexpr int ML_W = 4;                     // waves per workgroup
constexpr int ML_MAX_HQ = 128;
constexpr int ML_MAX_NF = 4;                // fragments of 16 heads in a head block
constexpr int ML_ROW = ML_DK * 2 + 32;      // bytes of a token's row in the LDS image
constexpr int ML_IMG = AT_TILE * ML_ROW;    // the image of a tile
constexpr int ML_QFRAG = 64 * CHUNK;        // one (fragment, k-step) of Q in LDS: 16 B per lane
constexpr int ML_SFRAG = 64 * 16;           // one fp32 score fragment: 16 B per lane

constexpr int ml_lds_bytes(int nf) { return nf * ML_KS * ML_QFRAG + ML_IMG + ML_W * nf * ML_SFRAG; }

// LDS traffic of this wave has landed, then the workgroup meets.  Unlike __syncthreads() it leaves vector-memory loads
// in flight.
__device__ __forceinline__ void ml_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  ph_barrier();
}

template <bool FP8, int NF, int F>
__global__ __launch_bounds__(ML_W * 64) void mla_kernel(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ KV,
                                                       const int32_t* __restrict__ block_table,
                                                       const int32_t* __restrict__ seq_lens, uint16_t* __restrict__ O,
                                                       float* __restrict__ ws_acc, float* __restrict__ ws_ml, int Hq,
                                                       int nhb, int page, int num_pages, int table_stride,
                                                       int max_seq_len, int splits, float qk_scale, float out_scale) {
  constexpr int ROWB = FP8 ? ML_DK : 2 * ML_DK;  // bytes of a token's row in the cache
  constexpr int CPR = ROWB / CHUNK;              // 16-B chunks of a row
  constexpr int NCH = AT_TILE * CPR;             // chunks of a tile
  constexpr int NR = (NCH + ML_W * 64 - 1) / (ML_W * 64);  // chunks a thread fetches per tile (the last may be ragged)
  constexpr int ND = ML_DV / ML_W / 16;          // output fragments of 16 d a wave owns
  constexpr float NEG_INF = -__builtin_inff();
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const ql = lds;                           // Q: [fragment][k-step][lane]
  char* const tl = lds + NF * ML_KS * ML_QFRAG;   // the tile's image
  char* const sl = tl + ML_IMG;                   // partial scores: [wave][fragment][lane]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int split = blockIdx.x % splits;
  const int rest = blockIdx.x / splits;
  const int hb = rest % nhb, b = rest / nhb;
  const int head0 = hb * 16 * NF;

  int len = seq_lens[b];
  len = len < 0 ? 0 : len > max_seq_len ? max_seq_len : len;
  const int nt = (len + AT_TILE - 1) / AT_TILE;
  const int tps = (nt + splits - 1) / splits;  // tiles per split
  const int t0 = split * tps;
  const int n = t0 + tps < nt ? tps : nt > t0 ? nt - t0 : 0;  // this split's tiles: workgroup-uniform
  const int32_t* bt = block_table + static_cast<size_t>(b) * table_stride;

  // Q into LDS.  k-step s covers, per lane, the 8 elements 32 s + 8 fq ..; a column past Hq names the buffer's end and
  // reads zeros.  The first tile's barrier publishes it.
  {
    const uint32_t qbytes = static_cast<uint32_t>(Hq * ML_DK * 2);
    const __amdgpu_buffer_rsrc_t qbuf = rows_buffer(Q + static_cast<size_t>(b) * Hq * ML_DK, qbytes);
    for (int i = wid; i < NF * ML_KS; i += ML_W) {
      const int f = i / ML_KS, s = i - f * ML_KS;
      const int head = head0 + 16 * f + fr;
      const int off = head < Hq ? (head * ML_DK + 32 * s + 8 * fq) * 2 : static_cast<int>(qbytes);
      const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(qbuf, off, 0, 0);
      *reinterpret_cast<i32x4*>(ql + i * ML_QFRAG + lane * CHUNK) = v;
    }
  }

  // the ring: slot i holds the thread's chunks of one tile.  Chunk r of a thread is chunk r * 256 + tid of the tile:
  // row (r * 256 + tid) / CPR, chunk of the row the remainder.
  i32x4 rg[F][NR];
  auto chunk_at = [&](int r, int& row, int& c) __attribute__((always_inline)) {
    const int i = r * (ML_W * 64) + tid;
    row = i / CPR;
    c = i - row * CPR;
    return (r + 1) * (ML_W * 64) <= NCH || i < NCH;  // only an e4m3 tile's last round is ragged: a constant elsewhere
  };

  auto load = [&](auto slot, int j) __attribute__((always_inline)) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + j) * AT_TILE;
    // The first row of each half of 16 tokens, in rows of the cache.  A half lies in one page (page % 16 == 0).  The
    // second half of the sequence's last tile can lie wholly past the end, where the block table need not have an
    // entry: it then reads what the first half reads, and is stored as zeros.
    size_t first[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tok0 = tb + 16 * h < len ? tb + 16 * h : tb;
      const int lp = tok0 / page;
      uint32_t pp = static_cast<uint32_t>(bt[lp]);
      pp = pp < static_cast<uint32_t>(num_pages - 1) ? pp : static_cast<uint32_t>(num_pages - 1);
      first[h] = static_cast<size_t>(pp) * page + (tok0 - lp * page);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      int row, c;
      if (chunk_at(r, row, c))
        rg[i][r] = *reinterpret_cast<const i32x4*>(KV + (first[row >> 4] + (row & 15)) * ROWB + c * CHUNK);
    }
  };

  // the slot's chunks into the image, as bf16; zeros for a token at or past the end (0 * NaN in an MFMA would be NaN)
  auto stage = [&](auto slot, int j) __attribute__((always_inline)) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + j) * AT_TILE;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      int row, c;
      if (chunk_at(r, row, c)) {
        const i32x4 raw = tb + row < len ? rg[i][r] : i32x4{0, 0, 0, 0};
        char* const dst = tl + row * ML_ROW + c * (FP8 ? 2 * CHUNK : CHUNK);
        if constexpr (FP8) {
          *reinterpret_cast<i32x4*>(dst) = fp8x8_to_bf16x8(raw[0], raw[1]);
          *reinterpret_cast<i32x4*>(dst + CHUNK) = fp8x8_to_bf16x8(raw[2], raw[3]);
        } else {
          *reinterpret_cast<i32x4*>(dst) = raw;
        }
      }
    }
  };

  // per fragment: the column's running maximum, the lane's part of l (the sum over its own 8 tokens of every tile),
  // and the wave's 128 output elements of the column
  float m[NF], l[NF];
  f32x4 acc[NF][ND];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    m[f] = NEG_INF;
    l[f] = 0.f;
#pragma unroll
    for (int nn = 0; nn < ND; ++nn) acc[f][nn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int th = wid & 1, kh = wid >> 1;  // the wave's token half and k half of the score product
  // K operand: row 16 th + fr of the image, the 16 B of k-step s at 64 s + 16 fq
  const char* const kp = tl + (16 * th + fr) * ML_ROW + (kh * (ML_KS / 2)) * 64 + fq * CHUNK;
  const char* const qp = ql + (kh * (ML_KS / 2)) * ML_QFRAG + lane * CHUNK;
  // the transposed read of attn_kernel: group fq reads rows (tokens) 4 fq .. 4 fq + 3 and, 16 rows on, the same of the
  // second half; the block's 16 columns are d = 128 wid + 16 n ..
  const char* const vtr = tl + (4 * fq + (fr >> 2)) * ML_ROW + (fr & 3) * 8 + wid * (ML_DV / ML_W) * 2;

  auto compute = [&](int j) __attribute__((always_inline)) {
    const int tb = (t0 + j) * AT_TILE;
    // the wave's part of S^T = K Q^T: 16 tokens, half of k, every fragment
    {
      f32x4 sp[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) sp[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < ML_KS / 2; ++s) {
        const bf16x8 kf = *(lds_bf16x8_t)(kp + s * 64);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const bf16x8 q = *(lds_bf16x8_t)(qp + (f * ML_KS + s) * ML_QFRAG);
          sp[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, q, sp[f], 0, 0, 0);
        }
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) *reinterpret_cast<f32x4*>(sl + (wid * NF + f) * ML_SFRAG + lane * 16) = sp[f];
    }
    ml_barrier();

    bf16x8 pf[NF];
    static_for<NF>([&](auto frag) {
      constexpr int f = decltype(frag)::value;
      // token half h: wave h has k half 0, wave h + 2 k half 1
      f32x4 s[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
        s[h] = *reinterpret_cast<const f32x4*>(sl + (h * NF + f) * ML_SFRAG + lane * 16) +
               *reinterpret_cast<const f32x4*>(sl + ((h + 2) * NF + f) * ML_SFRAG + lane * 16);
      // the lane's 8 tokens of column fr: x, masked by select (a NaN from a slot past the end goes with it)
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
      const float mn = fmaxf(m[f], mx);
      const float ms = mn == NEG_INF ? 0.f : mn;  // every x at -inf: p = exp2(-inf) = 0, not exp2(-inf + inf)
      const float alpha = __builtin_amdgcn_exp2f(m[f] - ms);
      m[f] = mn;
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p = __builtin_amdgcn_exp2f(x[e] - ms);
        ps += p;
        pf[f][e] = static_cast<__bf16>(p);  // round to nearest even
      }
      l[f] = l[f] * alpha + ps;
#pragma unroll
      for (int nn = 0; nn < ND; ++nn)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[f][nn][jj] *= alpha;
      __builtin_amdgcn_sched_barrier(0);
    });

    // O^T += V^T P^T over the wave's 128 d: one transposed read of V per 16 d, used by every fragment
#pragma unroll
    for (int nn = 0; nn < ND; ++nn) {
      const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + nn * 32));
      const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + 16 * ML_ROW + nn * 32));
      const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f][nn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[f], acc[f][nn], 0, 0, 0);
    }
    ml_barrier();  // the image and the scores have been read
  };

  // Slot i holds tile j + i until its turn, then tile j + i + F.  Every condition is workgroup-uniform.
  static_for<F>([&](auto i) {
    if (i < n) load(i, i);
  });
  for (int j = 0; j < n; j += F) {
    static_for<F>([&](auto i) {
      if (j + i < n) {
        stage(i, j + i);
        if (j + i + F < n) load(i, j + i + F);
        ml_barrier();  // the image (and, the first time, Q) is written
        compute(j + i);
      }
    });
  }

  // Every wave holds the same (m, l) and its own 128 d of every column.  A split without a token has m = -inf, l = 0
  // and zeros.
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int head = head0 + 16 * f + fr;
    if (head >= Hq) continue;
    float L = l[f] + __shfl_xor(l[f], 16);
    L = L + __shfl_xor(L, 32);
    const size_t orow = static_cast<size_t>(b) * Hq + head;
#pragma unroll
    for (int nn = 0; nn < ND; ++nn) {
      const int d0 = wid * (ML_DV / ML_W) + 16 * nn + 4 * fq;  // O^T map: row (d) 4 fq + j, column fr
      if (splits == 1) {
        uint16_t r[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) r[jj] = L > 0.f || L != L ? f2bf((acc[f][nn][jj] / L) * out_scale) : uint16_t{0};
        *reinterpret_cast<i32x2*>(O + orow * ML_DV + d0) =
            i32x2{static_cast<int>(r[0] | (static_cast<uint32_t>(r[1]) << 16)),
                  static_cast<int>(r[2] | (static_cast<uint32_t>(r[3]) << 16))};
      } else {
        *reinterpret_cast<f32x4*>(ws_acc + (orow * splits + split) * ML_DV + d0) = acc[f][nn];
      }
    }
    if (splits > 1 && wid == 0 && fq == 0) {
      ws_ml[(orow * splits + split) * 2] = m[f];
      ws_ml[(orow * splits + split) * 2 + 1] = L;
    }
  }
}

// One workgroup of 512 threads per row of O (sequence, head): thread d merges the splits' partials in split order.  A
// sequence of length 0 has l == 0 in every split and gives zeros.
__global__ __launch_bounds__(ML_DV) void mla_merge_kernel(const float* __restrict__ ws_acc,
                                                          const float* __restrict__ ws_ml, uint16_t* __restrict__ O,
                                                          int splits, float out_scale) {
  const size_t at = static_cast<size_t>(blockIdx.x) * splits;
  const int d = threadIdx.x;
  float M = -__builtin_inff();
  for (int s = 0; s < splits; ++s) M = fmaxf(M, ws_ml[(at + s) * 2]);
  float L = 0.f, o = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float a = merge_weight(ws_ml[(at + s) * 2], M);
    L += a * ws_ml[(at + s) * 2 + 1];
    o += a * ws_acc[(at + s) * ML_DV + d];
  }
  O[static_cast<size_t>(blockIdx.x) * ML_DV + d] = L > 0.f || L != L ? f2bf((o / L) * out_scale) : uint16_t{0};
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

constexpr int kKinds = 2;

struct MlaArgs {
  int kind;
  const void *Q, *KV, *block_table, *seq_lens;
  void* O;
  int B, Hq, page, num_pages, table_stride, max_seq_len;
  float scale, kv_scale;
  void* workspace;
  uint64_t workspace_bytes;
};

int ml_head_blocks(int Hq) { return Hq > 64 ? 2 : 1; }
// fragments of 16 heads per block: the heads are dealt to the blocks evenly
int ml_frags(int Hq) { return ((Hq + ml_head_blocks(Hq) - 1) / ml_head_blocks(Hq) + 15) / 16; }

// fp32 partials of `splits` splits: acc[B][Hq][splits][512], then (m, l)[B][Hq][splits]
uint64_t ml_ws_bytes(int B, int Hq, int splits) {
  return splits <= 1 ? 0 : static_cast<uint64_t>(B) * Hq * splits * (ML_DV + 2) * sizeof(float);
}

// What the shape arguments alone can get wrong (no pointers): shared by the launchers and the workspace query.
int ml_validate_shape(const char* who, int B, int Hq, int page, int max_seq_len) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (B < 1 || B > (1 << 20)) return refuse("need 1 <= B <= 2^20");
  if (Hq < 1 || Hq > ML_MAX_HQ) return refuse("need 1 <= Hq <= 128");
  if (page < 16 || page > 256 || page % 16) return refuse("need page % 16 == 0 and 16 <= page <= 256");
  if (max_seq_len < 1) return refuse("need max_seq_len >= 1");
  return 0;
}

struct MlSpan {
  const void* p;
  uint64_t bytes;
};
bool ml_overlap(const MlSpan& a, const MlSpan& b) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}

// Everything the entry points refuse, before the first device call.
int ml_validate(const char* who, const MlaArgs& a, int splits) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind < 0 || a.kind >= kKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (int rc = ml_validate_shape(who, a.B, a.Hq, a.page, a.max_seq_len)) return rc;
  if (a.num_pages < 1) return refuse("need num_pages >= 1");
  if (a.table_stride < 1) return refuse("need table_stride >= 1");
  if (static_cast<int64_t>(a.max_seq_len) > static_cast<int64_t>(a.table_stride) * a.page)
    return refuse("need max_seq_len <= table_stride * page");
  if (!a.Q || !a.KV || !a.O || !a.block_table || !a.seq_lens)
    return refuse("Q, KV_cache, O, block_table and seq_lens must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.Q) | reinterpret_cast<uintptr_t>(a.KV) | reinterpret_cast<uintptr_t>(a.O)) % 16)
    return refuse("Q, KV_cache and O must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.block_table) | reinterpret_cast<uintptr_t>(a.seq_lens)) % 4)
    return refuse("block_table and seq_lens must be 4-B aligned");
  if (!std::isfinite(a.scale) || !std::isfinite(a.kv_scale) || a.scale <= 0.f || a.kv_scale <= 0.f)
    return refuse("scale and kv_scale must be finite and > 0");
  if (a.kind == GSX_ATTN_KV_BF16 && a.kv_scale != 1.0f)
    return refuse("a bf16 cache takes no scale: kv_scale must be 1.0");
  if (splits < 1 || splits > AT_MAX_SPLITS) return refuse("need 1 <= splits <= 64");
  const uint64_t need = ml_ws_bytes(a.B, a.Hq, splits);
  if (need) {
    if (!a.workspace || a.workspace_bytes < need) {
      std::snprintf(msg, sizeof(msg), "%s: workspace too small: %d splits need %llu bytes", who, splits,
                    static_cast<unsigned long long>(need));
      return fail_arg(msg);
    }
    if (reinterpret_cast<uintptr_t>(a.workspace) % 16) return refuse("workspace must be 16-B aligned");
  }
  const uint64_t rows = static_cast<uint64_t>(a.B) * a.Hq;
  const MlSpan o{a.O, rows * ML_DV * 2};
  const MlSpan q{a.Q, rows * ML_DK * 2};
  const MlSpan in[] = {
      {a.KV, static_cast<uint64_t>(a.num_pages) * a.page * ML_DK * (a.kind == GSX_ATTN_KV_FP8 ? 1 : 2)},
      {a.block_table, static_cast<uint64_t>(a.B) * a.table_stride * 4},
      {a.seq_lens, static_cast<uint64_t>(a.B) * 4},
      {a.workspace, need}};
  if (ml_overlap(o, q)) return refuse("O must not overlap Q");
  for (const MlSpan& s : in)
    if (ml_overlap(o, s)) return refuse("O must not overlap KV_cache, block_table, seq_lens or the workspace");
  return 0;
}

using ml_launch_t = int (*)(const char* who, hipStream_t s, const MlaArgs& a, int splits);

template <bool FP8, int NF, int F>
int ml_launch(const char* who, hipStream_t s, const MlaArgs& a, int splits) {
  constexpr int LDS = ml_lds_bytes(NF);
  // more dynamic LDS than the default limit has to be asked for, per device, as in the dense launcher (gemm_tile.h)
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (int rc = current_device(who, &dev)) return rc;
  if (!attr[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mla_kernel<FP8, NF, F>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) return fail(e, who);
    attr[dev].store(true, std::memory_order_release);
  }
  const size_t rows = static_cast<size_t>(a.B) * a.Hq;
  float* ws_acc = static_cast<float*>(a.workspace);
  float* ws_ml = ws_acc ? ws_acc + rows * splits * ML_DV : nullptr;
  if (splits == 1) ws_acc = ws_ml = nullptr;
  const int nhb = ml_head_blocks(a.Hq);
  const float qk_scale = (a.scale * a.kv_scale) * 1.4426950408889634f;
  hipLaunchKernelGGL((mla_kernel<FP8, NF, F>), dim3(a.B * nhb * splits), dim3(ML_W * 64), LDS, s,
                     static_cast<const uint16_t*>(a.Q), static_cast<const uint8_t*>(a.KV),
                     static_cast<const int32_t*>(a.block_table), static_cast<const int32_t*>(a.seq_lens),
                     static_cast<uint16_t*>(a.O), ws_acc, ws_ml, a.Hq, nhb, a.page, a.num_pages, a.table_stride,
                     a.max_seq_len, splits, qk_scale, a.kv_scale);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, who);
  if (splits > 1) {
    hipLaunchKernelGGL(mla_merge_kernel, dim3(static_cast<uint32_t>(rows)), dim3(ML_DV), 0, s, ws_acc, ws_ml,
                       static_cast<uint16_t*>(a.O), splits, a.kv_scale);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e, who);
  }
  return 0;
}

struct MlaCfg {
  const char* name;
  int waves, inflight;
  ml_launch_t launch[kKinds][ML_MAX_NF];  // indexed by GSX_ATTN_KV_* and by the fragments of 16 heads, less one
};
template <int F>
constexpr MlaCfg ml_cfg(const char* name) {
  return {name,
          ML_W,
          F,
          {{&ml_launch<false, 1, F>, &ml_launch<false, 2, F>, &ml_launch<false, 3, F>, &ml_launch<false, 4, F>},
           {&ml_launch<true, 1, F>, &ml_launch<true, 2, F>, &ml_launch<true, 3, F>, &ml_launch<true, 4, F>}}};
}

// name: waves per workgroup - tiles of 32 tokens a workgroup keeps in flight in registers
constexpr MlaCfg kMlaCfgs[] = {
    ml_cfg<1>("4w-f1"),
    ml_cfg<2>("4w-f2"),
};
constexpr int kNumMlaCfgs = sizeof(kMlaCfgs) / sizeof(kMlaCfgs[0]);

const MlaCfg* ml_row(int cfg) { return cfg >= 0 && cfg < kNumMlaCfgs ? &kMlaCfgs[cfg] : nullptr; }

int ml_run(const MlaCfg& c, const char* who, hipStream_t s, const MlaArgs& a, int splits) {
  return c.launch[a.kind][ml_frags(a.Hq) - 1](who, s, a, splits);
}

// The dispatch rule, from B, Hq and max_seq_len alone (a stream's CU mask is not known here, and the lengths are in
// device memory):
//   configuration "4w-f1" for both cache types and every head count;
//   splits = ceil(W / (B * head blocks)) with W = 512 workgroups for Hq <= 32 (one or two fragments: 60 or 83 KiB of
//   LDS; two workgroups fit a CU at one fragment and, by registers, for e4m3 at two) and W = 256, one for each CU,
//   above; but no more than leave every split 8 tiles (max_seq_len / 256), and at most 64.
// Measured on one MI355X on a ring of per-layer latent caches of more than 1 GiB, pages of 16 tokens in random order,
// microseconds per launch by splits for "4w-f1" (profiles/attn_mla/README.md has "4w-f2" and torch's path):
//                        Hq  splits: 1       2       4       8      16      32      64   rule
//   bf16  B 1  x 32768    16                                    120.0   71.61   55.65     64
//   bf16  B 1  x 32768   128                           537.23   281.0  157.53   104.4     64
//   bf16  B 8  x 8192     16            223.5  117.43   64.88   41.04   34.72             32
//   bf16  B 8  x 8192    128  1062.46  540.28   280.5  153.22   95.27  113.89             16
//   bf16  B 64 x 2048     16   115.53   65.54   42.93    43.7                              8
//   bf16  B 64 x 2048    128   283.06  169.14  185.97  232.33                              2
//   fp8   B 1  x 32768    16                                   115.14   68.57    53.2     64
//   fp8   B 1  x 32768   128                           456.49   239.5  136.92   94.53     64
//   fp8   B 8  x 8192     16           216.61  113.46   62.78   39.79   33.13             32
//   fp8   B 8  x 8192    128   906.62  461.49  241.03  133.14    83.7  102.52             16
//   fp8   B 64 x 2048     16   112.53   62.98   38.82   33.64                              8
//   fp8   B 64 x 2048    128   243.94  148.51  161.57   199.5                              2
// The rule's cell is the best cell of every row but bf16 B 64 x 2048 at 16 heads, where 4 splits are 1.8 % ahead of
// its 8 (the row's spread is 4 %; for e4m3 the 8 are 15 % ahead of 4).  W = 512 was measured at 16 heads only: 17 to
// 32 heads take it on the LDS arithmetic alone.  With one sequence the limit of 64 splits decides and the times still
// fall with the split count: 64 (128 for two head blocks) workgroups leave most of the 256 CUs idle, which a larger
// limit or a split of the heads would mend.  "4w-f2" is 0 to 7 % behind "4w-f1" in every cell: the compiler waits for
// nearly all of the ring's loads before a tile is stored to LDS (s_waitcnt vmcnt of 8 at the most), so the second tile
// in flight buys registers and no overlap; the table keeps it for the day the waits are counted by hand.
// Against torch's path on the gathered dense latent (bf16 matmul, softmax, matmul) the dispatched call is 1.9 to 2.5
// times faster at 16 heads and 1.13 to 1.8 times at 128, with ONE MISS: bf16, B 64 x 2048, 128 heads, 165.4 against
// 164.4 us.  That row is bound by the workgroup's own LDS traffic and barriers at four fragments (221 TFLOP/s), not by
// HBM (0.9 TB/s).
void mla_pick(int B, int Hq, int max_seq_len, int* cfg, int* splits) {
  const int tiles = (max_seq_len - 1) / AT_TILE + 1;
  const int64_t items = static_cast<int64_t>(B) * ml_head_blocks(Hq);
  const int workgroups = ml_frags(Hq) <= 2 ? 512 : 256;
  *cfg = 0;
  int64_t want = (workgroups + items - 1) / items;
  const int most = tiles / 8;
  if (want > most) want = most;
  if (want > AT_MAX_SPLITS) want = AT_MAX_SPLITS;
  *splits = want < 1 ? 1 : static_cast<int>(want);
}

MlaArgs ml_args(int kind, const void* Q, const void* KV, const void* block_table, const void* seq_lens, void* O, int B,
                int Hq, int page, int num_pages, int table_stride, int max_seq_len, float scale, float kv_scale,
                void* workspace, uint64_t workspace_bytes) {
  return {kind, Q, KV, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride, max_seq_len, scale, kv_scale,
          workspace, workspace_bytes};
}

// What the dispatching entry point will run, or why it refuses: no device call.
int ml_plan(const char* who, const MlaArgs& a, int* cfg, int* splits) {
  if (int rc = ml_validate(who, a, 1)) return rc;  // everything but the workspace
  mla_pick(a.B, a.Hq, a.max_seq_len, cfg, splits);
  return ml_validate(who, a, *splits);
}

int ml_dispatch(const char* who, void* stream, const MlaArgs& a) {
  int cfg = 0, splits = 1;
  if (int rc = ml_plan(who, a, &cfg, &splits)) return rc;
  return ml_run(kMlaCfgs[cfg], who, S(stream), a, splits);
}

}  // namespace
}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_mla_decode_attn_cfg_name(int cfg) { return ml_row(cfg) ? ml_row(cfg)->name : nullptr; }

int gsx_mla_decode_attn_cfg_shape(int cfg, int* waves, int* inflight) {
  const MlaCfg* c = ml_row(cfg);
  if (!c) return -1;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_mla_decode_attn_workspace_bytes(int B, int Hq, int page, int max_seq_len, uint64_t* bytes) {
  if (!bytes) return fail_arg("gsx_mla_decode_attn_workspace_bytes: bytes must not be NULL");
  if (int rc = ml_validate_shape("gsx_mla_decode_attn_workspace_bytes", B, Hq, page, max_seq_len)) return rc;
  int cfg = 0, splits = 1;
  mla_pick(B, Hq, max_seq_len, &cfg, &splits);
  *bytes = ml_ws_bytes(B, Hq, splits);
  return 0;
}

int gsx_mla_decode_attn_launch_cfg(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                                   const void* seq_lens, void* O, int B, int Hq, int page, int num_pages,
                                   int table_stride, int max_seq_len, float scale, float kv_scale, void* workspace,
                                   uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_mla_decode_attn_launch_cfg";
  const MlaCfg* c = ml_row(cfg);
  if (!c) return fail_arg("gsx_mla_decode_attn_launch_cfg: unknown config");
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  if (int rc = ml_validate(who, a, splits)) return rc;
  return ml_run(*c, who, S(stream), a, splits);
}

int gsx_mla_decode_attn(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                        const void* seq_lens, void* O, int B, int Hq, int page, int num_pages, int table_stride,
                        int max_seq_len, float scale, float kv_scale, void* workspace, uint64_t workspace_bytes) {
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  return ml_dispatch("gsx_mla_decode_attn", stream, a);
}

int gsx_event_time_mla_decode_attn(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                                   const void* seq_lens, void* O, int B, int Hq, int page, int num_pages,
                                   int table_stride, int max_seq_len, float scale, float kv_scale, void* workspace,
                                   uint64_t workspace_bytes, int iters, float* ms) {
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  // refused before the events are made, under the name of the entry point that is timed
  int cfg = 0, splits = 1;
  if (int rc = ml_plan("gsx_mla_decode_attn", a, &cfg, &splits)) return rc;
  return event_time(stream, iters, ms, [&] { return ml_dispatch("gsx_mla_decode_attn", stream, a); });
}

}  // extern "C"
