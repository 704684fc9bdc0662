// What the two MLA decode attention entry points share (attn_mla.hip: one new token per sequence; attn_mla_multi.hip:
// 1 .. 16): the kernel, the merge of the splits, the validation and the launcher.  A sequence's columns are its (token,
// head) pairs, C = T * Hq of them, T = 1 in attn_mla.hip; the MULTI instantiations differ in the mask alone.
//
// mla_kernel: a workgroup of four waves owns one (sequence, column block, split).
//   * Columns.  The columns of a block are the COLUMNS of the transposed products on v_mfma_f32_16x16x32_bf16, NF = 1 ..
//     4 fragments of 16 (the orientation of attn_multi_kernel).  C <= 64 is one block of ceil(C / 16) fragments; more
//     columns are ceil(C / 64) blocks of NF = ceil(C / (16 blocks)) fragments each, so 65 are 48 + 17 and not 64 + 1.
//     Column c = t * Hq + h is row b * C + c of Q and of O: the layout Q[B * T][Hq][576] makes them contiguous.
//     Columns at or past C read zeros from a bounds-checked buffer load and are never stored.  The block's Q lies in
//     LDS in fragment order, [fragment][k-step][lane] of 16 B (up to 72 KiB), written once.
//   * The tile.  32 tokens x 576 elements are staged in LDS ONCE, as bf16 whatever the cache holds (an e4m3 row is
//     widened on the way in, which is exact), in rows of 1152 + 32 B: all 256 threads fetch 16-B chunks of the rows
//     (consecutive threads, consecutive chunks) into a ring of F register sets, F tiles ahead, and store a set to the
//     image when its tile's turn comes.  A slot at or past the sequence's end (seq_len; with MULTI min(base + T,
//     max_seq_len)) is stored as zeros.  The image is read twice: row-wise, ds_read_b128, as the K operand of the score
//     product, and through ds_read_b64_tr_b16 over its first 512 columns as the transposed V operand of the output
//     product.  The row pitch, 37 * 32 B, puts the 8 rows of a half-wave's transposed read on disjoint banks.
//   * Scores: split by token half and by k.  Wave w takes the 16 tokens of half w & 1 and the 9 k-steps of k half
//     w >> 1, for all NF fragments: 9 NF MFMAs on 9 reads of K, the same count for every wave and every NF.  The fp32
//     partial S^T fragments meet in LDS (NF KiB per wave); after one barrier EVERY wave reads all four, adds the two k
//     halves of each token half (k half 0 + k half 1) and so holds the tile's 32 x 16 NF scores in the register shape
//     of attn_multi_kernel.  Each wave then runs the online softmax itself: mask by select (a token at or past the
//     column's limit has its x replaced by -inf), tile maximum, p = exp2(x - m), the lane's part of l, P rounded to
//     bf16.  The four waves compute the same m, l and P bit for bit, so neither P nor the maximum has to be exchanged:
//     the one exchange per tile is the 4 NF KiB of partial scores.
//   * The limit.  Without MULTI every column's limit is seq_len.  With MULTI column c of a sequence whose length before
//     the chunk is base sees tokens 0 .. base + c / Hq: its limit is that plus one when base + c / Hq < max_seq_len and
//     0 otherwise (the row is not live: l stays 0 and the row is stored as zeros).  A lane computes the limits of its NF
//     columns once, before the tile loop.  The tiles and the cuts of the splits are counted up to the sequence's end
//     and do not depend on the column block.
//   * Output: split by d.  Wave w owns output elements 128 w .. 128 w + 127 of every column: 8 transposed reads pairs of
//     V per tile, each feeding the NF fragments, 32 accumulator VGPRs per fragment.  No wave merge exists: at the end
//     wave w stores its quarter of the rows, O = bf16((acc / l) * kv_scale), or with splits > 1 its quarter of the fp32
//     partials; mla_merge_kernel then merges the splits in split order.
//   * Barriers: three per tile (image written / partial scores written / image and scores read), raw s_barrier behind
//     s_waitcnt lgkmcnt(0), so the ring's global loads stay in flight across them.  Every condition around a barrier
//     depends on (sequence, split) alone and is workgroup-uniform; every wave takes part in every exchange.
// LDS: NF * 18 KiB of Q + 37888 B of tile + NF * 4 KiB of scores: 60416 B (NF 1) to 128000 B (NF 4).  No scratch in any
// instantiation, no atomics (profiles/attn_mla/README.md and profiles/attn_mla_multi/README.md have the resource
// tables).
// Offsets into the cache are 64-bit.  A page index is clamped into [0, num_pages) and a length into [0, max_seq_len],
// so no content of block_table, seq_lens or the cache makes the kernel read outside the cache or write outside O and
// the workspace.
#pragma once

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
constexpr int ML_MAX_T = 16;                // new tokens per sequence (attn_mla_multi.hip)
constexpr int ML_MAX_NF = 4;                // fragments of 16 columns in a column block
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

// C: the sequence's columns, Hq without MULTI and T * Hq with it; nblk: its column blocks.
template <bool FP8, int NF, int F, bool MULTI>
__global__ __launch_bounds__(ML_W * 64) void mla_kernel(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ KV,
                                                       const int32_t* __restrict__ block_table,
                                                       const int32_t* __restrict__ seq_lens, uint16_t* __restrict__ O,
                                                       float* __restrict__ ws_acc, float* __restrict__ ws_ml, int C,
                                                       int nblk, int page, int num_pages, int table_stride,
                                                       int max_seq_len, int splits, float qk_scale, float out_scale,
                                                       int T, int Hq) {
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
  const int hb = rest % nblk, b = rest / nblk;
  const int col0 = hb * 16 * NF;

  // len: the sequence's end, past which slots are staged as zeros and up to which the tiles are counted
  int base = seq_lens[b];
  base = base < 0 ? 0 : base > max_seq_len ? max_seq_len : base;
  const int len = MULTI ? (max_seq_len - base < T ? max_seq_len : base + T) : base;
  const int nt = (len + AT_TILE - 1) / AT_TILE;
  const int tps = (nt + splits - 1) / splits;  // tiles per split
  const int t0 = split * tps;
  const int n = t0 + tps < nt ? tps : nt > t0 ? nt - t0 : 0;  // this split's tiles: workgroup-uniform
  const int32_t* bt = block_table + static_cast<size_t>(b) * table_stride;

  // the limits of the lane's columns (MULTI): a column at or past C, like a row that is not live, sees no token
  [[maybe_unused]] int lim[MULTI ? NF : 1];
  if constexpr (MULTI) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int col = col0 + 16 * f + fr;
      const int t = col / Hq;
      lim[f] = col < C && t < max_seq_len - base ? base + t + 1 : 0;
    }
  }

  // Q into LDS.  k-step s covers, per lane, the 8 elements 32 s + 8 fq ..; a column past C names the buffer's end and
  // reads zeros.  The first tile's barrier publishes it.
  {
    const uint32_t qbytes = static_cast<uint32_t>(C * ML_DK * 2);
    const __amdgpu_buffer_rsrc_t qbuf = rows_buffer(Q + static_cast<size_t>(b) * C * ML_DK, qbytes);
    for (int i = wid; i < NF * ML_KS; i += ML_W) {
      const int f = i / ML_KS, s = i - f * ML_KS;
      const int col = col0 + 16 * f + fr;
      const int off = col < C ? (col * ML_DK + 32 * s + 8 * fq) * 2 : static_cast<int>(qbytes);
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
      int limit = len;
      if constexpr (MULTI) limit = lim[f];
      float x[8];
      float mx = NEG_INF;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int tok = tb + 16 * (e >> 2) + 4 * fq + (e & 3);
        x[e] = tok < limit ? s[e >> 2][e & 3] * qk_scale : NEG_INF;
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

  // Every wave holds the same (m, l) and its own 128 d of every column.  A split in which a column saw no token has
  // m = -inf, l = 0 and zeros.
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int col = col0 + 16 * f + fr;
    if (col >= C) continue;
    float L = l[f] + __shfl_xor(l[f], 16);
    L = L + __shfl_xor(L, 32);
    const size_t orow = static_cast<size_t>(b) * C + col;
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

// One workgroup of 512 threads per row of O (sequence, column): thread d merges the splits' partials in split order.  A
// row that saw no token (a sequence of length 0, a row that is not live) has l == 0 in every split and gives zeros.
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
  int T = 1;  // new tokens per sequence: Q and O have B * T * Hq rows
};

// a sequence's columns, its column blocks, and the fragments of 16 columns per block: the columns are dealt to the
// blocks evenly
int ml_cols(const MlaArgs& a) { return a.T * a.Hq; }
int ml_col_blocks(int C) { return (C + 63) / 64; }
int ml_frags(int C) { return ((C + ml_col_blocks(C) - 1) / ml_col_blocks(C) + 15) / 16; }

// fp32 partials of `splits` splits: acc[rows][splits][512], then (m, l)[rows][splits]
uint64_t ml_ws_bytes(uint64_t rows, int splits) {
  return splits <= 1 ? 0 : rows * splits * (ML_DV + 2) * sizeof(float);
}

// What the shape arguments alone can get wrong (no pointers): shared by the launchers and the workspace queries.
int ml_validate_shape(const char* who, int B, int T, int Hq, int page, int max_seq_len) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (B < 1 || B > (1 << 20)) return refuse("need 1 <= B <= 2^20");
  if (T < 1 || T > ML_MAX_T) return refuse("need 1 <= T <= 16");
  if (Hq < 1 || Hq > ML_MAX_HQ) return refuse("need 1 <= Hq <= 128");
  if (static_cast<int64_t>(B) * T * Hq > INT32_MAX) return refuse("need B * T * Hq below 2^31");
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
  if (int rc = ml_validate_shape(who, a.B, a.T, a.Hq, a.page, a.max_seq_len)) return rc;
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
  if (static_cast<int64_t>(a.B) * ml_col_blocks(ml_cols(a)) * splits > INT32_MAX)
    return refuse("need B * column blocks * splits below 2^31");
  const uint64_t rows = static_cast<uint64_t>(a.B) * ml_cols(a);
  const uint64_t need = ml_ws_bytes(rows, splits);
  if (need) {
    if (!a.workspace || a.workspace_bytes < need) {
      std::snprintf(msg, sizeof(msg), "%s: workspace too small: %d splits need %llu bytes", who, splits,
                    static_cast<unsigned long long>(need));
      return fail_arg(msg);
    }
    if (reinterpret_cast<uintptr_t>(a.workspace) % 16) return refuse("workspace must be 16-B aligned");
  }
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

template <bool FP8, int NF, int F, bool MULTI>
int ml_launch(const char* who, hipStream_t s, const MlaArgs& a, int splits) {
  constexpr int LDS = ml_lds_bytes(NF);
  // more dynamic LDS than the default limit has to be asked for, per device, as in the dense launcher (gemm_tile.h)
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (int rc = current_device(who, &dev)) return rc;
  if (!attr[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mla_kernel<FP8, NF, F, MULTI>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) return fail(e, who);
    attr[dev].store(true, std::memory_order_release);
  }
  const int C = ml_cols(a), nblk = ml_col_blocks(C);
  const size_t rows = static_cast<size_t>(a.B) * C;
  float* ws_acc = static_cast<float*>(a.workspace);
  float* ws_ml = ws_acc ? ws_acc + rows * splits * ML_DV : nullptr;
  if (splits == 1) ws_acc = ws_ml = nullptr;
  const float qk_scale = (a.scale * a.kv_scale) * 1.4426950408889634f;
  hipLaunchKernelGGL((mla_kernel<FP8, NF, F, MULTI>), dim3(a.B * nblk * splits), dim3(ML_W * 64), LDS, s,
                     static_cast<const uint16_t*>(a.Q), static_cast<const uint8_t*>(a.KV),
                     static_cast<const int32_t*>(a.block_table), static_cast<const int32_t*>(a.seq_lens),
                     static_cast<uint16_t*>(a.O), ws_acc, ws_ml, C, nblk, a.page, a.num_pages, a.table_stride,
                     a.max_seq_len, splits, qk_scale, a.kv_scale, a.T, a.Hq);
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
  ml_launch_t launch[kKinds][ML_MAX_NF];  // indexed by GSX_ATTN_KV_* and by the fragments of 16 columns, less one
};
template <int F, bool MULTI>
constexpr MlaCfg ml_cfg(const char* name) {
  return {name,
          ML_W,
          F,
          {{&ml_launch<false, 1, F, MULTI>, &ml_launch<false, 2, F, MULTI>, &ml_launch<false, 3, F, MULTI>,
            &ml_launch<false, 4, F, MULTI>},
           {&ml_launch<true, 1, F, MULTI>, &ml_launch<true, 2, F, MULTI>, &ml_launch<true, 3, F, MULTI>,
            &ml_launch<true, 4, F, MULTI>}}};
}

int ml_run(const MlaCfg& c, const char* who, hipStream_t s, const MlaArgs& a, int splits) {
  return c.launch[a.kind][ml_frags(ml_cols(a)) - 1](who, s, a, splits);
}

MlaArgs ml_args(int kind, const void* Q, const void* KV, const void* block_table, const void* seq_lens, void* O, int B,
                int T, int Hq, int page, int num_pages, int table_stride, int max_seq_len, float scale, float kv_scale,
                void* workspace, uint64_t workspace_bytes) {
  return {kind, Q, KV, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride, max_seq_len, scale, kv_scale,
          workspace, workspace_bytes, T};
}

}  // namespace
}  // namespace gsxgemm
