// Multi-token decode attention: 2 to 16 new tokens per sequence (T == 1 is accepted too) attend, causally, over the
// paged KV cache of attn_decode.hip, on that kernel's bandwidth-bound plan.  It is what a server runs when it verifies
// speculative drafts, predicts several tokens at once, or finishes a chunked prefill: the cache is streamed from HBM
// once for all T tokens, where T launches of gsx_decode_attn stream it T times and gsx_prefill_attn spends a block of
// 256 query rows and G fetches of every KV head on it.  C ABI and numeric contract in gsx_kernels.h.
//
// attn_multi_kernel: a workgroup owns one (sequence, KV head, split), as attn_kernel does.
//   * The R = G * T query rows that share the KV head are the COLUMNS c = t * G + g of the transposed products, in
//     NF = ceil(R / 16) fragments of 16 (the kernel is a template on NF = 1 .. 4).  For a fixed t the G rows are
//     contiguous in Q, and the causal limit, base + c / G + 1 tokens, is monotone in c.  Columns at or past R read
//     zeros from a bounds-checked buffer load and are never stored.
//   * One tile of 32 tokens of K and V is loaded once, K from global memory to VGPRs in fragment shape and V through
//     the wave-private LDS image read back with ds_read_b64_tr_b16, exactly as in attn_kernel, and feeds all NF
//     fragments: S^T = K Q^T is 8 MFMAs per fragment on one set of K registers, O^T = V^T P^T 8 per fragment on one
//     set of transposed V reads.  The HBM bytes are those of one decode step for up to 64 query rows.
//   * A lane's column of a fragment is one query row, so the softmax state (m, l), the causal limit and the 32
//     accumulators per fragment are per lane.  The mask is the select attn_kernel has for seq_len, with the column's
//     own limit in its place: a token at or past it has its x replaced by -inf.  A column may be masked entirely in a
//     tile in which its neighbours are live (a tile that starts at base + 1, for the column of t = 0): its tile
//     maximum is -inf, the subtrahend of the exponent is then 0 and not -inf, and in a merge such a partial has
//     weight 0 (merge_weight), so exp2(-inf - -inf) is never formed.  A row that is not live (pos >= max_seq_len) has
//     limit 0: every token masked, l == 0, a row of zeros.  V at or past the sequence's end is written to the image as
//     zeros.
//   * Q: NF <= 2 keeps the fragments in VGPRs (32 at most).  NF >= 3 puts them into LDS once, in fragment order
//     ([fragment][k-step][lane] of 16 B, read back without a bank conflict), and reads the 4 NF fragments per tile:
//     16 KiB of LDS reads next to 16 KiB (bf16) of HBM, on a path with ten times the bandwidth.  That leaves the
//     register file to the 32 NF accumulators and the K/V ring.
//   * The waves' partials meet in LDS one fragment at a time, NF rounds over the V images in the layout of
//     attn_kernel (all of them at once would be 8 waves x 32 KiB at NF = 4), merged in wave order; with splits > 1 the
//     triples go to the workspace and attn_multi_merge_kernel merges the splits in split order.
// Resources (hipcc -O3, gfx950; profiles/attn_multi/README.md has the table): no scratch in any instantiation, no
// atomics; LDS W * 9216 B, plus NF * 4096 B of Q for NF >= 3.
// Offsets into the caches are 64-bit.  A page index is clamped into [0, num_pages) and a length to max_seq_len, so no
// content of block_table, seq_lens or the caches makes the kernel read outside the caches or write outside O and the
// workspace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "attn_tile.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {
namespace {

typedef __attribute__((address_space(3))) const char* lds_cptr_t;
typedef __attribute__((address_space(3))) const bf16x8* lds_bf16x8_t;

constexpr int AM_MAX_T = 16;     // new tokens per sequence
constexpr int AM_MAX_ROWS = 64;  // G * T: four fragments of 16 columns
constexpr int AM_MAX_NF = AM_MAX_ROWS / 16;
constexpr int AM_QFRAG = 64 * CHUNK;  // bytes of one (fragment, k-step) of Q in LDS: 16 B per lane

template <bool FP8, int NF, int W, int F>
__global__ __launch_bounds__(W * 64) void attn_multi_kernel(
    const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kc, const uint8_t* __restrict__ Vc,
    const int32_t* __restrict__ block_table, const int32_t* __restrict__ seq_lens, uint16_t* __restrict__ O,
    float* __restrict__ ws_acc, float* __restrict__ ws_ml, int T, int Hq, int Hkv, int page, int num_pages,
    int table_stride, int max_seq_len, int splits, float qk_scale, float v_scale) {
  constexpr int ROWB = FP8 ? AT_D : 2 * AT_D;  // bytes of a token's row in the cache
  constexpr int NCK = ROWB / 64;               // 16-B chunks of K a lane loads per 16-token half
  constexpr int NV = ROWB / 32;                // 16-B chunks of V a lane loads per tile
  constexpr int VLPR = ROWB / 16;              // lanes that share a row of V in one load
  constexpr int VROWS = 64 / VLPR;             // rows of V one load instruction covers
  constexpr bool QLDS = NF > 2;                // Q in LDS, not in VGPRs
  constexpr int ND = AT_D / 16;                // output fragments of 16 d
  constexpr float NEG_INF = -__builtin_inff();
  __shared__ __attribute__((aligned(16))) char lds[W * AT_WAVE_LDS + (QLDS ? NF * 4 * AM_QFRAG : 0)];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int G = Hq / Hkv;
  const int R = G * T;
  const int split = blockIdx.x % splits;
  const int pair = blockIdx.x / splits;
  const int kvh = pair % Hkv, b = pair / Hkv;

  int base = seq_lens[b];
  base = base < 0 ? 0 : base > max_seq_len ? max_seq_len : base;
  const int end = max_seq_len - base < T ? max_seq_len : base + T;  // the tokens the caches hold after the chunk, >= 1
  const int nt = (end - 1) / AT_TILE + 1;
  const int tps = (nt + splits - 1) / splits;  // tiles per split
  const int t0 = split * tps;
  const int t1 = t0 + tps < nt ? t0 + tps : nt;
  const int mine = t0 + wid < t1 ? (t1 - t0 - wid + W - 1) / W : 0;  // tiles t0 + wid, t0 + wid + W, ...
  const int32_t* bt = block_table + static_cast<size_t>(b) * table_stride;

  // Column c = 16 f + fr is query row (t, g) = (c / G, c % G) of the group: element offset `qoff` in the sequence's
  // Q and O, and `lim` tokens to see: base + t + 1, or 0 for a column past R and for a row that is not live.
  const size_t seq_off = static_cast<size_t>(b) * T * Hq * AT_D;
  const uint32_t seq_bytes = static_cast<uint32_t>(T * Hq * AT_D * 2);
  auto column = [&](int f, int& qoff, int& lim) __attribute__((always_inline)) {
    const int c = 16 * f + fr;
    const int t = c / G, g = c - t * G;
    qoff = (t * Hq + kvh * G + g) * AT_D;
    lim = c < R && t < max_seq_len - base ? base + t + 1 : 0;
    return c < R;
  };
  int lim[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    int qoff;
    column(f, qoff, lim[f]);
  }

  // Q.  k-step s of the first product covers, per lane, the 8 d of chunk 4 s + fq (bf16), or of the half (s & 1) of
  // the cache's 16-B chunk 4 (s >> 1) + fq (e4m3, 16 d per chunk).
  bf16x8 qf[QLDS ? 1 : NF][4];
  char* const ql = lds + W * AT_WAVE_LDS;
  {
    const __amdgpu_buffer_rsrc_t qbuf = rows_buffer(Q + seq_off, seq_bytes);
    auto qload = [&](int f, int s) __attribute__((always_inline)) {
      int qoff, unused;
      const bool ok = column(f, qoff, unused);
      const int d0 = FP8 ? 16 * (4 * (s >> 1) + fq) + 8 * (s & 1) : 8 * (4 * s + fq);
      // a column past R names the buffer's end: zeros
      return __builtin_amdgcn_raw_buffer_load_b128(qbuf, ok ? (qoff + d0) * 2 : static_cast<int>(seq_bytes), 0, 0);
    };
    if constexpr (QLDS) {
      for (int i = wid; i < NF * 4; i += W)
        *reinterpret_cast<i32x4*>(ql + i * AM_QFRAG + lane * CHUNK) = qload(i >> 2, i & 3);
      __syncthreads();
    } else {
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[f][s] = __builtin_bit_cast(bf16x8, qload(f, s));
    }
  }

  // the ring: slot i holds one tile's chunks of K (two halves of 16 tokens) and of V
  i32x4 rk[F][2][NCK], rv[F][NV];

  auto load = [&](auto slot, int j) __attribute__((always_inline)) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + wid + j * W) * AT_TILE;
    // The first row of each half, in rows of the cache.  A half lies in one page (page % 16 == 0).  The second half
    // of the sequence's last tile can lie wholly past the end, where the block table need not have an entry: it then
    // reads what the first half reads, and is masked.
    size_t row[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tok0 = tb + 16 * h < end ? tb + 16 * h : tb;
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

  // per fragment: the column's running maximum, the lane's part of l (the sum over its own 8 tokens of every tile)
  float m[NF], l[NF];
  f32x4 acc[NF][ND];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    m[f] = NEG_INF;
    l[f] = 0.f;
#pragma unroll
    for (int n = 0; n < ND; ++n) acc[f][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  char* const vl = lds + wid * AT_WAVE_LDS;
  // the transposed read of attn_kernel: group fq reads rows (tokens) 4 fq .. 4 fq + 3 and, 16 rows on, the same of
  // the second half; the block's 16 columns are d = 16 n .. 16 n + 15
  const char* const vtr = vl + (4 * fq + (fr >> 2)) * AT_VROW + (fr & 3) * 8;

  auto compute = [&](auto slot, int j) __attribute__((always_inline)) {
    constexpr int i = decltype(slot)::value;
    const int tb = (t0 + wid + j * W) * AT_TILE;

    bf16x8 kf[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        if constexpr (FP8) {
          const i32x4 raw = rk[i][h][st >> 1];
          kf[h][st] =
              __builtin_bit_cast(bf16x8, (st & 1) ? fp8x8_to_bf16x8(raw[2], raw[3]) : fp8x8_to_bf16x8(raw[0], raw[1]));
        } else {
          kf[h][st] = __builtin_bit_cast(bf16x8, rk[i][h][st]);
        }
      }

    // Q's address is made opaque once a tile: its reads stay inside the loop and out of the register file
    lds_cptr_t qp = (lds_cptr_t)(ql + lane * CHUNK);
    if constexpr (QLDS) asm volatile("" : "+v"(qp));

    bf16x8 pf[NF];
    static_for<NF>([&](auto frag) {
      constexpr int f = decltype(frag)::value;
      // S^T = K Q^T for both halves, on the tile's one set of K registers
      f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        bf16x8 q;
        if constexpr (QLDS) {
          q = *(lds_bf16x8_t)(qp + (f * 4 + st) * AM_QFRAG);
        } else {
          q = qf[f][st];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) s[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[h][st], q, s[h], 0, 0, 0);
      }

      // the lane's 8 tokens of the fragment's column fr: x, masked by select at the column's own limit (a NaN from a
      // slot past the end goes with it)
      float x[8];
      float mx = NEG_INF;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int tok = tb + 16 * (e >> 2) + 4 * fq + (e & 3);
        x[e] = tok < lim[f] ? s[e >> 2][e & 3] * qk_scale : NEG_INF;
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
      for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[f][n][jj] *= alpha;
      // one fragment's scores and probabilities at a time: only its 16 bits per token outlive it
      __builtin_amdgcn_sched_barrier(0);
    });

    // V into the wave's image: zeros for a slot at or past the end (0 * NaN in the MFMA would be NaN)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // behind the previous tile's reads
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int r = c * VROWS + lane / VLPR;
      const bool ok = tb + r < end;
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
    // O^T += V^T P^T: one transposed read of V per 16 d, used by every fragment
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + n * 32));
      const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t)(vtr + 16 * AT_VROW + n * 32));
      const bf16x8 vf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[f], acc[f][n], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  // The ring of attn_kernel: slot i holds tile t + i until it is consumed, then tile t + i + F.  Every condition is
  // wave-uniform (the transposed read needs EXEC all ones).
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

  // The waves' partials meet in LDS one fragment at a time, each in its own image: acc as [n][j][lane], then m and
  // the lane's part of l.  A wave without a tile contributes m = -inf, l = 0 and zeros.  In every round every wave
  // merges, in wave order, the output fragments n = wid, wid + W, ...; all of them compute M and L.
  static_for<NF>([&](auto frag) {
    constexpr int f = decltype(frag)::value;
    if (f) __syncthreads();  // the previous round has been read
    {
      float* const mine_f = reinterpret_cast<float*>(vl);
#pragma unroll
      for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) mine_f[(n * 4 + jj) * 64 + lane] = acc[f][n][jj];
      mine_f[32 * 64 + lane] = m[f];
      mine_f[33 * 64 + lane] = l[f];
    }
    __syncthreads();

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
    int qoff, unused;
    const bool stored = column(f, qoff, unused);
    const size_t orow = (seq_off + qoff) / AT_D;  // the lane's row of O and of the workspace
    for (int n = wid; n < ND; n += W) {
      f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float* aw_f = reinterpret_cast<const float*>(lds + w * AT_WAVE_LDS);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) o[jj] += aw[w] * aw_f[(n * 4 + jj) * 64 + lane];
      }
      if (!stored) continue;
      const int d0 = 16 * n + 4 * fq;  // O^T map: row (d) 4 fq + j, column fr
      if (splits == 1) {
        uint16_t r[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) r[jj] = L > 0.f || L != L ? f2bf((o[jj] / L) * v_scale) : uint16_t{0};
        *reinterpret_cast<i32x2*>(O + orow * AT_D + d0) =
            i32x2{static_cast<int>(r[0] | (static_cast<uint32_t>(r[1]) << 16)),
                  static_cast<int>(r[2] | (static_cast<uint32_t>(r[3]) << 16))};
      } else {
        const size_t at = orow * splits + split;
        *reinterpret_cast<f32x4*>(ws_acc + at * AT_D + d0) = o;
        if (n == 0 && fq == 0) {
          ws_ml[at * 2] = M;
          ws_ml[at * 2 + 1] = L;
        }
      }
    }
  });
}

// One workgroup of 128 threads per row of O (new token, query head): thread d merges the splits' partials in split
// order.  A row that is not live has l == 0 in every split and gives zeros.
__global__ __launch_bounds__(AT_D) void attn_multi_merge_kernel(const float* __restrict__ ws_acc,
                                                                const float* __restrict__ ws_ml,
                                                                uint16_t* __restrict__ O, int splits, float v_scale) {
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

constexpr int kKinds = 2;

struct MultiArgs {
  int kind;
  const void *Q, *K, *V, *block_table, *seq_lens;
  void* O;
  int B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len;
  float scale, k_scale, v_scale;
  void* workspace;
  uint64_t workspace_bytes;
};

// fp32 partials of `splits` splits: acc[B * T][Hq][splits][128], then (m, l)[B * T][Hq][splits]
uint64_t am_ws_bytes(int B, int T, int Hq, int splits) {
  return splits <= 1 ? 0 : static_cast<uint64_t>(B) * T * Hq * splits * (AT_D + 2) * sizeof(float);
}

// What the shape arguments alone can get wrong (no pointers): shared by the launchers and the workspace query.
int am_validate_shape(const char* who, int B, int T, int Hq, int D, int page, int max_seq_len) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (D != AT_D) return refuse("need D == 128");
  if (B < 1 || B > (1 << 20)) return refuse("need 1 <= B <= 2^20");
  if (T < 1 || T > AM_MAX_T) return refuse("need 1 <= T <= 16");
  if (Hq < 1 || Hq > 4096) return refuse("need 1 <= Hq <= 4096");
  if (static_cast<int64_t>(B) * T * Hq > INT32_MAX) return refuse("B * T * Hq must stay below 2^31");  // the merge's grid
  if (page < 16 || page > 256 || page % 16) return refuse("need page % 16 == 0 and 16 <= page <= 256");
  if (max_seq_len < 1) return refuse("need max_seq_len >= 1");
  return 0;
}

bool am_overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bytes && y < x + bytes;
}

// Everything the entry points refuse, before the first device call.
int am_validate(const char* who, const MultiArgs& a, int splits) {
  char msg[200];
  auto refuse = [&](const char* rule) {
    std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
    return fail_arg(msg);
  };
  if (a.kind < 0 || a.kind >= kKinds) {
    std::snprintf(msg, sizeof(msg), "%s: unknown kind %d", who, a.kind);
    return fail_arg(msg);
  }
  if (int rc = am_validate_shape(who, a.B, a.T, a.Hq, a.D, a.page, a.max_seq_len)) return rc;
  if (a.Hkv < 1 || a.Hq % a.Hkv || a.Hq / a.Hkv > 16) return refuse("need Hq % Hkv == 0 and Hq / Hkv <= 16");
  if (a.Hq / a.Hkv * a.T > AM_MAX_ROWS) return refuse("need (Hq / Hkv) * T <= 64");
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
  if (am_overlap(a.Q, a.O, static_cast<uint64_t>(a.B) * a.T * a.Hq * AT_D * 2)) return refuse("O must not overlap Q");
  if (!std::isfinite(a.scale) || !std::isfinite(a.k_scale) || !std::isfinite(a.v_scale))
    return refuse("scale, k_scale and v_scale must be finite");
  if (a.kind == GSX_ATTN_KV_BF16 && (a.k_scale != 1.0f || a.v_scale != 1.0f))
    return refuse("a bf16 cache takes no scales: k_scale and v_scale must be 1.0");
  if (splits < 1 || splits > AT_MAX_SPLITS) return refuse("need 1 <= splits <= 64");
  if (static_cast<int64_t>(a.B) * a.Hkv * splits > INT32_MAX) return refuse("B * Hkv * splits must stay below 2^31");
  const uint64_t need = am_ws_bytes(a.B, a.T, a.Hq, splits);
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

using am_launch_t = int (*)(const char* who, hipStream_t s, const MultiArgs& a, int splits);

template <bool FP8, int NF, int W, int F>
int am_launch(const char* who, hipStream_t s, const MultiArgs& a, int splits) {
  const size_t rows = static_cast<size_t>(a.B) * a.T * a.Hq;
  float* ws_acc = static_cast<float*>(a.workspace);
  float* ws_ml = ws_acc ? ws_acc + rows * splits * AT_D : nullptr;
  if (splits == 1) ws_acc = ws_ml = nullptr;
  const float qk_scale = (a.scale * a.k_scale) * 1.4426950408889634f;
  hipLaunchKernelGGL((attn_multi_kernel<FP8, NF, W, F>), dim3(a.B * a.Hkv * splits), dim3(W * 64), 0, s,
                     static_cast<const uint16_t*>(a.Q), static_cast<const uint8_t*>(a.K),
                     static_cast<const uint8_t*>(a.V), static_cast<const int32_t*>(a.block_table),
                     static_cast<const int32_t*>(a.seq_lens), static_cast<uint16_t*>(a.O), ws_acc, ws_ml, a.T, a.Hq,
                     a.Hkv, a.page, a.num_pages, a.table_stride, a.max_seq_len, splits, qk_scale, a.v_scale);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, who);
  if (splits > 1) {
    hipLaunchKernelGGL(attn_multi_merge_kernel, dim3(static_cast<uint32_t>(rows)), dim3(AT_D), 0, s, ws_acc, ws_ml,
                       static_cast<uint16_t*>(a.O), splits, a.v_scale);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e, who);
  }
  return 0;
}

struct MultiCfg {
  const char* name;
  int waves, inflight;
  am_launch_t launch[kKinds][AM_MAX_NF];  // indexed by GSX_ATTN_KV_* and by the fragments of 16 columns, less one
};
template <int W, int F>
constexpr MultiCfg am_cfg(const char* name) {
  return {name,
          W,
          F,
          {{&am_launch<false, 1, W, F>, &am_launch<false, 2, W, F>, &am_launch<false, 3, W, F>,
            &am_launch<false, 4, W, F>},
           {&am_launch<true, 1, W, F>, &am_launch<true, 2, W, F>, &am_launch<true, 3, W, F>,
            &am_launch<true, 4, W, F>}}};
}

// name: waves per workgroup - tiles of 32 tokens a wave keeps in flight
constexpr MultiCfg kMultiCfgs[] = {
    am_cfg<4, 1>("4w-f1"),
    am_cfg<4, 2>("4w-f2"),
};
constexpr int kNumMultiCfgs = sizeof(kMultiCfgs) / sizeof(kMultiCfgs[0]);

const MultiCfg* am_row(int cfg) { return cfg >= 0 && cfg < kNumMultiCfgs ? &kMultiCfgs[cfg] : nullptr; }

int am_run(const MultiCfg& c, const char* who, hipStream_t s, const MultiArgs& a, int splits) {
  const int nf = (a.Hq / a.Hkv * a.T + 15) / 16;
  return c.launch[a.kind][nf - 1](who, s, a, splits);
}

// The dispatch rule, from the (sequence, KV head) pairs, T and max_seq_len alone (a stream's CU mask is not known
// here, and the lengths are in device memory).  It is attn_pick()'s, and the measurement below let it stand:
//   configuration "4w-f2" for both cache types and every T;
//   splits = ceil(256 / pairs), one workgroup for each of the 256 CUs, but no more than leave every wave of a split 4
//   tiles (max_seq_len / 512), and at most 64.
// Measured on one MI355X on a ring of per-layer caches of more than 1 GiB, pages of 16 tokens in random order,
// microseconds per launch by splits for "4w-f2" (profiles/attn_multi/README.md has "4w-f1", every T and the yardsticks):
//                                       pairs  T  splits: 1      2      4      8      16     32     64    rule
//   bf16  B 1  x 32768, 64/8 heads          8  2                               55.9   38.8   38.3   51.8    32
//   bf16  B 1  x 32768, 64/8                8  8                               115.9  71.2   54.3   75.2    32
//   bf16  B 8  x 8192,  64/8               64  2          100.1  60.3   52.8   58.3   68.3   85.7            4
//   bf16  B 8  x 8192,  64/8               64  8          223.6  120.8  75.2   90.2   115.3  153.0           4
//   bf16  B 64 x 2048,  64/8              512  2          97.6   109.7  126.6                                1
//   bf16  B 64 x 2048,  64/8              512  8          147.3  179.5  227.2                                1
//   bf16  B 8  x 8192,  32/32             256  2          193.2  193.1  194.9  198.9                         1
//   bf16  B 8  x 8192,  32/32             256  16         187.4  187.9  195.6  204.8                         1
//   fp8   B 1  x 32768, 64/8                8  2                               56.0   35.7   29.2   39.5    32
//   fp8   B 8  x 8192,  64/8               64  2          100.4  56.4   34.8   35.0   41.0   49.3            4
//   fp8   B 8  x 8192,  64/8               64  8          239.9  128.8  74.8   83.5   102.9  136.8           4
//   fp8   B 64 x 2048,  64/8              512  8          139.9  162.6  202.8                                1
//   fp8   B 8  x 8192,  32/32             256  4          106.7  101.4  103.6  108.0                         1
// In every row ceil(256 / pairs) decides and is the best or within 5 % of the best split count of "4w-f2".  Between the
// configurations the best cells differ by 0 to 7 %: "4w-f1" is ahead at four fragments (T 8 at 64/8 heads: 2 to 7 %
// in bf16) and, with two splits, for e4m3 at 32/32 heads (3 to 7 %); "4w-f2" is ahead for e4m3 at one and two
// fragments (up to 15 % at B 64, T 4).  One rule serves both cache types, as attn_pick() does.
void am_pick(int64_t pairs, int T, int max_seq_len, int* cfg, int* splits) {
  const int tiles = (max_seq_len - 1) / AT_TILE + 1;
  *cfg = 1;
  const int w = kMultiCfgs[*cfg].waves;
  int64_t want = (256 + pairs - 1) / pairs;
  const int most = tiles / (4 * w);
  if (want > most) want = most;
  if (want > AT_MAX_SPLITS) want = AT_MAX_SPLITS;
  *splits = want < 1 ? 1 : static_cast<int>(want);
}

MultiArgs am_args(int kind, const void* Q, const void* K, const void* V, const void* block_table,
                  const void* seq_lens, void* O, int B, int T, int Hq, int Hkv, int D, int page, int num_pages,
                  int table_stride, int max_seq_len, float scale, float k_scale, float v_scale, void* workspace,
                  uint64_t workspace_bytes) {
  return {kind, Q, K, V, block_table, seq_lens, O, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len,
          scale, k_scale, v_scale, workspace, workspace_bytes};
}

// What the dispatching entry point will run, or why it refuses: no device call.
int am_plan(const char* who, const MultiArgs& a, int* cfg, int* splits) {
  if (int rc = am_validate(who, a, 1)) return rc;  // everything but the workspace
  am_pick(static_cast<int64_t>(a.B) * a.Hkv, a.T, a.max_seq_len, cfg, splits);
  return am_validate(who, a, *splits);
}

int am_dispatch(const char* who, void* stream, const MultiArgs& a) {
  int cfg = 0, splits = 1;
  if (int rc = am_plan(who, a, &cfg, &splits)) return rc;
  return am_run(kMultiCfgs[cfg], who, S(stream), a, splits);
}

}  // namespace
}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_decode_attn_multi_cfg_name(int cfg) { return am_row(cfg) ? am_row(cfg)->name : nullptr; }

int gsx_decode_attn_multi_cfg_shape(int cfg, int* waves, int* inflight) {
  const MultiCfg* c = am_row(cfg);
  if (!c) return -1;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_decode_attn_multi_workspace_bytes(int B, int T, int Hq, int D, int page, int max_seq_len, uint64_t* bytes) {
  const char* who = "gsx_decode_attn_multi_workspace_bytes";
  if (!bytes) return fail_arg("gsx_decode_attn_multi_workspace_bytes: bytes must not be NULL");
  if (int rc = am_validate_shape(who, B, T, Hq, D, page, max_seq_len)) return rc;
  // Hkv is not known here: the fewest KV heads Hq and T allow (the largest groups) give the fewest pairs and the
  // most splits
  const int gmax = AM_MAX_ROWS / T < 16 ? AM_MAX_ROWS / T : 16;
  int cfg = 0, splits = 1;
  am_pick(static_cast<int64_t>(B) * ((Hq + gmax - 1) / gmax), T, max_seq_len, &cfg, &splits);
  *bytes = am_ws_bytes(B, T, Hq, splits);
  return 0;
}

int gsx_decode_attn_multi_launch_cfg(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                     const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq,
                                     int Hkv, int D, int page, int num_pages, int table_stride, int max_seq_len,
                                     float scale, float k_scale, float v_scale, void* workspace,
                                     uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_decode_attn_multi_launch_cfg";
  const MultiCfg* c = am_row(cfg);
  if (!c) return fail_arg("gsx_decode_attn_multi_launch_cfg: unknown config");
  const MultiArgs a = am_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page, num_pages,
                              table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  if (int rc = am_validate(who, a, splits)) return rc;
  return am_run(*c, who, S(stream), a, splits);
}

int gsx_decode_attn_multi(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                          const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv, int D,
                          int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                          float v_scale, void* workspace, uint64_t workspace_bytes) {
  const MultiArgs a = am_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page, num_pages,
                              table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  return am_dispatch("gsx_decode_attn_multi", stream, a);
}

int gsx_event_time_decode_attn_multi(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                     const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq,
                                     int Hkv, int D, int page, int num_pages, int table_stride, int max_seq_len,
                                     float scale, float k_scale, float v_scale, void* workspace,
                                     uint64_t workspace_bytes, int iters, float* ms) {
  const MultiArgs a = am_args(kind, Q, K_cache, V_cache, block_table, seq_lens, O, B, T, Hq, Hkv, D, page, num_pages,
                              table_stride, max_seq_len, scale, k_scale, v_scale, workspace, workspace_bytes);
  // refused before the events are made, under the name of the entry point that is timed
  int cfg = 0, splits = 1;
  if (int rc = am_plan("gsx_decode_attn_multi", a, &cfg, &splits)) return rc;
  return event_time(stream, iters, ms, [&] { return am_dispatch("gsx_decode_attn_multi", stream, a); });
}

}  // extern "C"
