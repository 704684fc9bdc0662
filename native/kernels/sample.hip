// Token sampler and embedding gather for the pod workload: what closes a decode step.  gsx_sample turns a row of bf16
// logits (the LM head's output, gsx_decode_gemm_nt with N = vocabulary) into a token id, greedy or by temperature,
// top-k and top-p with a counter-based draw; gsx_embed_gather turns token ids back into rows of the embedding table.
// Both read their token ids and parameters from device memory, so a generation loop needs no host synchronisation.
// C ABI and numeric contract in gsx_kernels.h.
//
// sample_kernel: a workgroup of 1024 threads owns a row, and the row is read again from L2 in every pass (a row of
// 262144 logits does not fit LDS).  Thread t owns the 16-B chunks t, t + 1024, ..; four loads are in flight together.
// Every weight is an integer, so every sum is the same in whatever order LDS atomics add it.
// Top-k is settled on keys alone, which costs a compare and a count per logit; weights are computed for S only:
//   pass A   the largest key and the lowest index that holds it, packed into a u64 maximum, and for a sampled row a
//            histogram of counts over the key's high byte.  A greedy row ends here and counts nothing.
//   pass C   counts over the low byte, inside the high-byte bin that holds the k-th key: the k-th key.
//   pass D/E only when top-k cuts a tie group inside: counts over the index (high 9 bits, low 9 bits) of that group,
//            to the index of its last member in S.
//   compact  with k <= 1024, S is copied into LDS as (index, code) pairs, in whatever order the slots are claimed,
//            and the passes below read that list; with a larger k they read the row and test membership in S.
//   pass F/G with top-p: masses (u64) and counts of the tokens of weight > 0 over the high byte, then over the low
//            byte inside the bin where the mass reaches p Z: the last key of N, and Z_N.  A token of weight 0 adds to
//            no mass and is never drawn, so it is never binned.
//   pass H/I masses over the index of N's tokens (high 9 bits, low 9 bits): the prefix crossing.
// A histogram has 256 bins x 16 copies or 512 bins x 8 copies (a lane adds to copy lane % copies, which keeps lanes
// that hit one bin apart); the copies are summed, one wave scans the 512 sums, and the first bin that satisfies a
// monotone predicate is found with an LDS atomic minimum.  No float atomics, nothing between workgroups, no scratch.
// Contraction is off for the whole file: the contract rounds every multiply and add of the weight on its own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "bf16_key.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "mix64.h"

#pragma clang fp contract(off)

namespace gsxgemm {

constexpr int SM_THREADS = 1024;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_BINS = 512;      // bins the scan covers; a 256-bin pass leaves the upper half zero
constexpr int SM_SLOTS = 4096;    // bins x copies of a histogram
constexpr int SM_INFLIGHT = 4;    // chunks a thread loads before it uses the first
constexpr int SM_LIST = 1024;     // the largest S that is compacted into LDS
constexpr int SM_MAX_V = 262144;  // 512 x 512 indices
constexpr int EG_THREADS = 256;
constexpr int EG_MAX_GRID_ROWS = 65535;

struct SmShared {
  uint32_t hc[SM_SLOTS];  // histogram: counts
  uint64_t hm[SM_SLOTS];  // histogram: masses
  uint32_t sc[SM_BINS];   // the last pass: inclusive prefix sums in walk order
  uint64_t sm[SM_BINS];
  uint64_t list[SM_LIST];  // S, compacted: index << 16 | code
  uint64_t red[SM_WAVES];
  int found;
  uint32_t n;
};

// The integer weight of a logit (its bf16 code) against the row's maximum lf: trunc(g(f) * 2^(32 + n)).
__device__ __forceinline__ uint64_t sm_weight(uint32_t bits, float lf, float c) {
  const float l = __uint_as_float(bits << 16);
  const float d = l - lf;
  const float x = d * c;
  if (!(x >= -32.0f)) return 0;  // -inf and NaN as well
  const float nf = floorf(x);
  const float f = x - nf;
  float g = 0x1.e97886p-10f * f;
  g = g + 0x1.277576p-7f;
  g = g * f;
  g = g + 0x1.c91e04p-5f;
  g = g * f;
  g = g + 0x1.ebdb30p-3f;
  g = g * f;
  g = g + 0x1.62e4bcp-1f;
  g = g * f;
  g = g + 1.0f;
  // g = mant * 2^(e - 23), so g * 2^(32 + n) = mant * 2^(e + 9 + n): a shift, truncating
  const uint32_t gb = __float_as_uint(g);
  const int s = static_cast<int>(gb >> 23) - 127 + 9 + static_cast<int>(nf);
  const uint64_t mant = (gb & 0x7fffffu) | 0x800000u;
  return s >= 0 ? mant << (s & 63) : mant >> ((-s) & 63);
}

// f(index, bf16 code) for every element of the row that this thread owns
template <class F>
__device__ __forceinline__ void sm_for_each(const uint16_t* __restrict__ row, int nchunks, F&& f) {
  for (int c0 = threadIdx.x; c0 < nchunks; c0 += SM_THREADS * SM_INFLIGHT) {
    i32x4 v[SM_INFLIGHT];
    static_for<SM_INFLIGHT>([&](auto u) {
      const int c = c0 + SM_THREADS * u;
      if (c < nchunks) v[u] = *reinterpret_cast<const i32x4*>(row + 8 * static_cast<int64_t>(c));
    });
    static_for<SM_INFLIGHT>([&](auto u) {
      const int c = c0 + SM_THREADS * u;
      if (c >= nchunks) return;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t w = static_cast<uint32_t>(v[u][e >> 1]);
        f(8 * c + e, (e & 1) ? w >> 16 : w & 0xffffu);
      }
    });
  }
}

// Where a pass reads its tokens: the row, or S compacted into sh.list (n entries).
struct SmSource {
  const uint16_t* row;
  int nchunks;
  int n;  // >= 0: the list
};

template <class F>
__device__ __forceinline__ void sm_for_each(const SmShared& sh, const SmSource& src, F&& f) {
  if (src.n >= 0) {
    for (int i = threadIdx.x; i < src.n; i += SM_THREADS) {
      const uint64_t e = sh.list[i];
      f(static_cast<int>(e >> 16), static_cast<uint32_t>(e) & 0xffffu);
    }
  } else {
    sm_for_each(src.row, src.nchunks, f);
  }
}

__device__ __forceinline__ void sm_hist_zero(SmShared& sh) {
  for (int i = threadIdx.x; i < SM_SLOTS; i += SM_THREADS) {
    sh.hc[i] = 0;
    sh.hm[i] = 0;
  }
  __syncthreads();
}

template <int NB>
__device__ __forceinline__ void sm_hist_finish(SmShared& sh);

// One histogram pass over the tokens that `sel` gives a bin (>= 0) to, then the inclusive prefix sums of counts and
// masses over bins 0 .. 511 into sh.sc and sh.sm.  With MASS only tokens of weight > 0 are counted, and their weights
// added; without, every selected token is counted.  Ends with every thread past a barrier.
template <int NB, bool MASS, class SEL>
__device__ __forceinline__ void sm_hist_pass(SmShared& sh, const SmSource& src, float lf, float c, SEL&& sel) {
  constexpr int COPIES = SM_SLOTS / NB;
  sm_hist_zero(sh);
  const int copy = threadIdx.x & (COPIES - 1);
  sm_for_each(sh, src, [&](int idx, uint32_t bits) {
    const int bin = sel(sm_key(bits), idx);
    if (bin < 0) return;
    const int slot = (bin & (NB - 1)) * COPIES + copy;
    if constexpr (MASS) {
      const uint64_t w = sm_weight(bits, lf, c);
      if (w == 0) return;
      atomicAdd(reinterpret_cast<unsigned long long*>(&sh.hm[slot]), static_cast<unsigned long long>(w));
    }
    atomicAdd(&sh.hc[slot], 1u);
  });
  sm_hist_finish<NB>(sh);
}

// The copies summed, then the inclusive prefix sums over bins 0 .. 511.
template <int NB>
__device__ __forceinline__ void sm_hist_finish(SmShared& sh) {
  constexpr int COPIES = SM_SLOTS / NB;
  const int t = threadIdx.x;
  __syncthreads();
  if (t < SM_BINS) {
    uint32_t cs = 0;
    uint64_t ms = 0;
    if (t < NB) {
#pragma unroll
      for (int i = 0; i < COPIES; ++i) {
        cs += sh.hc[t * COPIES + i];
        ms += sh.hm[t * COPIES + i];
      }
    }
    sh.sc[t] = cs;
    sh.sm[t] = ms;
  }
  __syncthreads();
  if (t < 64) {  // one wave: 8 bins a lane in turn, then the lanes' totals by shuffles
    uint32_t pc[8];
    uint64_t pm[8];
    uint32_t cs = 0;
    uint64_t ms = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cs += sh.sc[8 * t + i];
      ms += sh.sm[8 * t + i];
      pc[i] = cs;
      pm[i] = ms;
    }
    uint32_t ic = cs;
    uint64_t im = ms;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t uc = __shfl_up(ic, o);
      const unsigned long long um = __shfl_up(static_cast<unsigned long long>(im), o);
      if (t >= o) {
        ic += uc;
        im += um;
      }
    }
    const uint32_t ec = ic - cs;  // exclusive
    const uint64_t em = im - ms;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sh.sc[8 * t + i] = pc[i] + ec;
      sh.sm[8 * t + i] = pm[i] + em;
    }
  }
  __syncthreads();
}

// The lowest bin in [0, 512) for which pred holds, or 512.
template <class P>
__device__ __forceinline__ int sm_first(SmShared& sh, P&& pred) {
  const int t = threadIdx.x;
  if (t == 0) sh.found = SM_BINS;
  __syncthreads();
  if (t < SM_BINS && pred(t)) atomicMin(&sh.found, t);
  __syncthreads();
  const int r = sh.found;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(SM_THREADS) void sample_kernel(const uint16_t* __restrict__ logits, int64_t stride,
                                                            const float* __restrict__ temperature,
                                                            const int32_t* __restrict__ top_k,
                                                            const float* __restrict__ top_p,
                                                            const uint64_t* __restrict__ seeds, uint64_t counter,
                                                            int32_t* __restrict__ out, int V) {
  __shared__ SmShared sh;
  const int64_t m = blockIdx.x;
  const int t = threadIdx.x;
  const int nchunks = V >> 3;
  const uint16_t* const row = logits + m * stride;

  // read before pass A, which counts keys only for a row that will sample
  float T = temperature ? temperature[m] : 0.f;
  const bool sampled = T > 0.f;  // false for a NaN

  // pass A: (key, ~index), the maximum; counts over the high byte.  Walk order is descending key: bin = 255 - byte.
  if (sampled) sm_hist_zero(sh);
  uint64_t best = 0;
  const int copy = t & 15;
  sm_for_each(row, nchunks, [&](int idx, uint32_t bits) {
    const uint32_t key = sm_key(bits);
    const uint64_t v = (static_cast<uint64_t>(key) << 32) | (0xffffffffu - static_cast<uint32_t>(idx));
    best = v > best ? v : best;
    if (sampled) atomicAdd(&sh.hc[(255 - static_cast<int>(key >> 8)) * 16 + copy], 1u);
  });
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t v = __shfl_xor(static_cast<unsigned long long>(best), o);
    best = v > best ? v : best;
  }
  if ((t & 63) == 0) sh.red[t >> 6] = best;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SM_WAVES; ++i) best = sh.red[i] > best ? sh.red[i] : best;
  const int first = static_cast<int>(0xffffffffu - static_cast<uint32_t>(best));
  const uint32_t kf = static_cast<uint32_t>(best >> 32);
  if (!sampled || !(kf > 0x007fu && kf < 0xff80u)) {  // greedy, or the maximum is a NaN or an infinity
    if (t == 0) out[m] = first;
    return;
  }
  const float lf = __uint_as_float((kf >= 0x8000u ? kf & 0x7fffu : ~kf & 0xffffu) << 16);
  T = fminf(fmaxf(T, 0x1p-16f), 0x1p16f);
  const float c = 0x1.715476p+0f / T;
  const int kin = top_k ? top_k[m] : 0;
  const uint32_t k = (kin <= 0 || kin >= V) ? static_cast<uint32_t>(V) : static_cast<uint32_t>(kin);
  float p = top_p ? top_p[m] : 1.0f;
  const bool nocut = !(p < 1.0f);  // NaN as well
  if (p < 0.f) p = 0.f;
  const SmSource whole{row, nchunks, -1};

  // the k-th key over all tokens.  Weights do not decrease with the key, so the tokens of weight > 0 are the head of
  // the descending order, and the tokens of weight 0 that this S holds change neither a mass nor a draw.
  sm_hist_finish<256>(sh);
  const int b1 = sm_first(sh, [&](int b) { return b < 256 && sh.sc[b] >= k; }) & 255;
  const uint32_t above1 = b1 ? sh.sc[b1 - 1] : 0;
  // pass C: the low byte inside bin b1
  sm_hist_pass<256, false>(sh, whole, lf, c, [&](uint32_t key, int) {
    return 255 - static_cast<int>(key >> 8) == b1 ? 255 - static_cast<int>(key & 255u) : -1;
  });
  const int b2 = sm_first(sh, [&](int b) { return b < 256 && above1 + sh.sc[b] >= k; }) & 255;
  const uint32_t kk = (static_cast<uint32_t>(255 - b1) << 8) | static_cast<uint32_t>(255 - b2);
  const uint32_t c2lo = b2 ? sh.sc[b2 - 1] : 0;
  const uint32_t gsize = sh.sc[b2] - c2lo;
  const uint32_t j = k - (above1 + c2lo);  // members of the k-th key's group that are in S; >= 1
  int idx_cut = 0x7fffffff;
  if (j < gsize) {
    // passes D and E: the j-th lowest index of the group
    sm_hist_pass<512, false>(sh, whole, lf, c, [&](uint32_t key, int idx) { return key == kk ? idx >> 9 : -1; });
    const int bi = sm_first(sh, [&](int b) { return sh.sc[b] >= j; }) & 511;
    const uint32_t jj = j - (bi ? sh.sc[bi - 1] : 0);
    sm_hist_pass<512, false>(sh, whole, lf, c,
                             [&](uint32_t key, int idx) { return key == kk && (idx >> 9) == bi ? idx & 511 : -1; });
    const int bj = sm_first(sh, [&](int b) { return sh.sc[b] >= jj; }) & 511;
    idx_cut = (bi << 9) | bj;
  }
  auto in_s = [&](uint32_t key, int idx) { return key > kk || (key == kk && idx <= idx_cut); };

  // a small S moves into LDS; the slots are claimed in any order, which no sum below depends on
  SmSource src = whole;
  const bool listed = k <= static_cast<uint32_t>(SM_LIST);
  if (listed) {
    if (t == 0) sh.n = 0;
    __syncthreads();
    sm_for_each(row, nchunks, [&](int idx, uint32_t bits) {
      if (!in_s(sm_key(bits), idx)) return;
      const uint32_t slot = atomicAdd(&sh.n, 1u);
      if (slot < static_cast<uint32_t>(SM_LIST)) sh.list[slot] = (static_cast<uint64_t>(idx) << 16) | bits;
    });
    __syncthreads();
    src.n = static_cast<int>(sh.n < static_cast<uint32_t>(SM_LIST) ? sh.n : SM_LIST);  // it is k
  }
  auto sel_s = [&](uint32_t key, int idx) { return listed || in_s(key, idx); };

  // top-p: the first group, by descending key, at which the mass reaches p Z
  uint32_t tkey = kk;
  uint64_t ZN = 0;
  if (!nocut) {
    // pass F: the masses of S over the high byte
    sm_hist_pass<256, true>(sh, src, lf, c,
                            [&](uint32_t key, int idx) { return sel_s(key, idx) ? 255 - static_cast<int>(key >> 8) : -1; });
    ZN = sh.sm[SM_BINS - 1];  // Z, if no group is found below
    const double thr = static_cast<double>(p) * static_cast<double>(ZN);
    const int B = sm_first(sh, [&](int b) {
      return b < 256 && sh.sc[b] - (b ? sh.sc[b - 1] : 0) > 0 && static_cast<double>(sh.sm[b]) >= thr;
    });
    if (B < 256) {
      // pass G: the low byte inside bin B
      const uint64_t base = B ? sh.sm[B - 1] : 0;
      sm_hist_pass<256, true>(sh, src, lf, c, [&](uint32_t key, int idx) {
        return sel_s(key, idx) && 255 - static_cast<int>(key >> 8) == B ? 255 - static_cast<int>(key & 255u) : -1;
      });
      const int b = sm_first(sh, [&](int b) {
        return b < 256 && sh.sc[b] - (b ? sh.sc[b - 1] : 0) > 0 && static_cast<double>(base + sh.sm[b]) >= thr;
      });
      if (b < 256) {
        tkey = (static_cast<uint32_t>(255 - B) << 8) | static_cast<uint32_t>(255 - b);
        ZN = base + sh.sm[b];
      }
      __syncthreads();
    }
  }

  // the draw: the lowest index of N whose inclusive prefix mass, in index order, exceeds target.  N is what S holds
  // down to the key tkey.
  auto in_n = [&](uint32_t key, int idx) { return key >= tkey && sel_s(key, idx); };
  sm_hist_pass<512, true>(sh, src, lf, c, [&](uint32_t key, int idx) { return in_n(key, idx) ? idx >> 9 : -1; });
  if (nocut) ZN = sh.sm[SM_BINS - 1];
  const uint64_t a = mix64(seeds[m] + kGolden);
  const uint64_t r = mix64(a + (counter + 1ull) * kGolden);
  const uint64_t target = __umul64hi(r, ZN);
  const int bi = sm_first(sh, [&](int b) { return sh.sm[b] > target; });
  const uint64_t base = (bi > 0 && bi < SM_BINS) ? sh.sm[bi - 1] : 0;
  sm_hist_pass<512, true>(sh, src, lf, c, [&](uint32_t key, int idx) {
    return in_n(key, idx) && (idx >> 9) == bi ? idx & 511 : -1;
  });
  const int bj = sm_first(sh, [&](int b) { return base + sh.sm[b] > target; });
  int token = (bi << 9) | bj;
  if (bi >= SM_BINS || bj >= SM_BINS || token >= V) token = first;  // never reached: the masses add up to Z_N
  if (t == 0) out[m] = token;
}

__global__ __launch_bounds__(EG_THREADS) void embed_gather_kernel(const uint16_t* __restrict__ table,
                                                                  int64_t table_stride,
                                                                  const int32_t* __restrict__ tokens,
                                                                  uint16_t* __restrict__ out, int64_t out_stride,
                                                                  int M, int H, int V) {
  const int c = blockIdx.x * EG_THREADS + threadIdx.x;
  if (c >= (H >> 3)) return;
  for (int64_t m = blockIdx.y; m < M; m += gridDim.y) {
    const int tok = tokens[m];
    i32x4 v = {0, 0, 0, 0};
    if (tok >= 0 && tok < V)
      v = *reinterpret_cast<const i32x4*>(table + static_cast<int64_t>(tok) * table_stride + 8 * static_cast<int64_t>(c));
    *reinterpret_cast<i32x4*>(out + m * out_stride + 8 * static_cast<int64_t>(c)) = v;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct SmSpan {  // [p, p + bytes); p == nullptr: nothing
  const void* p;
  uint64_t bytes;
};

static bool sm_overlap(const SmSpan& a, const SmSpan& b) {
  if (!a.p || !b.p) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

static int sm_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

struct SampleArgs {
  const void* logits;
  int64_t stride;
  const float* temperature;
  const int32_t* top_k;
  const float* top_p;
  const uint64_t* seeds;
  uint64_t counter;
  int32_t* out;
  int M, V;
};

static int sample_validate(const char* who, const SampleArgs& a) {
  if (a.M < 1) return sm_refuse(who, "need M >= 1");
  if (a.V < 8 || a.V > SM_MAX_V || a.V % 8) return sm_refuse(who, "need 8 <= V <= 262144 and V % 8 == 0");
  if (a.stride != 0 && (a.stride < a.V || a.stride % 8))
    return sm_refuse(who, "need logits_stride == 0, or logits_stride >= V and logits_stride % 8 == 0");
  if (!a.logits || !a.out) return sm_refuse(who, "logits and tokens_out must not be NULL");
  if (a.temperature && !a.seeds) return sm_refuse(who, "seeds may be NULL only when temperature is NULL");
  if (reinterpret_cast<uintptr_t>(a.logits) % 16) return sm_refuse(who, "logits must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.temperature) | reinterpret_cast<uintptr_t>(a.top_k) |
       reinterpret_cast<uintptr_t>(a.top_p) | reinterpret_cast<uintptr_t>(a.out)) % 4)
    return sm_refuse(who, "temperature, top_k, top_p and tokens_out must be 4-B aligned");
  if (reinterpret_cast<uintptr_t>(a.seeds) % 8) return sm_refuse(who, "seeds must be 8-B aligned");
  const uint64_t rows = static_cast<uint64_t>(a.M);
  const SmSpan lg{a.logits, ((rows - 1) * static_cast<uint64_t>(a.stride) + static_cast<uint64_t>(a.V)) * 2},
      tm{a.temperature, rows * 4}, tk{a.top_k, rows * 4}, tp{a.top_p, rows * 4}, sd{a.seeds, rows * 8},
      o{a.out, rows * 4};
  if (sm_overlap(o, lg) || sm_overlap(o, tm) || sm_overlap(o, tk) || sm_overlap(o, tp) || sm_overlap(o, sd))
    return sm_refuse(who, "tokens_out must not overlap logits, temperature, top_k, top_p or seeds");
  return 0;
}

static int sample_run(const char* who, void* stream, const SampleArgs& a) {
  hipLaunchKernelGGL(sample_kernel, dim3(a.M), dim3(SM_THREADS), 0, S(stream), static_cast<const uint16_t*>(a.logits),
                     a.stride, a.temperature, a.top_k, a.top_p, a.seeds, a.counter, a.out, a.V);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct EmbedArgs {
  const void* table;
  int64_t table_stride;
  const int32_t* tokens;
  void* out;
  int64_t out_stride;
  int M, H, V;
};

static int embed_validate(const char* who, const EmbedArgs& a) {
  if (a.M < 1) return sm_refuse(who, "need M >= 1");
  if (a.V < 1) return sm_refuse(who, "need V >= 1");
  if (a.H < 8 || a.H % 8) return sm_refuse(who, "need H >= 8 and H % 8 == 0");
  if (a.table_stride < a.H || a.table_stride % 8)
    return sm_refuse(who, "need table_stride >= H and table_stride % 8 == 0");
  if (a.out_stride < a.H || a.out_stride % 8) return sm_refuse(who, "need out_stride >= H and out_stride % 8 == 0");
  if (!a.table || !a.tokens || !a.out) return sm_refuse(who, "table, tokens and out must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.table) | reinterpret_cast<uintptr_t>(a.out)) % 16)
    return sm_refuse(who, "table and out must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(a.tokens) % 4) return sm_refuse(who, "tokens must be 4-B aligned");
  const uint64_t h = static_cast<uint64_t>(a.H);
  const SmSpan tb{a.table, (static_cast<uint64_t>(a.V - 1) * static_cast<uint64_t>(a.table_stride) + h) * 2},
      tk{a.tokens, static_cast<uint64_t>(a.M) * 4},
      o{a.out, (static_cast<uint64_t>(a.M - 1) * static_cast<uint64_t>(a.out_stride) + h) * 2};
  if (sm_overlap(o, tb) || sm_overlap(o, tk)) return sm_refuse(who, "out must not overlap table or tokens");
  return 0;
}

static int embed_run(const char* who, void* stream, const EmbedArgs& a) {
  const int nchunks = a.H / 8;
  const dim3 grid((nchunks + EG_THREADS - 1) / EG_THREADS, a.M < EG_MAX_GRID_ROWS ? a.M : EG_MAX_GRID_ROWS);
  hipLaunchKernelGGL(embed_gather_kernel, grid, dim3(EG_THREADS), 0, S(stream), static_cast<const uint16_t*>(a.table),
                     a.table_stride, a.tokens, static_cast<uint16_t*>(a.out), a.out_stride, a.M, a.H, a.V);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

int gsx_sample(void* stream, const void* logits, int64_t logits_stride, const float* temperature,
               const int32_t* top_k, const float* top_p, const uint64_t* seeds, uint64_t counter,
               int32_t* tokens_out, int M, int V) {
  const SampleArgs a{logits, logits_stride, temperature, top_k, top_p, seeds, counter, tokens_out, M, V};
  if (int rc = sample_validate("gsx_sample", a)) return rc;
  return sample_run("gsx_sample", stream, a);
}

int gsx_event_time_sample(void* stream, const void* logits, int64_t logits_stride, const float* temperature,
                          const int32_t* top_k, const float* top_p, const uint64_t* seeds, uint64_t counter,
                          int32_t* tokens_out, int M, int V, int iters, float* ms) {
  const SampleArgs a{logits, logits_stride, temperature, top_k, top_p, seeds, counter, tokens_out, M, V};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = sample_validate("gsx_sample", a)) return rc;
  return event_time(stream, iters, ms, [&] { return sample_run("gsx_sample", stream, a); });
}

int gsx_embed_gather(void* stream, const void* table, int64_t table_stride, const int32_t* tokens, void* out,
                     int64_t out_stride, int M, int H, int V) {
  const EmbedArgs a{table, table_stride, tokens, out, out_stride, M, H, V};
  if (int rc = embed_validate("gsx_embed_gather", a)) return rc;
  return embed_run("gsx_embed_gather", stream, a);
}

int gsx_event_time_embed_gather(void* stream, const void* table, int64_t table_stride, const int32_t* tokens,
                                void* out, int64_t out_stride, int M, int H, int V, int iters, float* ms) {
  const EmbedArgs a{table, table_stride, tokens, out, out_stride, M, H, V};
  if (int rc = embed_validate("gsx_embed_gather", a)) return rc;
  return event_time(stream, iters, ms, [&] { return embed_run("gsx_embed_gather", stream, a); });
}

}  // extern "C"
