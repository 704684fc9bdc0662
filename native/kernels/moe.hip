// Mixture-of-experts decode for the pod workload: the router and the combine around the grouped expert GEMM
// (moe_kernel in gemm_decode.hip, which shares decode_kernel's body).  gsx_moe_route turns M <= 16 rows of bf16 router
// logits into topk expert ids and softmax weights per token and into a plan in device memory that groups the
// P = M topk (token, expert) pairs by expert; gsx_moe_combine adds a token's topk expert outputs with those weights.
// Ids, weights and plan stay on the device, so an MoE layer needs no host synchronisation.  C ABI and numeric contract
// in gsx_kernels.h.
//
// moe_route_kernel: one workgroup of 1024 threads, nothing between workgroups, no atomics.
//   * selection: wave m owns token m.  A lane holds the E / 64 (at most 16) logits l, l + 64, .. of the row as
//     (key << 10 | 1023 - index) + 1, which is distinct for every index and orders by key first and by lower index
//     second; 0 stands for "no logit" and "taken".  topk times: the wave's maximum by xor shuffles, and the lane that
//     holds it zeroes it.  Every lane then knows the topk winners in order and computes the topk weights itself, in
//     the order of j; lane j writes id and weight j.
//   * plan: the P ids meet in LDS.  Thread p marks whether pair p is the first with its expert; behind a barrier
//     thread e scans the P ids once and finds its count, the pairs of lower experts (its begin) and the distinct
//     lower experts (its slot), and an expert with a pair writes its slot and its run of rows in ascending pair
//     order.  Threads 0 .. 127 write the unused slots and rows.
// moe_combine_kernel: a thread owns a 16-B chunk of a token's row; the topk loads are issued before the first is used.
// Contraction is off for the whole file: both contracts round every multiply and add on its own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "bf16_key.h"
#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

#pragma clang fp contract(off)

namespace gsxgemm {

constexpr int MR_THREADS = 1024;
constexpr int MR_WAVES = MR_THREADS / 64;  // the most tokens
constexpr int MR_PER_LANE = 16;            // E <= 1024
constexpr int MR_MAX_TOPK = 8;
constexpr int MR_PAIRS = GSX_MOE_MAX_PAIRS;
constexpr int MC_THREADS = 256;

__device__ __forceinline__ float mr_bf16(uint32_t code) { return __uint_as_float(code << 16); }

__global__ __launch_bounds__(MR_THREADS) void moe_route_kernel(const uint16_t* __restrict__ logits, int64_t stride,
                                                               int32_t* __restrict__ topk_ids,
                                                               float* __restrict__ topk_w, int32_t* __restrict__ plan,
                                                               int M, int E, int topk) {
  __shared__ int32_t ids[MR_PAIRS];
  __shared__ int32_t first[MR_PAIRS];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int P = M * topk;

  if (wid < M) {
    const uint16_t* const row = logits + wid * stride;
    uint32_t comp[MR_PER_LANE];
    static_for<MR_PER_LANE>([&](auto i) {
      const int idx = i * 64 + lane;
      comp[i] = idx < E ? ((sm_key(row[idx]) << 10) | static_cast<uint32_t>(1023 - idx)) + 1u : 0u;
    });
    int id[MR_MAX_TOPK];
    uint32_t code[MR_MAX_TOPK];
    static_for<MR_MAX_TOPK>([&](auto j) {
      id[j] = 0;
      code[j] = 0;
      if (j >= topk) return;  // uniform
      uint32_t best = 0;
#pragma unroll
      for (int i = 0; i < MR_PER_LANE; ++i) best = comp[i] > best ? comp[i] : best;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = __shfl_xor(best, o);
        best = v > best ? v : best;
      }
      // topk <= E: there is a logit left, so best >= 1
#pragma unroll
      for (int i = 0; i < MR_PER_LANE; ++i) comp[i] = comp[i] == best ? 0u : comp[i];
      id[j] = 1023 - static_cast<int>((best - 1u) & 1023u);
      code[j] = row[id[j]];
    });
    // the weights: a softmax over the selected logits, in the order of j
    const float l0 = mr_bf16(code[0]);
    const bool finite0 = (code[0] & 0x7f80u) != 0x7f80u;
    float p[MR_MAX_TOPK];
    float sum = 0.f;
    static_for<MR_MAX_TOPK>([&](auto j) {
      p[j] = 0.f;
      if (j >= topk) return;
      if (!finite0) {
        p[j] = j == 0 ? 1.0f : 0.f;
      } else if ((code[j] & 0x7f80u) != 0x7f80u) {  // -inf and NaN weigh nothing
        const float d = mr_bf16(code[j]) - l0;
        const float x = d * 0x1.715476p+0f;
        p[j] = x == 0.f ? 1.0f : __builtin_amdgcn_exp2f(x);
      }
      sum = j == 0 ? p[j] : sum + p[j];
    });
    static_for<MR_MAX_TOPK>([&](auto j) {
      if (j >= topk || lane != j) return;
      const int pair = wid * topk + j;
      topk_ids[pair] = id[j];
      topk_w[pair] = p[j] / sum;  // sum >= p[0] = 1
      ids[pair] = id[j];
    });
  }
  __syncthreads();
  if (t < P) {
    int f = 1;
    for (int q = 0; q < t; ++q) f = ids[q] == ids[t] ? 0 : f;
    first[t] = f;
  }
  __syncthreads();
  int count = 0, begin = 0, slot = 0, n_active = 0;
  for (int q = 0; q < P; ++q) {
    const int e = ids[q], f = first[q];
    count += e == t;
    begin += e < t;
    slot += (e < t) & f;
    n_active += f;
  }
  int32_t* const slot_expert = plan + 4;
  int32_t* const slot_begin = slot_expert + MR_PAIRS;
  int32_t* const slot_count = slot_begin + MR_PAIRS;
  int32_t* const rows = slot_count + MR_PAIRS;
  if (t == 0) {
    plan[0] = n_active;
    plan[1] = P;
    plan[2] = E;
    plan[3] = 0;
  }
  if (t < E && count > 0) {  // slot < n_active <= P and begin + count <= P, by construction
    slot_expert[slot] = t;
    slot_begin[slot] = begin;
    slot_count[slot] = count;
    int k = begin;
    for (int q = 0; q < P; ++q)
      if (ids[q] == t) rows[k++] = q;
  }
  if (t < MR_PAIRS) {
    if (t >= n_active) {
      slot_expert[t] = -1;
      slot_begin[t] = 0;
      slot_count[t] = 0;
    }
    if (t >= P) rows[t] = -1;
  }
}

__global__ __launch_bounds__(MC_THREADS) void moe_combine_kernel(const uint16_t* __restrict__ Y, int64_t y_stride,
                                                                 const float* __restrict__ topk_w,
                                                                 uint16_t* __restrict__ out, int64_t out_stride,
                                                                 int topk, int H) {
  const int c = blockIdx.x * MC_THREADS + threadIdx.x;
  if (c >= (H >> 3)) return;
  const int64_t m = blockIdx.y;
  i32x4 yv[MR_MAX_TOPK];
  float w[MR_MAX_TOPK];
  static_for<MR_MAX_TOPK>([&](auto j) {
    if (j >= topk) return;
    yv[j] = *reinterpret_cast<const i32x4*>(Y + (m * topk + j) * y_stride + 8 * static_cast<int64_t>(c));
    w[j] = topk_w[m * topk + j];
  });
  float acc[8];
  static_for<MR_MAX_TOPK>([&](auto j) {
    if (j >= topk) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t word = static_cast<uint32_t>(yv[j][e >> 1]);
      const float y = __uint_as_float((e & 1) ? word & 0xffff0000u : word << 16);
      const float prod = w[j] * y;
      acc[e] = j == 0 ? prod : acc[e] + prod;
    }
  });
  i32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = static_cast<int>(f2bf(acc[2 * i]) | (static_cast<uint32_t>(f2bf(acc[2 * i + 1])) << 16));
  *reinterpret_cast<i32x4*>(out + m * out_stride + 8 * static_cast<int64_t>(c)) = o;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct MoeSpan {  // [p, p + bytes)
  const void* p;
  uint64_t bytes;
};

static bool moe_overlap(const MoeSpan& a, const MoeSpan& b) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

static int moe_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

struct RouteArgs {
  const void* logits;
  int64_t stride;
  int32_t* ids;
  float* w;
  int32_t* plan;
  int M, E, topk;
};

static int route_validate(const char* who, const RouteArgs& a) {
  if (a.M < 1 || a.M > MR_WAVES) return moe_refuse(who, "need 1 <= M <= 16");
  if (a.E < 8 || a.E > MR_THREADS || a.E % 8) return moe_refuse(who, "need 8 <= E <= 1024 and E % 8 == 0");
  if (a.topk < 1 || a.topk > MR_MAX_TOPK || a.topk > a.E) return moe_refuse(who, "need 1 <= topk <= min(8, E)");
  if (a.stride < a.E || a.stride % 8) return moe_refuse(who, "need logits_stride >= E and logits_stride % 8 == 0");
  if (!a.logits || !a.ids || !a.w || !a.plan)
    return moe_refuse(who, "logits, topk_ids, topk_w and plan must not be NULL");
  if (reinterpret_cast<uintptr_t>(a.logits) % 16) return moe_refuse(who, "logits must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(a.ids) | reinterpret_cast<uintptr_t>(a.w) | reinterpret_cast<uintptr_t>(a.plan)) % 4)
    return moe_refuse(who, "topk_ids, topk_w and plan must be 4-B aligned");
  const uint64_t pairs = static_cast<uint64_t>(a.M) * a.topk;
  const MoeSpan lg{a.logits, (static_cast<uint64_t>(a.M - 1) * a.stride + a.E) * 2}, id{a.ids, pairs * 4},
      w{a.w, pairs * 4}, pl{a.plan, GSX_MOE_PLAN_INTS * 4ull};
  if (moe_overlap(id, lg) || moe_overlap(w, lg) || moe_overlap(pl, lg) || moe_overlap(id, w) || moe_overlap(id, pl) ||
      moe_overlap(w, pl))
    return moe_refuse(who, "topk_ids, topk_w and plan must not overlap logits or each other");
  return 0;
}

static int route_run(const char* who, void* stream, const RouteArgs& a) {
  hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(MR_THREADS), 0, S(stream),
                     static_cast<const uint16_t*>(a.logits), a.stride, a.ids, a.w, a.plan, a.M, a.E, a.topk);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

struct CombineArgs {
  const void* Y;
  int64_t y_stride;
  const float* w;
  void* out;
  int64_t out_stride;
  int M, topk, H;
};

static int combine_validate(const char* who, const CombineArgs& a) {
  if (a.M < 1 || a.M > MR_WAVES) return moe_refuse(who, "need 1 <= M <= 16");
  if (a.topk < 1 || a.topk > MR_MAX_TOPK) return moe_refuse(who, "need 1 <= topk <= 8");
  if (a.H < 8 || a.H % 8) return moe_refuse(who, "need H >= 8 and H % 8 == 0");
  if (a.y_stride < a.H || a.y_stride % 8) return moe_refuse(who, "need y_stride >= H and y_stride % 8 == 0");
  if (a.out_stride < a.H || a.out_stride % 8) return moe_refuse(who, "need out_stride >= H and out_stride % 8 == 0");
  if (!a.Y || !a.w || !a.out) return moe_refuse(who, "Y, topk_w and out must not be NULL");
  if ((reinterpret_cast<uintptr_t>(a.Y) | reinterpret_cast<uintptr_t>(a.out)) % 16)
    return moe_refuse(who, "Y and out must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(a.w) % 4) return moe_refuse(who, "topk_w must be 4-B aligned");
  const uint64_t pairs = static_cast<uint64_t>(a.M) * a.topk, h = static_cast<uint64_t>(a.H);
  const MoeSpan y{a.Y, ((pairs - 1) * a.y_stride + h) * 2}, w{a.w, pairs * 4},
      o{a.out, (static_cast<uint64_t>(a.M - 1) * a.out_stride + h) * 2};
  if (moe_overlap(o, y) || moe_overlap(o, w)) return moe_refuse(who, "out must not overlap Y or topk_w");
  return 0;
}

static int combine_run(const char* who, void* stream, const CombineArgs& a) {
  const dim3 grid((a.H / 8 + MC_THREADS - 1) / MC_THREADS, a.M);
  hipLaunchKernelGGL(moe_combine_kernel, grid, dim3(MC_THREADS), 0, S(stream), static_cast<const uint16_t*>(a.Y),
                     a.y_stride, a.w, static_cast<uint16_t*>(a.out), a.out_stride, a.topk, a.H);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, who);
}

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

int gsx_moe_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids, float* topk_w,
                  int32_t* plan, int M, int E, int topk) {
  const RouteArgs a{logits, logits_stride, topk_ids, topk_w, plan, M, E, topk};
  if (int rc = route_validate("gsx_moe_route", a)) return rc;
  return route_run("gsx_moe_route", stream, a);
}

int gsx_event_time_moe_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids, float* topk_w,
                             int32_t* plan, int M, int E, int topk, int iters, float* ms) {
  const RouteArgs a{logits, logits_stride, topk_ids, topk_w, plan, M, E, topk};
  // refused before the events are made, under the name of the entry point that is timed
  if (int rc = route_validate("gsx_moe_route", a)) return rc;
  return event_time(stream, iters, ms, [&] { return route_run("gsx_moe_route", stream, a); });
}

int gsx_moe_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out, int64_t out_stride,
                    int M, int topk, int H) {
  const CombineArgs a{Y, y_stride, topk_w, out, out_stride, M, topk, H};
  if (int rc = combine_validate("gsx_moe_combine", a)) return rc;
  return combine_run("gsx_moe_combine", stream, a);
}

int gsx_event_time_moe_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out,
                               int64_t out_stride, int M, int topk, int H, int iters, float* ms) {
  const CombineArgs a{Y, y_stride, topk_w, out, out_stride, M, topk, H};
  if (int rc = combine_validate("gsx_moe_combine", a)) return rc;
  return event_time(stream, iters, ms, [&] { return combine_run("gsx_moe_combine", stream, a); });
}

}  // extern "C"
