// What the translation units of MoE prefill share on the host (moe_prefill.hip: router, plan, bf16 grouped GEMM and
// combine; moe_prefill_fp8_block.hip: the block-scaled fp8 grouped GEMM): the size limits, the geometry of the tile plan
// and the helpers of their argument checks.  Internal, like gsx_internal.h.
#pragma once

#include <cstdint>
#include <cstdio>

#include "gsx_internal.h"

namespace gsxgemm {

using namespace gsx;

constexpr int PF_MAX_M = 32768;
constexpr int PF_MAX_E = 1024;
constexpr int PF_MAX_TOPK = 8;
constexpr int PF_BM = 128, PF_BN = 128;  // the grouped GEMMs' block tile; BM is the plan's padding unit

struct PfSpan {  // [p, p + bytes)
  const void* p;
  uint64_t bytes;
};

static inline bool pf_overlap(const PfSpan& a, const PfSpan& b) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

static inline uintptr_t pf_bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }

static inline int pf_refuse(const char* who, const char* rule) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, rule);
  return fail_arg(msg);
}

// the sizes every entry point but the combine shares
static inline int pf_sizes(const char* who, int M, int topk, int E) {
  if (M < 1 || M > PF_MAX_M) return pf_refuse(who, "need 1 <= M <= 32768");
  if (E < 8 || E > PF_MAX_E || E % 8) return pf_refuse(who, "need 8 <= E <= 1024 and E % 8 == 0");
  if (topk < 1 || topk > PF_MAX_TOPK || topk > E) return pf_refuse(who, "need 1 <= topk <= min(8, E)");
  return 0;
}

static inline int64_t pf_tmax(int M, int topk, int E) {
  const int64_t P = static_cast<int64_t>(M) * topk;
  return (P + (E < P ? E : P) * (PF_BM - 1)) / PF_BM;
}
static inline uint64_t pf_plan_ints(int M, int topk, int E) {
  const uint64_t t = static_cast<uint64_t>(pf_tmax(M, topk, E));
  return 4 + t + PF_BM * t;
}

}  // namespace gsxgemm
