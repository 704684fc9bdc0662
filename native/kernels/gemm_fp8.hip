// fp8 MFMA GEMM family for the pod workload: C[M][N] (bf16) = A[M][K] * B[N][K]^T, OCP e4m3 operands
// (torch.float8_e4m3fn), fp32 accumulate, optional scales in the epilogue.  C ABI in gsx_kernels.h.
//
// The schedules, the tile map, the swizzle and the epilogue are gemm_tile.h's, the ones the bf16 family (gemm.hip)
// runs: a row of a K-tile is 128 B there (64 bf16) and here (128 fp8), so staging and LDS reads are the same
// instructions.  What differs is the MFMA burst (the operand kinds Fp8K128 and Fp8K32 of gemm_tile.h) and that the
// accumulator is scaled in fp32 before it is converted: c = bf16((acc * sa[row]) * sb[col]).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gemm_tile.h"
#include "gsx_internal.h"
#include "gsx_kernels.h"

namespace gsxgemm {

// The scale arguments are checked here, the rest by launch(); nothing touches the device before both have passed.
// The kernels get (nullptr, nullptr, 0) for no scales, and the stride of the scale vectors otherwise.
template <auto KERNEL, int THREADS, int LDS, int BM, int BN>
int launch_fp8(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
               const float* sa, const float* sb, int mode) {
  char msg[160];
  if (mode != GSX_GEMM_SCALE_NONE && mode != GSX_GEMM_SCALE_TENSOR && mode != GSX_GEMM_SCALE_ROW) {
    std::snprintf(msg, sizeof(msg), "%s: unknown scale_mode %d", who, mode);
    return fail_arg(msg);
  }
  if (mode == GSX_GEMM_SCALE_NONE) {
    sa = sb = nullptr;
  } else if (!sa || !sb) {
    std::snprintf(msg, sizeof(msg), "%s: scale_a and scale_b must not be NULL in this scale_mode", who);
    return fail_arg(msg);
  } else if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) % 4) {
    std::snprintf(msg, sizeof(msg), "%s: scale_a and scale_b must be 4-B aligned", who);
    return fail_arg(msg);
  }
  return launch<KERNEL, uint8_t, THREADS, LDS, BM, BN>(who, s, A, B, C, M, N, K, sa, sb,
                                                       mode == GSX_GEMM_SCALE_ROW ? 1 : 0);
}

struct Fp8Cfg {
  const char* name;
  int bm, bn;
  int (*launch)(const char* who, hipStream_t s, const void* A, const void* B, void* C, int M, int N, int K,
                const float* sa, const float* sb, int mode);
};
// the kernels of gemm_tile.h with Scaled's members (sa, sb, stride) as their arguments after K
template <class OP, int BM, int BN, int WM, int WN, int GM>
constexpr Fp8Cfg plain(const char* name) {
  constexpr auto kernel = &gemm_kernel<OP, BM, BN, WM, WN, GM, const float*, const float*, int>;
  return {name, BM, BN, &launch_fp8<kernel, WM * WN * 64, 2 * (BM + BN) * ROW_BYTES, BM, BN>};
}
template <class OP, int GM>
constexpr Fp8Cfg phased(const char* name) {
  constexpr auto kernel = &gemm_phased_kernel<OP, GM, false, const float*, const float*, int>;
  return {name, 256, 256, &launch_fp8<kernel, 512, 8 * PH_HALF, 256, 256>};
}

constexpr Fp8Cfg kFp8Cfgs[] = {
    plain<Fp8K128, 128, 128, 2, 2, 8>("128x128/4w"),
    phased<Fp8K128, 4>("256x256/8w-phased-g4"),
    phased<Fp8K32, 4>("256x256/8w-phased-g4-mfma32"),  // ablation: what the K=128 instruction buys
};
constexpr int kNumFp8Cfgs = sizeof(kFp8Cfgs) / sizeof(kFp8Cfgs[0]);
// the two rows gsx_gemm_fp8_nt dispatches to
constexpr int kFp8Grouped128 = 0, kFp8Phased = 1;

static const Fp8Cfg* fp8_row(int cfg) { return cfg >= 0 && cfg < kNumFp8Cfgs ? &kFp8Cfgs[cfg] : nullptr; }

}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_gemm_fp8_cfg_name(int cfg) { return fp8_row(cfg) ? fp8_row(cfg)->name : nullptr; }

int gsx_gemm_fp8_cfg_tile(int cfg, int* bm, int* bn) {
  const Fp8Cfg* c = fp8_row(cfg);
  if (!c) return -1;
  *bm = c->bm;
  *bn = c->bn;
  return 0;
}

int gsx_gemm_fp8_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                               const float* scale_a, const float* scale_b, int scale_mode, int cfg) {
  const Fp8Cfg* c = fp8_row(cfg);
  if (!c) return fail_arg("gsx_gemm_fp8_nt_launch_cfg: unknown config");
  return c->launch("gsx_gemm_fp8_nt_launch_cfg", S(stream), A, B, C, M, N, K, scale_a, scale_b, scale_mode);
}

int gsx_gemm_fp8_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K, const float* scale_a,
                    const float* scale_b, int scale_mode) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % 128)
    return fail_arg("gsx_gemm_fp8_nt: need M%128==0, N%128==0, K%128==0");
  const Fp8Cfg& c = kFp8Cfgs[(M % 256 == 0 && N % 256 == 0) ? kFp8Phased : kFp8Grouped128];
  return c.launch("gsx_gemm_fp8_nt", S(stream), A, B, C, M, N, K, scale_a, scale_b, scale_mode);
}

int gsx_event_time_gemm_fp8(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                            const float* scale_a, const float* scale_b, int scale_mode, int iters, float* ms) {
  return event_time(stream, iters, ms,
                    [&] { return gsx_gemm_fp8_nt(stream, A, B, C, M, N, K, scale_a, scale_b, scale_mode); });
}

}  // extern "C"
