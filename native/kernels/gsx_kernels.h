// C ABI of libgsx_kernels.so: the MI355X (gfx950) device-side pieces of the
// GPU-share stack.  The reference has no GPU code at all;
// these are new capabilities that make the shares verifiable on hardware:
//
//  * CU probe            — every workgroup records the hardware XCC / SE / CU /
//                          SIMD it ran on (s_getreg HW_ID, XCC_ID), so a CU
//                          mask (the MPS stand-in of BASELINE.json) can be
//                          checked against what the hardware actually used;
//  * HBM stamp / verify  — a pod's gpu-mem slice is stamped with its tag and
//                          verified later: proves co-resident pods placed by
//                          the binpack allocator really fit and never overlap
//                          (hbm_stamp.hip);
//  * HBM scrub           — the memory test's SOLID write pass, used to wipe a slice
//                          when a pod leaves (and as the HBM roofline probe);
//  * HBM memory test     — pattern write / check / moving-inversions passes at HBM
//                          bandwidth: the device plugin's pre-flight (memtest.hip);
//  * compute test        — a known-answer test of every CU's MFMA, VALU and LDS that
//                          names the physical CUs and SIMDs that answered wrong: the
//                          plugin's compute pre-flight (cutest.hip);
//  * bf16 MFMA GEMM      — the pod workload used to measure isolation
//                          (throughput under per-pod CU partitions);
//  * fp8 MFMA GEMM       — the same workload on OCP e4m3 operands and the K=128
//                          MFMA, with per-tensor or per-row scales (gemm_fp8.hip);
//  * MXFP4 MFMA GEMM     — the same workload on e2m1 operands with e8m0 block scales
//                          on the block-scaled MFMA, and the quantiser that makes
//                          such operands from bf16 (gemm_mxfp4.hip);
//  * decode GEMM / attention — an inference server's decode step: M <= 16 rows against
//                          weights streamed from HBM (gemm_decode.hip), attention
//                          over a paged KV cache in bf16 or e4m3 (attn_decode.hip);
//  * RoPE + KV append    — rotates Q and K and writes the new tokens' K and V into
//                          their page slots, quantised for an e4m3 cache: what makes
//                          the cache the attention reads (kv_append.hip);
//  * prefill attention   — causal attention of a chunk of new tokens over the same paged
//                          cache, the compute-bound half of an inference server
//                          (attn_prefill.hip);
//  * add + RMSNorm, SwiGLU — the residual stream, the normalisation and the MLP's activation of
//                          a decoder layer, to bf16 or to e4m3 with a scale per row
//                          (norm_act.hip);
//  * CU-masked streams   — hipExtStreamCreateWithCUMask.
//
// All functions return 0 or a hipError_t value; gsx_last_error() has text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  char name[64];
  char arch[32];
  char pci_bus_id[32];
  uint64_t total_mem;
  int32_t cu_count;
  int32_t xcc_count;  // not reported by HIP; filled from the probe by callers
  int32_t clock_khz;
  int32_t wave_size;
  uint64_t lds_per_block;
} gsx_devinfo;

const char* gsx_last_error(void);
int gsx_device_count(int* n);
int gsx_device_info(int dev, gsx_devinfo* out);
int gsx_mem_info(int dev, uint64_t* free_b, uint64_t* total_b);
int gsx_synchronize(int dev);
// Make `dev` current on the calling thread (native runtime threads launch admission kernels).
int gsx_set_device(int dev);

// streams (mask_words == 0: plain stream)
int gsx_stream_create(int dev, const uint32_t* cu_mask, int mask_words, void** stream);
int gsx_stream_get_mask(void* stream, uint32_t* cu_mask, int mask_words);
int gsx_stream_destroy(void* stream);
int gsx_stream_sync(void* stream);

// memory
int gsx_malloc(int dev, uint64_t bytes, void** ptr);
int gsx_free(void* ptr);
int gsx_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int gsx_memcpy_h2d(void* dst, const void* src, uint64_t bytes);

// CU probe: `blocks` workgroups of 64 threads each spin `spin` iterations and
// record (HW_ID, XCC_ID) into out[2*b] / out[2*b+1].  Runs on `stream`
// (may be a CU-masked stream) and synchronises it.
int gsx_cuprobe(void* stream, int blocks, int spin, uint32_t* out_host);

// HBM stamp/verify (hbm_stamp.hip): 16-byte stamps {tag, offset} every `stride` bytes of
// [base, base+bytes).  stamp launches and returns without synchronising; verify returns the
// number of bad stamps in *bad after one stream sync.
int gsx_hbm_stamp(void* stream, void* base, uint64_t bytes, uint64_t stride, uint64_t tag);
int gsx_hbm_verify(void* stream, const void* base, uint64_t bytes, uint64_t stride, uint64_t tag, uint64_t* bad);
// Batched pod admission.  A pod is made of one or several extents (its slice is not contiguous when the arena
// is fragmented): stamp slices[0, n_stamp), then (verify != 0) verify all n slices, each in one launch per 32
// extents; *bad = total bad stamps.  The bad-stamp counter lives in pinned host memory, so there is no memset /
// copy kernel and exactly one stream sync per call.
typedef struct {
  uint64_t addr;
  uint64_t bytes;
  uint64_t tag;
} gsx_slice;
int gsx_hbm_admit_n(void* stream, const gsx_slice* slices, int n, int n_stamp, int verify, uint64_t stride,
                    uint64_t* bad);

// Fill [base, base+bytes) with a 32-bit pattern (bytes % 16 == 0): gsx_memtest_write's SOLID pass (memtest.hip).
int gsx_hbm_fill(void* stream, void* base, uint64_t bytes, uint32_t pattern);

// bf16 GEMM (gemm.hip): C[M][N] (bf16) = A[M][K] (bf16, row-major) * B[N][K]^T (bf16, row-major), fp32 accumulate.
// A, B and C are 16-B aligned.  Launches on `stream` and returns without synchronising.
// K is limited by the 32-bit offsets inside an operand tile: (max(BM, BN) - 1) * K + 56 < 2^31, which is
// K <= 8421504 for a tile side of 256 and K <= 16909312 for 128; a longer K is rejected.
// gsx_gemm_bf16_nt requires M % 128 == 0, N % 128 == 0, K % 64 == 0 and dispatches to one of the configurations
// below: the phased 256x256 kernel when M and N are multiples of 256, the grouped 128x128 tile otherwise.
int gsx_gemm_bf16_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K);
// The configurations, one table in gemm.hip: index 0 .. 10, each a kernel with a BM x BN block tile and a name
// ("256x256/8w-phased-g4"); most are ablations kept for benchmarking.  _cfg_name returns NULL and _cfg_tile
// nonzero outside the table.  _launch_cfg launches configuration `cfg`, which requires M % BM == 0, N % BN == 0,
// K % 64 == 0.
const char* gsx_gemm_cfg_name(int cfg);
int gsx_gemm_cfg_tile(int cfg, int* bm, int* bn);
int gsx_gemm_bf16_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int cfg);

// elapsed milliseconds of `iters` back-to-back gsx_gemm_bf16_nt on `stream`, by hip events (for benches)
int gsx_event_time_gemm(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int iters,
                        float* ms);

// fp8 GEMM (gemm_fp8.hip): C[M][N] (bf16) = A[M][K] * B[N][K]^T with A and B in OCP e4m3 (torch.float8_e4m3fn, not
// the fnuz encoding), row-major, fp32 accumulate; the same schedules as the bf16 kernels on
// v_mfma_f32_16x16x128_f8f6f4.  Before the conversion to bf16 the accumulator is scaled by two fp32 multiplies in
// this order, c = bf16((acc * sa) * sb):
//   GSX_GEMM_SCALE_NONE    no multiply; scale_a and scale_b are ignored
//   GSX_GEMM_SCALE_TENSOR  sa = scale_a[0], sb = scale_b[0]
//   GSX_GEMM_SCALE_ROW     sa = scale_a[row] (M floats), sb = scale_b[col] (N floats)
// The scales are in device memory, non-NULL and 4-B aligned unless the mode is NONE; A, B and C are 16-B aligned.
// Launches on `stream` and returns without synchronising; everything is validated before the first device call.
// K is limited by the 32-bit offsets inside an operand tile: (max(BM, BN) - 1) * K + 112 < 2^31, which is
// K <= 8421504 for a tile side of 256 and K <= 16909312 for 128 (multiples of 128); a longer K is rejected.
// gsx_gemm_fp8_nt requires M % 128 == 0, N % 128 == 0, K % 128 == 0 and dispatches like gsx_gemm_bf16_nt: the phased
// 256x256 kernel when M and N are multiples of 256, the grouped 128x128 tile otherwise.
enum { GSX_GEMM_SCALE_NONE = 0, GSX_GEMM_SCALE_TENSOR = 1, GSX_GEMM_SCALE_ROW = 2 };
int gsx_gemm_fp8_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K, const float* scale_a,
                    const float* scale_b, int scale_mode);
// The fp8 configurations, a table of their own in gemm_fp8.hip: 0 "128x128/4w", 1 "256x256/8w-phased-g4" (the
// dispatched one), 2 "256x256/8w-phased-g4-mfma32" (v_mfma_f32_16x16x32_fp8_fp8, which runs at the bf16 rate: the
// ablation of the K=128 instruction).  Same conventions as the bf16 table; _launch_cfg requires M % BM == 0,
// N % BN == 0, K % 128 == 0.
const char* gsx_gemm_fp8_cfg_name(int cfg);
int gsx_gemm_fp8_cfg_tile(int cfg, int* bm, int* bn);
int gsx_gemm_fp8_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                               const float* scale_a, const float* scale_b, int scale_mode, int cfg);
// elapsed milliseconds of `iters` back-to-back gsx_gemm_fp8_nt on `stream`, by hip events (for benches)
int gsx_event_time_gemm_fp8(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                            const float* scale_a, const float* scale_b, int scale_mode, int iters, float* ms);

// MXFP4 GEMM (gemm_mxfp4.hip), on v_mfma_scale_f32_16x16x128_f8f6f4 with the same schedules as the other families.
// The operand format:
//   A[M][K], B[N][K]   OCP e2m1, two per byte, row-major (torch.float4_e2m1fn_x2): a row is K / 2 bytes, element k
//                      is in byte k / 2, the low nibble for even k and the high nibble for odd k
//   scale_a[M][K / 32], scale_b[N][K / 32]
//                      bytes, row-major, e8m0 (torch.float8_e8m0fnu): code c means 2^(c - 127) and applies to
//                      elements 32 g .. 32 g + 31 of its row, g the column of the code.  This plain layout is the
//                      one in memory; what the instruction wants is arranged inside the kernels.
//   C[i][j] = bf16( sum over g of 2^(sa[i][g] - 127) * 2^(sb[j][g] - 127) * sum over k in block g of A[i][k] B[j][k] )
//                      accumulated in fp32; C is bf16, row-major.
// Scale codes 1 .. 254 are the contract.  With code 0 (2^-127) or 255 (NaN) anywhere the result is whatever the
// instruction gives.  A, B, C, scale_a and scale_b are 16-B aligned and not NULL.  Launches on `stream` and returns
// without synchronising; everything is validated before the first device call.
// K is limited by the 32-bit byte offsets inside an operand tile: (max(BM, BN) - 1) * K / 2 + 112 < 2^31, which is
// K <= 16843008 for a tile side of 256 and K <= 33818624 for 128 (multiples of 256); a longer K is rejected.
// gsx_gemm_mxfp4_nt requires M % 128 == 0, N % 128 == 0, K % 256 == 0 and dispatches like gsx_gemm_fp8_nt.
int gsx_gemm_mxfp4_nt(void* stream, const void* A, const void* B, void* C, int M, int N, int K, const void* scale_a,
                      const void* scale_b);
// The mxfp4 configurations, a table of their own in gemm_mxfp4.hip: 0 "128x128/4w", 1 "256x256/8w-phased-g4" (the
// dispatched one), 2 "256x256/8w-phased-g4-unit" (the same kernel without the scale path: every scale is taken as
// code 127 and scale_a and scale_b are validated but not read; the ablation of the scale path).  Same conventions as
// the fp8 table; _launch_cfg requires M % BM == 0, N % BN == 0, K % 256 == 0.
const char* gsx_gemm_mxfp4_cfg_name(int cfg);
int gsx_gemm_mxfp4_cfg_tile(int cfg, int* bm, int* bn);
int gsx_gemm_mxfp4_nt_launch_cfg(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                                 const void* scale_a, const void* scale_b, int cfg);
// elapsed milliseconds of `iters` back-to-back gsx_gemm_mxfp4_nt on `stream`, by hip events (for benches)
int gsx_event_time_gemm_mxfp4(void* stream, const void* A, const void* B, void* C, int M, int N, int K,
                              const void* scale_a, const void* scale_b, int iters, float* ms);
// The quantiser: bf16 X[R][K] (K % 32 == 0) -> Q[R][K / 2] and S[R][K / 32] in the format above, per OCP MX v1.0.
// Per block of 32, e = floor(log2(max|x|)) - 2 and the code is clamp(e + 127, 1, 254); the elements are x / 2^e
// rounded to nearest even onto the e2m1 grid, saturated to +-6, the sign of a zero kept.  An all-zero block gets code
// 127; a block that holds an inf or a NaN gets code 255 and unspecified elements (outside the GEMM's contract).  X
// and Q are 16-B aligned.  Launches on `stream` and returns without synchronising.
int gsx_quant_mxfp4(void* stream, const void* X, void* Q, void* S, int R, int K);

// Decode GEMM (gemm_decode.hip): C[M][N] (bf16) = A[M][K] * B[N][K]^T with 1 <= M <= 16, a few activation rows against
// weights that are read once, bound by HBM bandwidth.  B goes from global memory straight to the MFMA's registers; a
// workgroup owns a strip of 16 (or 32) columns and its waves split K.  `kind` selects the operand format, each exactly
// that of the family above with the same name:
//   GSX_DECODE_BF16   A and B bf16; scale_a and scale_b NULL and scale_mode GSX_GEMM_SCALE_NONE; K % 64 == 0
//   GSX_DECODE_FP8    A and B OCP e4m3; scale_a, scale_b and scale_mode as gsx_gemm_fp8_nt takes them (fp32, M and N
//                     of them with GSX_GEMM_SCALE_ROW), c = bf16((acc * sa) * sb); K % 128 == 0
//   GSX_DECODE_MXFP4  A and B e2m1, two per byte; scale_a[M][K / 32] (exactly M rows) and scale_b[N][K / 32] e8m0,
//                     plain row-major, codes 1 .. 254, non-NULL and 16-B aligned; scale_mode NONE; K % 256 == 0
// A, B and C are 16-B aligned and not NULL; N % 16 == 0.  Nothing is read of A or scale_a past row M - 1 and nothing
// written of C past it.  Row offsets into B, scale_b and C are 64-bit (B may exceed 4 GiB); K is limited only by int.
// Accumulation is fp32 with one rounding to bf16.  The result is deterministic and does not depend on where
// workgroups run: there is no communication between them.  For general inputs the summation order (the K-tiles a
// wave takes, then the waves in order) differs from that of gsx_gemm_*_nt, and so may the last bits.
// Launches on `stream` and returns without synchronising; everything is validated before the first device call.
// gsx_decode_gemm_nt picks a configuration by N and K alone (the rule is at decode_pick() in gemm_decode.hip).
enum { GSX_DECODE_BF16 = 0, GSX_DECODE_FP8 = 1, GSX_DECODE_MXFP4 = 2 };
int gsx_decode_gemm_nt(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                       const void* scale_a, const void* scale_b, int scale_mode);
// The decode configurations, one table for the three kinds: 0 "16/4w-f4", 1 "16/8w-f4", 2 "16/8w-f8", 3 "16/16w-f4",
// 4 "32/8w-f4", 5 "16/8w-f4-nt" (non-temporal loads of B; ablation): columns of a strip (BN) / waves per workgroup -
// K-tiles a wave keeps in flight.  _cfg_name returns NULL and _cfg_shape nonzero outside the table.  _launch_cfg
// requires N % BN == 0 and otherwise what gsx_decode_gemm_nt requires.
const char* gsx_decode_gemm_cfg_name(int cfg);
int gsx_decode_gemm_cfg_shape(int cfg, int* bn, int* waves, int* inflight);
int gsx_decode_gemm_nt_launch_cfg(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                                  const void* scale_a, const void* scale_b, int scale_mode, int cfg);
// elapsed milliseconds of `iters` back-to-back gsx_decode_gemm_nt on `stream`, by hip events (for benches)
int gsx_event_time_decode_gemm(void* stream, int kind, const void* A, const void* B, void* C, int M, int N, int K,
                               const void* scale_a, const void* scale_b, int scale_mode, int iters, float* ms);

// Decode attention over a paged KV cache (attn_decode.hip): one new token per sequence, grouped-query attention in
// which Hq query heads share Hkv KV heads in groups of G = Hq / Hkv.
//   Q[B][Hq][D], O[B][Hq][D]              bf16, D == 128
//   K_cache, V_cache [num_pages][Hkv][page][D]
//                                         bf16 (GSX_ATTN_KV_BF16) or OCP e4m3 (GSX_ATTN_KV_FP8, torch.float8_e4m3fn),
//                                         both the same; one (page, KV head) is a contiguous run of page * D elements
//   block_table[B][table_stride]          int32, device memory: entry i of a row is the page of tokens i * page ..
//   seq_lens[B]                           int32, device memory
// Requirements: Hq % Hkv == 0 and G <= 16; page % 16 == 0 and 16 <= page <= 256; 1 <= max_seq_len <= table_stride *
// page; every pointer non-NULL, Q, the caches, O and a workspace 16-B aligned, block_table and seq_lens 4-B aligned;
// k_scale and v_scale (host floats, the per-tensor dequantisation factors of an e4m3 cache) exactly 1.0f for bf16.
// A seq_lens[b] above max_seq_len is clamped to it (one below 0 to 0) and a page index into [0, num_pages) by an
// unsigned min, so no input makes the kernel read outside the caches.  Offsets into the caches are 64-bit: a cache
// may exceed 4 GiB.  Everything is validated before the first device call; launches on `stream` and returns without
// synchronising.
// Numerics, per (sequence, query head g), over the tokens t < seq_len:
//   x[g][t] = (q_g . k_t) * (scale * k_scale * log2 e)   fp32; bf16 products accumulated in fp32 on
//                                                        v_mfma_f32_16x16x32_bf16; e4m3 K and V are converted to
//                                                        bf16 in registers, which is exact
//   p = exp2(x - m)                                      fp32, m a running maximum
//   l = sum of p                                         fp32, of the unrounded p
//   P = bf16(p), round to nearest even                   the operand of the PV MFMA, accumulated in fp32
//   O = bf16((acc / l) * v_scale)                        rounded once
// Partial results are triples (m, l, acc), merged in fp32 in a fixed order: the tiles of 32 tokens a wave takes, the
// waves of a workgroup by index, then the splits by index; a partial without a token has m = -inf, l = 0 and weight
// 0.  A sequence of length 0 gives a row of zeros.  Slots at or past seq_len and block-table entries past the last
// used page contribute nothing, whatever the cache holds there (NaN and inf included): their x is replaced by -inf
// and their V by zeros.  The result is deterministic and does not depend on where workgroups run: nothing passes
// between workgroups inside a launch.  It depends on `splits`.
// Split-KV: with splits > 1 each (sequence, KV head) is cut into `splits` runs of tiles, the partials go to
// `workspace` (B * Hq * splits * 520 bytes) and a second small launch on the same stream merges them; with
// splits == 1 there is one launch and the workspace is not used (it may be NULL).  gsx_decode_attn picks the
// configuration and `splits` from B * Hkv and max_seq_len alone (attn_pick() in attn_decode.hip);
// gsx_decode_attn_workspace_bytes returns what it can need for these arguments with any legal Hkv.
enum { GSX_ATTN_KV_BF16 = 0, GSX_ATTN_KV_FP8 = 1 };
int gsx_decode_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                    const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D, int page,
                    int num_pages, int table_stride, int max_seq_len, float scale, float k_scale, float v_scale,
                    void* workspace, uint64_t workspace_bytes);
int gsx_decode_attn_workspace_bytes(int B, int Hq, int D, int page, int max_seq_len, uint64_t* bytes);
// The attention configurations, one table for both cache types: 0 "4w-f1", 1 "4w-f2", 2 "8w-f1", 3 "8w-f2": waves per
// workgroup - tiles of 32 tokens a wave keeps in flight.  _cfg_name returns NULL and _cfg_shape nonzero outside the
// table.  _launch_cfg takes 1 <= splits <= 64 and otherwise what gsx_decode_attn takes; a workspace that is too
// small for `splits` is refused with the bytes needed in the text.
const char* gsx_decode_attn_cfg_name(int cfg);
int gsx_decode_attn_cfg_shape(int cfg, int* waves, int* inflight);
int gsx_decode_attn_launch_cfg(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                               const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D,
                               int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                               float v_scale, void* workspace, uint64_t workspace_bytes, int cfg, int splits);
// elapsed milliseconds of `iters` back-to-back gsx_decode_attn on `stream`, by hip events (for benches)
int gsx_event_time_decode_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                               const void* block_table, const void* seq_lens, void* O, int B, int Hq, int Hkv, int D,
                               int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                               float v_scale, void* workspace, uint64_t workspace_bytes, int iters, float* ms);

// RoPE and KV-cache append (kv_append.hip): the producer of the caches gsx_decode_attn reads, same kinds and layout.
//   QKV[B * T][qkv_stride]                bf16, elements: row n is token n's Hq query heads, then Hkv key heads, then
//                                         Hkv value heads, D == 128 each (the fused projection's output)
//   Q_out[B * T][Hq][D]                   bf16, contiguous; with T == 1 the Q[B][Hq][D] of gsx_decode_attn
//   K_cache, V_cache [num_pages][Hkv][page][D]   bf16 (GSX_ATTN_KV_BF16) or OCP e4m3 (GSX_ATTN_KV_FP8)
//   block_table[B][table_stride], seq_lens[B]    int32, device memory, as gsx_decode_attn takes them
//   lens_out[B]                           int32, device memory, or NULL
//   rope_cos, rope_sin [rope_len][D / 2]  fp32, device memory
// Token n belongs to sequence b = n / T and is its new token t = n % T (T == 1: a decode step; larger: a prefill
// chunk).  base = clamp(seq_lens[b], 0, max_seq_len), the clamp the attention applies, and pos = base + t.  A token
// is LIVE when pos < max_seq_len and block_table[b][pos / page] lies in [0, num_pages).  A live token writes slot
// pos % page of that page for every KV head in both caches (64-bit offsets: a cache may exceed 4 GiB) and its
// rotated queries to Q_out.  Any other token writes nothing to the caches and zeros to its Q_out row: a bad page index
// is dropped, not clamped (a clamped write would land in another sequence's page), so no input makes the kernel write
// outside the caches, Q_out or lens_out.  lens_out[b] = min(base + T, max_seq_len), written by exactly one workgroup
// per sequence; it must not overlap seq_lens, which other workgroups are still reading.  Two sequences that share a
// page and write the same slot race: that is the caller's business.
// Numerics, bit for bit.  Half-split ("NeoX") pairing: (x1, x2) = (x[i], x[i + 64]), c = rope_cos[pos][i],
// s = rope_sin[pos][i], i < 64:
//   x1' = fl(fl(x1 * c) - fl(x2 * s))     x2' = fl(fl(x2 * c) + fl(x1 * s))
// every fp32 operation rounded on its own, nothing contracted into an FMA; the tables are whatever fp32 the caller
// supplies.  Q_out = bf16(x'), round to nearest even.  bf16 cache: K = bf16(x'), V a raw 16-bit copy, and k_inv_scale
// and v_inv_scale exactly 1.0f.  e4m3 cache: K = e4m3(fl(x' * k_inv_scale)), V = e4m3(fl(v * v_inv_scale)), round to
// nearest even onto OCP e4m3fn, saturating: every finite value beyond +-448, and +-inf, give +-448 (0x7e / 0xfe); a NaN
// gives a NaN code (0x7f or 0xff).  The inverse scales are finite and > 0; gsx_decode_attn's k_scale and v_scale are
// their reciprocals.  Intermediate magnitudes below 2^-100 that are not exact zeros are outside the contract.
// Requirements: a known kind; D == 128; Hq % Hkv == 0 and Hq / Hkv <= 16; page % 16 == 0 and 16 <= page <= 256;
// B, T >= 1 and B * T below 2^31; 1 <= max_seq_len <= table_stride * page; rope_len >= max_seq_len; qkv_stride >=
// (Hq + 2 Hkv) * D and qkv_stride % 8 == 0; every pointer but lens_out non-NULL; QKV, Q_out, the caches and the tables
// 16-B aligned, the int32 arrays 4-B aligned; Q_out does not overlap QKV.  Everything is validated before the first
// device call; launches on `stream` and returns without synchronising.
int gsx_kv_append(void* stream, int kind, const void* QKV, int64_t qkv_stride, void* Q_out, void* K_cache,
                  void* V_cache, const void* block_table, const void* seq_lens, void* lens_out, const float* rope_cos,
                  const float* rope_sin, int rope_len, int B, int T, int Hq, int Hkv, int D, int page, int num_pages,
                  int table_stride, int max_seq_len, float k_inv_scale, float v_inv_scale);
// elapsed milliseconds of `iters` back-to-back gsx_kv_append on `stream`, by hip events (for benches)
int gsx_event_time_kv_append(void* stream, int kind, const void* QKV, int64_t qkv_stride, void* Q_out, void* K_cache,
                             void* V_cache, const void* block_table, const void* seq_lens, void* lens_out,
                             const float* rope_cos, const float* rope_sin, int rope_len, int B, int T, int Hq, int Hkv,
                             int D, int page, int num_pages, int table_stride, int max_seq_len, float k_inv_scale,
                             float v_inv_scale, int iters, float* ms);

// Causal prefill attention over the paged KV cache (attn_prefill.hip): T new tokens per sequence attend over the cache
// that gsx_kv_append(T) has just extended; kinds, cache layout, block_table and seq_lens as gsx_decode_attn takes them.
//   Q[B * T][Hq][D], O[B * T][Hq][D]      bf16, D == 128; Q is exactly the Q_out of gsx_kv_append
//   seq_lens[B]                           the lengths BEFORE the chunk: the buffer gsx_kv_append took, not its lens_out
// base = clamp(seq_lens[b], 0, max_seq_len).  Row n = b * T + t is at pos = base + t and is LIVE when pos <
// max_seq_len, the rule of gsx_kv_append.  A live row attends to tokens 0 .. pos of its sequence (causal, its own token
// included); a row that is not live gives a row of zeros.  With T == 1 this is gsx_decode_attn on lengths base + 1.
// Requirements: a known kind; D == 128; 1 <= Hq <= 4096, Hq % Hkv == 0 and Hq / Hkv <= 16; page % 16 == 0 and 16 <=
// page <= 256; B, T >= 1, B * T below 2^31 and ceil(T / 256) * B * Hq below 2^31 (the grid); num_pages >= 1; 1 <=
// max_seq_len <= table_stride * page; every pointer non-NULL, Q, the caches and O 16-B aligned, the int32 arrays 4-B
// aligned; O does not overlap Q; scale, k_scale and v_scale finite and > 0, the latter two exactly 1.0f for a bf16
// cache.  Everything is validated before the first device call; launches on `stream` and returns without synchronising.
// Safety: a page index is clamped into [0, num_pages) by an unsigned min; block-table entries past the page of the
// last live row of a block of 256 query rows are never read by that block; offsets into the caches are 64-bit.  No
// content of block_table, seq_lens or the caches makes the kernel read outside the caches or write outside O.
// Numerics, the contract of gsx_decode_attn per query row, over the tokens j <= pos:
//   x[j] = (q . k_j) * (scale * k_scale * log2 e)        fp32; bf16 products accumulated in fp32 on
//                                                        v_mfma_f32_32x32x16_bf16; e4m3 K and V are converted to
//                                                        bf16 on the way into LDS, which is exact
//   p = exp2(x - m)                                      fp32, m a running maximum (plain online softmax: the
//                                                        accumulator is rescaled at every tile, nothing is deferred)
//   l = sum of p                                         fp32, of the unrounded p
//   P = bf16(p), round to nearest even                   the operand of the PV MFMA, accumulated in fp32
//   O = bf16((acc / l) * v_scale)                        rounded once
// One workgroup takes the sequence's KV tiles of 64 tokens front to back, from token 0: no split-KV, no workspace,
// nothing passes between workgroups, and the result is deterministic.  A row's bytes depend only on its own query,
// its pos and its sequence's cache: not on B, T, or which rows share the launch.  A token a row may not see has its x
// replaced by -inf by a select, so it contributes nothing whatever its K holds; V of tokens past the last live row
// of the row's block of 256 is replaced by zeros.  Between a row's pos and that last row (tokens the same launch's
// later rows do see) V must be finite: 0 * NaN in the PV product would reach the row.
int gsx_prefill_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                     const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv, int D,
                     int page, int num_pages, int table_stride, int max_seq_len, float scale, float k_scale,
                     float v_scale);
// The prefill configurations, one table for both cache types: 0 "8w-q256-k64": waves per workgroup - query rows per
// workgroup - tokens per KV tile.  _cfg_name returns NULL and _cfg_shape nonzero outside the table; _launch_cfg takes
// what gsx_prefill_attn takes.
const char* gsx_prefill_attn_cfg_name(int cfg);
int gsx_prefill_attn_cfg_shape(int cfg, int* q_rows, int* kv_tile, int* waves);
int gsx_prefill_attn_launch_cfg(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv,
                                int D, int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                float k_scale, float v_scale, int cfg);
// elapsed milliseconds of `iters` back-to-back gsx_prefill_attn on `stream`, by hip events (for benches)
int gsx_event_time_prefill_attn(void* stream, int kind, const void* Q, const void* K_cache, const void* V_cache,
                                const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq, int Hkv,
                                int D, int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                float k_scale, float v_scale, int iters, float* ms);

// Fused residual add + RMSNorm, and SwiGLU (norm_act.hip): what a decoder layer has between its projections.  Both
// write bf16, or OCP e4m3 with one fp32 scale per row, which is exactly the A and scale_a that
// gsx_decode_gemm_nt(GSX_DECODE_FP8, .., GSX_GEMM_SCALE_ROW) takes.  Strides are in elements of the row's type.
//   GSX_ACT_OUT_BF16      Y[M][y_stride] bf16 = bf16(y32), round to nearest even; scale_out NULL
//   GSX_ACT_OUT_FP8_ROW   Y[M][y_stride] bytes, OCP e4m3fn; scale_out[M] fp32, device memory, 4-B aligned.  Per row,
//                         amax = max |y32| over the unrounded fp32 values, scale_out[m] = fl(amax / 448) and
//                         Y = e4m3(fl(y32 * fl(448 / amax))), round to nearest even, saturating at +-448 (the
//                         conversion of gsx_kv_append): the row's largest element is 0x7e or 0xfe.  A row of zeros
//                         has scale 1.0f and every code 0x00.  The encoded value is within 3 * 2^-24 (relative) of
//                         y32 / scale_out[m]: two divisions and one multiplication.
// gsx_add_rmsnorm: X[M][x_stride] bf16 (a sublayer's output), W[H] bf16, R_in and R_out bf16 [M][r_stride] (the
// residual stream; either may be NULL; R_out == R_in updates it in place).  Per row:
//   h = bf16(fl(x + r))           round to nearest even; with R_in NULL h = x, a raw 16-bit copy
//   R_out = h                     if R_out is given
//   ss = sum of h^2               fp32; every square is exact
//   rinv = 1 / sqrt(ss / H + eps)
//   y32 = (h * rinv) * w          fp32
// The norm works on the rounded h.  A row whose ss / H + eps is 0 is outside the contract.
// gsx_silu_mul: row m of GU[M][gu_stride] (bf16) holds I gate values, then I up values (the fused gate / up
// projection's output); y32 = g / (1 + exp(-g)) * u.  The contract covers finite inputs with |g| <= 64; an exact
// result of nonzero magnitude below 2^-100 is outside it.  A non-finite g or u makes that element unspecified with
// GSX_ACT_OUT_BF16 and its whole row (scale included) with GSX_ACT_OUT_FP8_ROW; nothing is ever written outside Y and
// scale_out.
// Numerics: a bound, not bit-exactness (an FMA may stand for a multiply and an add).  y32 lies within a relative
// error delta of the exact value, u = 2^-24 per correctly rounded fp32 operation:
//   norm   delta = (n_chain + n_tree + 6) u.  The sum of squares adds a thread's 8 * ceil(H / 2048) squares in turn
//          (n_chain; at most 64) and combines 256 threads in a fixed tree of n_tree = 8 levels, so ss is off by at most
//          (n_chain + n_tree) u <= 72 u.  Then ss / H, + eps, sqrtf and 1 / x, each correctly rounded (the square
//          root halves what precedes it; the bound does not claim that), h * rinv and * w: 6 u.
//   silu   delta(g) = (4 + |g|) 2^-23.  t = fl(g * -log2 e) is off by 2 u |t| with the constant's own rounding, which
//          v_exp_f32 turns into |g| 2^-23 relative; v_exp_f32 itself 2^-23; 1 + e: u; v_rcp_f32: 2^-23; the two
//          multiplies: 2 u.  In all (|g| + 3.5) 2^-23.  The 2^-23 of v_exp_f32 and v_rcp_f32 is the ISA's documented
//          1 ulp.
// The result is deterministic and does not depend on M, on a row's index or on where workgroups run: nothing passes
// between workgroups.
// Requirements: a known out_kind; M >= 1; 8 <= H <= 16384 and H % 8 == 0; I >= 8, I % 8 == 0, and I <= 32768 with
// GSX_ACT_OUT_FP8_ROW (a workgroup holds a row); every stride at least its row (gu_stride >= 2 I) and a multiple of 8;
// X, W, GU and Y non-NULL; scale_out NULL exactly with GSX_ACT_OUT_BF16; X, R_in, R_out, W, GU and Y 16-B aligned (rows
// of e4m3 are then 8-B aligned); Y overlaps no input; R_out overlaps nothing but an R_in equal to it; scale_out
// overlaps nothing; eps finite and >= 0.  Row offsets are 64-bit: M * stride may exceed 2^31.  Everything is validated
// before the first device call; launches on `stream` and returns without synchronising.
enum { GSX_ACT_OUT_BF16 = 0, GSX_ACT_OUT_FP8_ROW = 1 };
int gsx_add_rmsnorm(void* stream, int out_kind, const void* X, int64_t x_stride, const void* R_in, void* R_out,
                    int64_t r_stride, const void* W, void* Y, int64_t y_stride, float* scale_out, int M, int H,
                    float eps);
int gsx_silu_mul(void* stream, int out_kind, const void* GU, int64_t gu_stride, void* Y, int64_t y_stride,
                 float* scale_out, int M, int I);
// elapsed milliseconds of `iters` back-to-back calls on `stream`, by hip events (for benches)
int gsx_event_time_add_rmsnorm(void* stream, int out_kind, const void* X, int64_t x_stride, const void* R_in,
                               void* R_out, int64_t r_stride, const void* W, void* Y, int64_t y_stride,
                               float* scale_out, int M, int H, float eps, int iters, float* ms);
int gsx_event_time_silu_mul(void* stream, int out_kind, const void* GU, int64_t gu_stride, void* Y, int64_t y_stride,
                            float* scale_out, int M, int I, int iters, float* ms);

// Token sampler and embedding gather (sample.hip): what closes a decode step.  The LM head is gsx_decode_gemm_nt with
// N = vocabulary; gsx_sample turns its bf16 logits into token ids and gsx_embed_gather turns token ids into the next
// step's input rows, both through device memory, so generation needs no host synchronisation.
// gsx_sample: logits[M][logits_stride] bf16; a stride of 0 makes every row read the same logits.  temperature[M]
// (fp32), top_k[M] (int32), top_p[M] (fp32) and seeds[M] (uint64) are per-row arrays in device memory;
// temperature == NULL makes every row greedy, top_k == NULL and top_p == NULL mean no limit, seeds may be NULL only
// when temperature is.  counter is the step number.  tokens_out[M] int32.  The result is exact: a NumPy twin
// (tests/sample_cases.py) reproduces every token.  No parameter value and no logit content makes the kernel write
// outside tokens_out[m] or write a value outside [0, V).  Per row:
//   key      a 16-bit integer that orders bf16 codes; -0 is +0; every NaN has one key, below -inf.  `first` is the
//            lowest index that holds the largest key.
//   greedy   the token is `first` when temperature[m] is NaN or <= 0, or the logit at `first` is not finite; top_k,
//            top_p and seeds are not read for such a row.
//   c        otherwise T = clamp(temperature, 2^-16, 2^16) and c = fl(fl32(log2 e) / T), one correctly rounded
//            fp32 division.
//   S        k = top_k (k <= 0 or k >= V: V); the k tokens of the largest keys, ties at the k-th key to the lowest
//            indices.
//   w        an integer.  d = fl(l - l_first), x = fl(d c); w = 0 when x < -32 and for a -inf or NaN logit.
//            Otherwise n = floor(x), f = fl(x - n), g = ((((c5 f + c4) f + c3) f + c2) f + c1) f + 1 with every
//            multiply and add rounded to fp32 on its own (no FMA), and w = trunc(g 2^(32 + n)) as a uint64.  `first`
//            has w = 2^32.  c1 = 0x1.62e4bcp-1, c2 = 0x1.ebdb30p-3, c3 = 0x1.c91e04p-5, c4 = 0x1.277576p-7,
//            c5 = 0x1.e97886p-10: g is within 2^-20 of 2^f on [0, 1).
//   N        p = top_p (NaN or p >= 1: no cut; p < 0: 0) and Z = sum of w over S.  S is walked by descending key,
//            every group of equal keys whole (of the group that top-k cuts, its members in S), up to and including
//            the first group at which (double)mass >= (double)p * (double)Z.  N holds `first`.
//   draw     a = mix64(seeds[m] + kGolden), r = mix64(a + (counter + 1) kGolden), wrapping (mix64.h);
//            target = the high 64 bits of r * Z_N, Z_N the sum of w over N.  The token is the lowest index of N whose
//            inclusive prefix sum of w, over N in index order, exceeds target.  A token of weight 0 is never drawn.
// Every sum is a sum of integers, so the result does not depend on the order of addition, on M, on a row's index or
// on where workgroups run; a workgroup owns a row and nothing passes between workgroups.
// gsx_embed_gather: out[m][0..H) is a raw 16-bit copy of table[tokens[m]][0..H); a token outside [0, V) gives a row
// of zeros (dropped, not clamped).  Nothing is written past element H of a row.
// Requirements: M >= 1.  gsx_sample: 8 <= V <= 262144 and V % 8 == 0; logits_stride 0, or >= V and a multiple of 8;
// logits and tokens_out non-NULL; logits 16-B aligned; temperature, top_k, top_p and tokens_out 4-B aligned, seeds
// 8-B aligned; tokens_out overlaps nothing.  gsx_embed_gather: V >= 1; H >= 8 and H % 8 == 0; each stride >= H and a
// multiple of 8; table, tokens and out non-NULL; table and out 16-B aligned, tokens 4-B aligned; out overlaps
// nothing.  Row offsets are 64-bit: the table may exceed 4 GiB.  Everything is validated before the first device
// call; launches on `stream` and returns without synchronising.
int gsx_sample(void* stream, const void* logits, int64_t logits_stride, const float* temperature,
               const int32_t* top_k, const float* top_p, const uint64_t* seeds, uint64_t counter,
               int32_t* tokens_out, int M, int V);
int gsx_embed_gather(void* stream, const void* table, int64_t table_stride, const int32_t* tokens, void* out,
                     int64_t out_stride, int M, int H, int V);
// elapsed milliseconds of `iters` back-to-back calls on `stream`, by hip events (for benches)
int gsx_event_time_sample(void* stream, const void* logits, int64_t logits_stride, const float* temperature,
                          const int32_t* top_k, const float* top_p, const uint64_t* seeds, uint64_t counter,
                          int32_t* tokens_out, int M, int V, int iters, float* ms);
int gsx_event_time_embed_gather(void* stream, const void* table, int64_t table_stride, const int32_t* tokens,
                                void* out, int64_t out_stride, int M, int H, int V, int iters, float* ms);

// Mixture-of-experts decode (moe.hip, gemm_decode.hip): a router that picks topk of E experts per token, a grouped
// GEMM that streams only the chosen experts' weights, and the weighted sum of a token's expert outputs.  Decode-sized:
// 1 <= M <= 16 tokens and 1 <= topk <= 8, so at most P = M topk <= GSX_MOE_MAX_PAIRS (token, expert) pairs; pair
// p = m topk + j is token m's j-th choice.  A token never picks an expert twice, so an expert has at most 16 rows: one
// MFMA fragment of the decode kernel.  Ids, weights and the plan are device memory, written by one kernel and read by
// the next: an MoE layer needs no host synchronisation.
//
// gsx_moe_route: logits[M][logits_stride] bf16, what gsx_decode_gemm_nt writes with N = E against the router matrix.
// topk_ids[M][topk] int32, topk_w[M][topk] fp32, plan[GSX_MOE_PLAN_INTS] int32.  One launch of one workgroup.  Per row:
//   selection  by the sampler's key (gsx_sample): the topk largest keys, ties to the lowest index; -0 is +0 and every
//              NaN has one key below -inf.
//   ids        topk_ids[m][j] in descending key order, the lowest index first among equal keys; j = 0 is `first`.
//   weights    a softmax over the selected logits only (Mixtral, gpt-oss, Qwen3 with norm_topk_prob).  With l0 the
//              logit at `first`: if l0 is not finite, w_0 = 1 and the others 0.  Otherwise
//              p_j = exp2(fl(fl(l_j - l0) * fl32(log2 e))), p_j = 0 for a -inf or NaN l_j, and
//              w_j = p_j / (p_0 + ... + p_{topk-1}), summed in the order of j.
// Selection, ids and plan are exact (tests/moe_cases.py is their twin).  The weights have a bound, not bit-exactness,
// as gsx_silu_mul: with x_j = l_j - l0 <= 0 and u = 2^-24 per correctly rounded fp32 operation, w_j lies within a
// relative delta(x_j) = (3 |x_j| + 3.2 (topk - 1) + 4) u of the exact softmax weight wherever that is >= 2^-100, and
// within 2^-99 absolute below.  Operation by operation:
//   p_j    d = fl(l_j - l0): u.  fl32(log2 e) is within u of log2 e, and the multiply adds u: the argument t of the
//          exponential is off by 3 u |t|, |t| = |x_j| log2 e, which 2^t turns into 3 u |x_j| ln 2 log2 e = 3 |x_j| u
//          relative.  v_exp_f32: the ISA's documented 1 ulp, 2 u.  In all (3 |x_j| + 2) u; p_0 = 2^0 = 1 is exact, and
//          so is every p_j with l_j = l0.
//   sum    the exact sum of the computed p is off by sum_j p_j delta_j / sum_j p_j.  p_j <= e^x_j (1 + delta_j) and
//          e^-|x| (3 |x| + 2) <= 2.15 (at |x| = 1 / 3), the sum is >= p_0 = 1, and p_0 carries no error: at most
//          2.2 (topk - 1) u.  Its topk - 1 additions of positive terms: (topk - 1) u.  Together 3.2 (topk - 1) u.
//   w_j    the division: u.  One more u covers the second-order terms of the products above.
// A weight that these rules make exactly 0 or 1 is exactly that (topk = 1; a -inf or NaN logit; a non-finite l0).
// The plan: a header {n_active, P, E, 0}, then slot_expert, slot_begin, slot_count and rows, GSX_MOE_MAX_PAIRS int32
// each.  Slots 0 .. n_active - 1 are the experts that have at least one pair, in ascending expert index;
// rows[slot_begin[s] .. + slot_count[s]) are that expert's pairs in ascending order, and the slots' runs tile
// rows[0, P) in slot order.  Every unused slot is {-1, 0, 0} and every unused row -1: the whole buffer is defined, the
// same size for every M.  No logit content makes the kernel write outside its three outputs, and every id it writes
// lies in [0, E).
// Requirements: 1 <= M <= 16; 8 <= E <= 1024 and E % 8 == 0; 1 <= topk <= min(8, E); logits_stride >= E and a
// multiple of 8; every pointer non-NULL, logits 16-B aligned, the others 4-B aligned; the outputs overlap nothing.
//
// gsx_moe_gemm_nt: for every pair p of the plan, with e its slot's expert, C[p][0..N) = A[p / a_div][0..K) *
// B[e][N][K]^T.  a_div = topk is the up projection (a pair reads its token's row of xn[M][K]), a_div = 1 the down
// projection (a pair reads its own row of act[P][K]).  A has ceil(P / a_div) contiguous rows, C[P][N] is bf16 and
// contiguous, B[E][N][K] are the experts' matrices back to back.  `kind` and the operand formats are those of
// gsx_decode_gemm_nt.  GSX_DECODE_FP8 takes GSX_GEMM_SCALE_NONE, or GSX_GEMM_SCALE_ROW with scale_a one fp32 per row
// of A (what GSX_ACT_OUT_FP8_ROW writes) and scale_b[E][N]; GSX_DECODE_MXFP4 takes scale_a[rows of A][K / 32] and
// scale_b[E][N][K / 32].  The kernel is decode_kernel's body: workgroup (strip, slot), grid.y = min(E, P); a workgroup
// whose slot is not active returns at once, so the host never learns n_active.  The summation order of a (row,
// column) is that of the decode configuration of the same shape, so a pair's row of C has the bits that
// gsx_decode_gemm_nt_launch_cfg gives for that row against that expert.  Inactive experts' weights are never read.
// The plan is device memory anyone may have written, and no content of it makes the kernel read outside A, B or the
// scales or write outside C: a slot whose expert is outside [0, E) is skipped, slot_count is clamped to [0, 16], an
// index into rows outside [0, GSX_MOE_MAX_PAIRS) and a pair outside [0, P) are dropped (no load, no store).  The
// same pair listed twice is a race between equal or unequal values: the caller's business.
// Requirements: 1 <= M <= 16; E >= 1; 1 <= topk <= min(8, E); a_div >= 1; the K multiples of gsx_decode_gemm_nt and
// N % 16 == 0; A, B, C and plan non-NULL, A, B and C 16-B aligned, plan 4-B aligned; the scales as above; A's rows and
// one row more (where a lane without a pair points) fit a 32-bit buffer range, which is refused otherwise: there is no
// masked form; C overlaps nothing.  Offsets into B, scale_b and C are 64-bit: B may exceed 4 GiB.
// The configurations are a table of its own, the four shapes gsx_decode_gemm_nt dispatches to: 0 "16/4w-f4",
// 1 "16/8w-f4", 2 "16/16w-f4", 3 "32/8w-f4"; _cfg_shape also gives the decode configuration each equals.
// gsx_moe_gemm_nt picks by the decode GEMM's rule on (N, K).
//
// gsx_moe_combine: Y[P][y_stride] bf16 (the down projection's C), out[M][out_stride] bf16.  out[m][h] = bf16(acc),
// acc = fl(w_0 y_0), then acc = fl(acc + fl(w_j y_j)) for j = 1 .. topk - 1, with y_j = Y[m topk + j][h] and
// w_j = topk_w[m][j]: every fp32 operation rounded on its own, nothing contracted, one rounding to bf16.  Bit-exact
// and fixed in order.  Requirements: 1 <= M <= 16; 1 <= topk <= 8; H >= 8 and H % 8 == 0; each stride >= H and a
// multiple of 8; pointers non-NULL, Y and out 16-B aligned, topk_w 4-B aligned; out overlaps nothing.
// Everything is validated before the first device call; every launch is on `stream` and returns without synchronising.
#define GSX_MOE_MAX_PAIRS 128
#define GSX_MOE_PLAN_INTS (4 + 4 * GSX_MOE_MAX_PAIRS)  // 516
int gsx_moe_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids, float* topk_w,
                  int32_t* plan, int M, int E, int topk);
int gsx_moe_gemm_nt(void* stream, int kind, const void* A, int a_div, const void* B, void* C, const int32_t* plan,
                    int M, int topk, int E, int N, int K, const void* scale_a, const void* scale_b, int scale_mode);
const char* gsx_moe_gemm_cfg_name(int cfg);
int gsx_moe_gemm_cfg_shape(int cfg, int* bn, int* waves, int* inflight, int* decode_cfg);
int gsx_moe_gemm_nt_launch_cfg(void* stream, int kind, const void* A, int a_div, const void* B, void* C,
                               const int32_t* plan, int M, int topk, int E, int N, int K, const void* scale_a,
                               const void* scale_b, int scale_mode, int cfg);
int gsx_moe_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out, int64_t out_stride,
                    int M, int topk, int H);
// elapsed milliseconds of `iters` back-to-back calls on `stream`, by hip events (for benches)
int gsx_event_time_moe_route(void* stream, const void* logits, int64_t logits_stride, int32_t* topk_ids, float* topk_w,
                             int32_t* plan, int M, int E, int topk, int iters, float* ms);
int gsx_event_time_moe_gemm(void* stream, int kind, const void* A, int a_div, const void* B, void* C,
                            const int32_t* plan, int M, int topk, int E, int N, int K, const void* scale_a,
                            const void* scale_b, int scale_mode, int iters, float* ms);
int gsx_event_time_moe_combine(void* stream, const void* Y, int64_t y_stride, const float* topk_w, void* out,
                               int64_t out_stride, int M, int topk, int H, int iters, float* ms);

// HBM pre-flight memory test (memtest.hip).  The expected content of 16-byte word W = origin/16 + word index is
// generated from (pattern, seed, invert, W) and never stored; `origin` is the byte offset of `base` in the whole
// tested range, so a range tested chunk by chunk keeps globally unique content.
//   ADDR    dwords {lo32(W), hi32(W), ~lo32(W), ~hi32(W)}
//   SOLID   every dword = seed
//   WALK    dword j = 1u << ((4*W + j + seed) & 31)
//   RANDOM  two 64-bit outputs of a counter-based mixer (splitmix64's output function) of 2*W + half and seed
// invert != 0 complements all four dwords.  bytes and origin are multiples of 16; base is 16-B aligned.
enum { GSX_MEMTEST_ADDR = 0, GSX_MEMTEST_SOLID = 1, GSX_MEMTEST_WALK = 2, GSX_MEMTEST_RANDOM = 3 };
enum { GSX_MEMTEST_QUICK = 0, GSX_MEMTEST_FULL = 1 };
typedef struct {
  uint64_t offset;  // origin + byte offset of the dword
  uint32_t expected, actual;
} gsx_memtest_err;
#define GSX_MEMTEST_MAX_ERRS 32
typedef struct {
  uint64_t bad_dwords;  // exact count
  uint32_t flipped_or;  // OR of expected ^ actual over all bad dwords
  uint32_t n_errs;      // min(bad_dwords, MAX_ERRS)
  gsx_memtest_err errs[GSX_MEMTEST_MAX_ERRS];
} gsx_memtest_report;
// One launch on `stream`, not synchronised.
int gsx_memtest_write(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert);
// Compares every dword and ACCUMULATES into *report (the caller zeroes it); one stream sync.  rewrite != 0 also
// stores the complement of the expected word in the same pass (moving inversions: a bad word is overwritten
// with correct data).  The per-launch counters live in pinned host memory, as gsx_hbm_admit_n's do.
int gsx_memtest_check(void* stream, void* base, uint64_t bytes, uint64_t origin, int pattern, uint32_t seed,
                      int invert, int rewrite, gsx_memtest_report* report);
// The fixed pass sequence of a level, each a triple {write, check + rewrite, check inverted}: QUICK runs ADDR and
// RANDOM (8 x bytes of traffic); FULL adds SOLID with seeds 0, ~0, 0x55555555, 0xAAAAAAAA and WALK with seeds 0..31.
int gsx_memtest_run(void* stream, void* base, uint64_t bytes, uint64_t origin, int level, gsx_memtest_report* report,
                    uint32_t* passes_out, double* seconds_out);
// Pass `idx` of a level's sequence (what gsx_memtest_run and gsx-memtest execute): 0, or 1 past the last pass.
typedef struct {
  int pattern;
  uint32_t seed;
  int invert, rewrite, write;  // write != 0: a write pass; otherwise a check, with or without rewrite
} gsx_memtest_pass_t;
int gsx_memtest_pass(int level, uint32_t idx, gsx_memtest_pass_t* out);

// Compute pre-flight (cutest.hip): a known-answer test of every CU's matrix cores, vector ALU and LDS.  One launch
// runs workgroups of 4 waves that each take a CU's whole LDS (one workgroup per CU at a time); every wave reads
// its HW_ID / XCC_ID, runs the units below from `seed` and writes one record.  A unit ends in one 64-bit
// signature, the same for every healthy wave of a launch; NumPy twin in ops/cutest.py.
//   MFMA_*    R chained matrix instructions on integer operands that are a function of (seed, unit, round, matrix
//             coordinates); every result is an exact integer whatever the summation order
//   VALU_F32  MFMA_F32's product by v_fma_f32: the same signature
//   VALU_INT  a per-lane chain of 32-bit multiplies (low and high), 64-bit multiply-adds, rotates, xor, popcount
//             and compare-selects
//   LDS       two passes (the RANDOM words of the memory test, then their complement) over the workgroup's whole
//             LDS: every wave fills a quarter and checks the quarter another wave wrote, half of it with b128
//             and half with b32 reads
enum {
  GSX_CUTEST_MFMA_BF16_16 = 0,
  GSX_CUTEST_MFMA_BF16_32 = 1,
  GSX_CUTEST_MFMA_F16 = 2,
  GSX_CUTEST_MFMA_FP8 = 3,
  GSX_CUTEST_MFMA_I8 = 4,
  GSX_CUTEST_MFMA_F32 = 5,
  GSX_CUTEST_VALU_F32 = 6,
  GSX_CUTEST_VALU_INT = 7,
  GSX_CUTEST_LDS = 8,
  GSX_CUTEST_UNITS = 9
};
enum { GSX_CUTEST_QUICK = 0, GSX_CUTEST_FULL = 1 };
#define GSX_CUTEST_MAX_BAD 16      // bad-CU entries a report lists; its counts stay exact beyond
#define GSX_CUTEST_CU_SLOTS 4096   // a physical CU's slot: xcc << 8 | se << 5 | sh << 4 | cu
#define GSX_CUTEST_MAX_BLOCKS 8192
const char* gsx_cutest_unit_name(int unit);  // NULL outside the table
// The matrix units' table: a chain of `rounds` M x N x K products of integers in [-span/2, span/2 - 1].  Nonzero
// for a unit that is no matrix unit.
int gsx_cutest_unit_shape(int unit, int* m, int* n, int* k, int* rounds, int* span);
// Launches of a level (seeds 0 .. n - 1): QUICK 8, FULL 256; 0 for an unknown level.
uint32_t gsx_cutest_seeds(int level);
typedef struct {
  uint32_t hw_id, xcc_id;  // HW_REG_HW_ID and HW_REG_XCC_ID of the wave, as the CU probe records them
  uint32_t fail_mask;      // bit u: sig[u] is not the expected signature
  uint32_t seed;
  uint64_t sig[GSX_CUTEST_UNITS];
} gsx_cutest_record;
// For tests: a wave whose HW_ID fields match (simd < 0: any SIMD of the CU) XORs xor_mask into the raw 32 bits of
// result element (0, 0) of `unit` before the fold (VALU_INT: lane 0's 32-bit state; LDS: dword 0 of the quarter
// it read).  xor_mask == 0: off.  One value changes; nothing else does.
typedef struct {
  int32_t xcc, se, sh, cu, simd, unit;
  uint32_t xor_mask;
} gsx_cutest_inject;
typedef struct {
  uint32_t waves, bad_waves;
  uint16_t fail_mask;        // OR over the CU's waves
  uint8_t simds, bad_simds;  // 4-bit sets: the SIMDs that ran a wave / a bad wave
} gsx_cutest_cu;
typedef struct {
  uint8_t xcc, se, sh, cu;
  uint8_t simds;  // the SIMDs with a bad wave
  uint8_t unit;   // the first bad unit of the CU's first bad wave, with its seed and signatures
  uint16_t units;
  uint32_t seed;
  uint64_t expected, got;
} gsx_cutest_bad;
typedef struct {
  uint64_t waves, bad_waves;
  uint32_t cus_seen, simds_seen;  // CUs / (CU, SIMD) pairs that ran a wave
  uint32_t cus_covered;           // CUs all four of whose SIMDs ran a wave
  uint32_t bad_cus, n_bad;        // exact count; min(bad_cus, MAX_BAD) entries in bad[]
  uint32_t launches, cus_expected, covered;  // set by gsx_cutest_run
  gsx_cutest_bad bad[GSX_CUTEST_MAX_BAD];
  gsx_cutest_cu cu[GSX_CUTEST_CU_SLOTS];
} gsx_cutest_report;
// The host-side twin, in plain integer arithmetic: no device call.
int gsx_cutest_expected(int unit, uint32_t seed, uint64_t* sig);
// One launch of `blocks` workgroups and one stream sync; records_out[0, 4 * blocks) are the waves' records
// (n >= 4 * blocks).  inject may be NULL.
int gsx_cutest_launch(void* stream, uint32_t seed, int blocks, const gsx_cutest_inject* inject,
                      gsx_cutest_record* records_out, uint32_t n);
// Pure host code: ACCUMULATES n records into *report (the caller zeroes a new one).
int gsx_cutest_aggregate(const gsx_cutest_record* records, uint32_t n, gsx_cutest_report* report);
// A level's launches (4 workgroups per expected CU), accumulated into *report (the caller zeroes it).  While
// fewer than expect_cus CUs are covered, up to GSX_CUTEST_EXTRA_LAUNCHES more follow; coverage that stays short
// clears report->covered and is no error.  expect_cus == 0: the popcount of the stream's CU mask, or the device's
// CU count when the stream has none.
#define GSX_CUTEST_EXTRA_LAUNCHES 8
int gsx_cutest_run(void* stream, int level, uint32_t expect_cus, gsx_cutest_report* report, double* seconds_out);
// What expect_cus == 0 stands for on `stream`.
int gsx_cutest_stream_cus(void* stream, uint32_t* cus);

#ifdef __cplusplus
}
#endif
