// Multi-token MLA decode attention over the paged latent cache: T = 1 .. 16 new tokens per sequence (the verify step
// of speculative decoding with a multi-token-prediction head, a short chunked-prefill tail), causal among themselves,
// in one pass over the cache.  C ABI and numeric contract in gsx_kernels.h.
//
// The kernel is mla_kernel of attn_mla.h with MULTI: Q[B * T][Hq][576] makes a sequence's C = T * Hq (token, head)
// pairs C contiguous rows, which are dealt to ceil(C / 64) column blocks of NF = ceil(C / (16 blocks)) fragments, up to 32
// blocks at T = 16, Hq = 128.  A workgroup of four waves owns one (sequence, column block, split); it stages every tile
// of 32 tokens once for all of its columns, with the three barriers and the ring of attn_mla.hip, and masks every
// column against a limit of its own, base + c / Hq + 1 (0 for a row that is not live), by a select.  Four new tokens of
// a 16-head shard are exactly the 64 columns of one block: one staging of the tile serves them all.  The cuts of the
// splits are counted up to the sequence's end, min(base + T, max_seq_len), and do not depend on the column block, so
// the result depends on `splits` alone; T == 1 runs the grid, the tiles and the arithmetic of gsx_mla_decode_attn on
// lengths one larger.  A block runs all tiles up to the sequence's end: the at most 15 tokens past its own largest
// limit rarely fill a tile, and none is skipped.
// LDS, registers: profiles/attn_mla_multi/README.md.  No scratch, no atomics.
#include "attn_mla.h"

namespace gsxgemm {
namespace {

// name: waves per workgroup - tiles of 32 tokens a workgroup keeps in flight in registers
constexpr MlaCfg kMlmCfgs[] = {
    ml_cfg<1, true>("4w-f1"),
    ml_cfg<2, true>("4w-f2"),
};
constexpr int kNumMlmCfgs = sizeof(kMlmCfgs) / sizeof(kMlmCfgs[0]);

const MlaCfg* mlm_row(int cfg) { return cfg >= 0 && cfg < kNumMlmCfgs ? &kMlmCfgs[cfg] : nullptr; }

// The dispatch rule, from B, T * Hq and max_seq_len alone: mla_pick()'s rule (attn_mla.hip) with B * column blocks
// work items:
//   configuration "4w-f1";
//   splits = ceil(W / (B * column blocks)) with W = 512 workgroups at one fragment and 256, one for each CU, above; but
//   no more than leave every split 8 tiles (max_seq_len / 256), and at most 64.
// Measured on one MI355X under the protocol of mla_pick()'s table (a ring of per-layer latent caches of more than 1
// GiB, pages of 16 tokens in random order), microseconds per launch by splits for "4w-f1"; `gsx` is the dispatched call and
// `single` T back-to-back gsx_mla_decode_attn on the same caches and base lengths, the yardstick
// (profiles/attn_mla_multi/README.md has "4w-f2" and the spreads):
//                        Hq   T  splits: 1       2       4       8      16      32      64    gsx    single
//   bf16  B 1  x 32768    16   2                                   161.41   93.83   68.94    68.96    110.53
//   bf16  B 1  x 32768    16   4                                   277.07  154.53  102.03   102.27    222.01
//   bf16  B 1  x 32768    16   8                           529.63  277.31  156.23  103.85   103.38    443.04
//   bf16  B 1  x 32768   128   2                  1041.14  530.93  279.05  156.92  105.87   104.57    207.64
//   bf16  B 1  x 32768   128   4          2065.66 1042.11  534.08  280.86  161.35  184.87    159.8    414.79
//   bf16  B 1  x 32768   128   8  4124.38 2063.69 1044.29  533.42  283.72  302.23  343.58   282.42    832.98
//   bf16  B 8  x 8192     16   2           302.73  158.72   87.21   53.95   43.19            42.95     67.74
//   bf16  B 8  x 8192     16   4           529.17  274.57  148.65   89.08   65.08            64.45    134.37
//   bf16  B 8  x 8192     16   8  1048.41  532.16  275.87  151.24   93.33   112.6            91.22     267.1
//   bf16  B 8  x 8192    128   2  1049.12   534.7  279.59  158.02  174.77  213.75           156.06    184.45
//   bf16  B 8  x 8192    128   4  1050.35   538.2  287.76  304.33   340.5  484.02           285.56    368.73
//   bf16  B 8  x 8192    128   8  1051.14   548.8  564.38   603.0   746.3  970.34            547.3    737.33
//   bf16  B 64 x 2048     16   2    157.9   88.72   57.89   70.42                            57.16     81.54
//   bf16  B 64 x 2048     16   4   276.51  154.31   95.62  114.86                            93.92    156.53
//   bf16  B 64 x 2048     16   8   280.48  167.45   183.6  229.53                           164.16    305.11
//   bf16  B 64 x 2048    128   2   284.82  320.08  373.57  511.74                           284.06    327.62
//   bf16  B 64 x 2048    128   4   566.74  648.91  775.93 1020.63                           566.74    660.53
//   bf16  B 64 x 2048    128   8  1133.24 1321.91 1547.15                                   1134.2   1325.64
//   fp8   B 1  x 32768    16   2                                   155.85   90.36    66.5    66.51    107.33
//   fp8   B 1  x 32768    16   4                                   248.86  139.94   94.77    94.84    215.26
//   fp8   B 1  x 32768    16   8                           477.85  250.57  142.15   96.92    96.87    429.69
//   fp8   B 1  x 32768   128   2                   941.27   480.2  252.85  143.97   98.59     98.6    188.19
//   fp8   B 1  x 32768   128   4          1864.98  946.25  484.32  256.07  148.29  172.15   147.64     376.6
//   fp8   B 1  x 32768   128   8  3721.32 1873.84  949.52  487.23  259.46  278.16  317.55   258.65    757.81
//   fp8   B 8  x 8192     16   2           296.61  155.11   85.13   52.59   41.74            41.41     64.66
//   fp8   B 8  x 8192     16   4           477.86   249.0  135.57   81.92   60.81            60.45    128.79
//   fp8   B 8  x 8192     16   8   945.83  481.36  250.08  138.01   85.72  105.24            84.85    257.24
//   fp8   B 8  x 8192    128   2   947.88  484.19  254.59   143.9  161.55  199.94           142.89    164.17
//   fp8   B 8  x 8192    128   4   949.52  489.26  261.66  278.63   314.7  455.81           260.98    328.85
//   fp8   B 8  x 8192    128   8   952.84  498.27  513.99  550.14  690.69  920.76           497.34    657.18
//   fp8   B 64 x 2048     16   2   153.96   86.78    55.0    65.3                            54.52     63.98
//   fp8   B 64 x 2048     16   4   251.41  141.22   87.89   105.9                            86.76    126.08
//   fp8   B 64 x 2048     16   8   253.51  152.21  167.63  205.44                           150.19    249.76
//   fp8   B 64 x 2048    128   2   257.83   292.7  332.06  484.18                           257.64    288.13
//   fp8   B 64 x 2048    128   4   511.77   584.8  724.97  970.92                           510.82     572.9
//   fp8   B 64 x 2048    128   8  1018.78 1219.45 1443.82                                   1019.1   1157.55
// Decided by the rows B 64 x 2048, 16 heads, T 2 (32 columns, two fragments): 4 splits, 256 workgroups, are 17 % (bf16)
// and 15 % (e4m3) ahead of the 8 splits that mla_pick()'s W = 512 at two fragments gives, and with 8 the e4m3 row lost
// to `single` (65.3 against 64.3 us); so W = 512 stays for one fragment only.  With that the rule's cell is the best
// measured cell, or within the row's spread of it, in every row, and `gsx` is ahead of `single` in all 36: 1.17 to 4.4 times at 16
// heads, 1.9 to 2.95 times for one sequence at 128 heads, and 1.12 to 1.35 times at 128 heads with 8 and 64 sequences,
// where a block of 64 columns is what a single-token launch already runs and the gain is launches and merges only.
// "4w-f2" is 1 to 14 % behind "4w-f1" in every cell.  NOT MEASURED: one fragment (T * Hq <= 16: W = 512 is
// mla_pick()'s, measured there at T = 1), three fragments (T * Hq of 33 to 48 and what the even deal of more blocks
// makes of other counts), T above 8, head counts other than 16 and 128, and more than 64 sequences.
void mlm_pick(int B, int C, int max_seq_len, int* cfg, int* splits) {
  const int tiles = (max_seq_len - 1) / AT_TILE + 1;
  const int64_t items = static_cast<int64_t>(B) * ml_col_blocks(C);
  const int workgroups = ml_frags(C) <= 1 ? 512 : 256;
  *cfg = 0;
  int64_t want = (workgroups + items - 1) / items;
  const int most = tiles / 8;
  if (want > most) want = most;
  if (want > AT_MAX_SPLITS) want = AT_MAX_SPLITS;
  *splits = want < 1 ? 1 : static_cast<int>(want);
}

// What the dispatching entry point will run, or why it refuses: no device call.
int mlm_plan(const char* who, const MlaArgs& a, int* cfg, int* splits) {
  if (int rc = ml_validate(who, a, 1)) return rc;  // everything but the workspace
  mlm_pick(a.B, ml_cols(a), a.max_seq_len, cfg, splits);
  return ml_validate(who, a, *splits);
}

int mlm_dispatch(const char* who, void* stream, const MlaArgs& a) {
  int cfg = 0, splits = 1;
  if (int rc = mlm_plan(who, a, &cfg, &splits)) return rc;
  return ml_run(kMlmCfgs[cfg], who, S(stream), a, splits);
}

}  // namespace
}  // namespace gsxgemm

using namespace gsxgemm;

extern "C" {

const char* gsx_mla_decode_attn_multi_cfg_name(int cfg) { return mlm_row(cfg) ? mlm_row(cfg)->name : nullptr; }

int gsx_mla_decode_attn_multi_cfg_shape(int cfg, int* waves, int* inflight) {
  const MlaCfg* c = mlm_row(cfg);
  if (!c) return -1;
  *waves = c->waves;
  *inflight = c->inflight;
  return 0;
}

int gsx_mla_decode_attn_multi_workspace_bytes(int B, int T, int Hq, int page, int max_seq_len, uint64_t* bytes) {
  if (!bytes) return fail_arg("gsx_mla_decode_attn_multi_workspace_bytes: bytes must not be NULL");
  if (int rc = ml_validate_shape("gsx_mla_decode_attn_multi_workspace_bytes", B, T, Hq, page, max_seq_len)) return rc;
  int cfg = 0, splits = 1;
  mlm_pick(B, T * Hq, max_seq_len, &cfg, &splits);
  *bytes = ml_ws_bytes(static_cast<uint64_t>(B) * T * Hq, splits);
  return 0;
}

int gsx_mla_decode_attn_multi_launch_cfg(void* stream, int kind, const void* Q, const void* KV_cache,
                                         const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq,
                                         int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                         float kv_scale, void* workspace, uint64_t workspace_bytes, int cfg,
                                         int splits) {
  const char* who = "gsx_mla_decode_attn_multi_launch_cfg";
  const MlaCfg* c = mlm_row(cfg);
  if (!c) return fail_arg("gsx_mla_decode_attn_multi_launch_cfg: unknown config");
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, T, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  if (int rc = ml_validate(who, a, splits)) return rc;
  return ml_run(*c, who, S(stream), a, splits);
}

int gsx_mla_decode_attn_multi(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                              const void* seq_lens, void* O, int B, int T, int Hq, int page, int num_pages,
                              int table_stride, int max_seq_len, float scale, float kv_scale, void* workspace,
                              uint64_t workspace_bytes) {
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, T, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  return mlm_dispatch("gsx_mla_decode_attn_multi", stream, a);
}

int gsx_event_time_mla_decode_attn_multi(void* stream, int kind, const void* Q, const void* KV_cache,
                                         const void* block_table, const void* seq_lens, void* O, int B, int T, int Hq,
                                         int page, int num_pages, int table_stride, int max_seq_len, float scale,
                                         float kv_scale, void* workspace, uint64_t workspace_bytes, int iters,
                                         float* ms) {
  const MlaArgs a = ml_args(kind, Q, KV_cache, block_table, seq_lens, O, B, T, Hq, page, num_pages, table_stride,
                            max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  // refused before the events are made, under the name of the entry point that is timed
  int cfg = 0, splits = 1;
  if (int rc = mlm_plan("gsx_mla_decode_attn_multi", a, &cfg, &splits)) return rc;
  return event_time(stream, iters, ms, [&] { return mlm_dispatch("gsx_mla_decode_attn_multi", stream, a); });
}

}  // extern "C"
