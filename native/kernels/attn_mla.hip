// Multi-head latent attention (MLA) decode over a paged latent cache: the attention of DeepSeek-V2/V3/R1 and Kimi K2
// in its absorbed form.  One new token per sequence; every token of the cache is ONE row of 576 elements, 512 latent
// plus 64 rotated RoPE elements, shared by all 1 .. 128 query heads: all 576 are K, the first 512 are V as well.  C ABI
// and numeric contract in gsx_kernels.h.
//
// The kernel, the merge, the validation and the launcher are in attn_mla.h, shared with the multi-token form
// (attn_mla_multi.hip).  Here a sequence's columns are its heads: Hq <= 64 is one block of ceil(Hq / 16) fragments, more
// heads are two blocks of NF = ceil(Hq / 32) fragments each, and every column's limit is seq_len.  This file holds the
// configuration table, the dispatch rule and the entry points.
#include "attn_mla.h"

namespace gsxgemm {
namespace {

// name: waves per workgroup - tiles of 32 tokens a workgroup keeps in flight in registers
constexpr MlaCfg kMlaCfgs[] = {
    ml_cfg<1, false>("4w-f1"),
    ml_cfg<2, false>("4w-f2"),
};
constexpr int kNumMlaCfgs = sizeof(kMlaCfgs) / sizeof(kMlaCfgs[0]);

const MlaCfg* ml_row(int cfg) { return cfg >= 0 && cfg < kNumMlaCfgs ? &kMlaCfgs[cfg] : nullptr; }

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
  const int64_t items = static_cast<int64_t>(B) * ml_col_blocks(Hq);
  const int workgroups = ml_frags(Hq) <= 2 ? 512 : 256;
  *cfg = 0;
  int64_t want = (workgroups + items - 1) / items;
  const int most = tiles / 8;
  if (want > most) want = most;
  if (want > AT_MAX_SPLITS) want = AT_MAX_SPLITS;
  *splits = want < 1 ? 1 : static_cast<int>(want);
}

MlaArgs ml_args1(int kind, const void* Q, const void* KV, const void* block_table, const void* seq_lens, void* O, int B,
                 int Hq, int page, int num_pages, int table_stride, int max_seq_len, float scale, float kv_scale,
                 void* workspace, uint64_t workspace_bytes) {
  return ml_args(kind, Q, KV, block_table, seq_lens, O, B, 1, Hq, page, num_pages, table_stride, max_seq_len, scale,
                 kv_scale, workspace, workspace_bytes);
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
  if (int rc = ml_validate_shape("gsx_mla_decode_attn_workspace_bytes", B, 1, Hq, page, max_seq_len)) return rc;
  int cfg = 0, splits = 1;
  mla_pick(B, Hq, max_seq_len, &cfg, &splits);
  *bytes = ml_ws_bytes(static_cast<uint64_t>(B) * Hq, splits);
  return 0;
}

int gsx_mla_decode_attn_launch_cfg(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                                   const void* seq_lens, void* O, int B, int Hq, int page, int num_pages,
                                   int table_stride, int max_seq_len, float scale, float kv_scale, void* workspace,
                                   uint64_t workspace_bytes, int cfg, int splits) {
  const char* who = "gsx_mla_decode_attn_launch_cfg";
  const MlaCfg* c = ml_row(cfg);
  if (!c) return fail_arg("gsx_mla_decode_attn_launch_cfg: unknown config");
  const MlaArgs a = ml_args1(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                             max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  if (int rc = ml_validate(who, a, splits)) return rc;
  return ml_run(*c, who, S(stream), a, splits);
}

int gsx_mla_decode_attn(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                        const void* seq_lens, void* O, int B, int Hq, int page, int num_pages, int table_stride,
                        int max_seq_len, float scale, float kv_scale, void* workspace, uint64_t workspace_bytes) {
  const MlaArgs a = ml_args1(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                             max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  return ml_dispatch("gsx_mla_decode_attn", stream, a);
}

int gsx_event_time_mla_decode_attn(void* stream, int kind, const void* Q, const void* KV_cache, const void* block_table,
                                   const void* seq_lens, void* O, int B, int Hq, int page, int num_pages,
                                   int table_stride, int max_seq_len, float scale, float kv_scale, void* workspace,
                                   uint64_t workspace_bytes, int iters, float* ms) {
  const MlaArgs a = ml_args1(kind, Q, KV_cache, block_table, seq_lens, O, B, Hq, page, num_pages, table_stride,
                             max_seq_len, scale, kv_scale, workspace, workspace_bytes);
  // refused before the events are made, under the name of the entry point that is timed
  int cfg = 0, splits = 1;
  if (int rc = ml_plan("gsx_mla_decode_attn", a, &cfg, &splits)) return rc;
  return event_time(stream, iters, ms, [&] { return ml_dispatch("gsx_mla_decode_attn", stream, a); });
}

}  // extern "C"
