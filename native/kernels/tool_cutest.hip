// gsx-cutest: the compute pre-flight as an operator tool (kernel: cutest.hip).
//
//   gsx-cutest [--device N | --bdf DDDD:BB:DD.F] [--level quick|full] [--cu-mask W0,W1,...]
//              [--expect-cus N] [--max-seconds S] [--inject XCC:SE:SH:CU[:SIMD]:UNIT:XORMASK]
//
// Runs the level's launches (gsx_cutest_seeds; 4 workgroups per expected CU, each taking a CU's whole LDS) on the
// device, or on a stream restricted to --cu-mask (32-bit words, as hipExtStreamCreateWithCUMask takes them), and
// attributes every wave's answers to the physical CU and SIMD it ran on.  While fewer CUs than expected have had all
// four SIMDs run a wave, up to GSX_CUTEST_EXTRA_LAUNCHES more launches follow.  Expected CUs: --expect-cus, else the
// popcount of --cu-mask, else the device's CU count.  The loop is gsx::cutest_run, the one gsx_cutest_run has.
// --max-seconds is consulted between launches: the run ends early with "truncated": true, which is no failure.
// --inject (for tests) makes the waves on one physical CU (or one SIMD of it) flip bits of one result value of one
// unit (a name of the table in gsx_kernels.h, or its number).
//
// Prints one JSON line.  Exit 0: clean; 1: wrong answers; 2: the test could not run (bad arguments, which are
// rejected before any HIP call; no such device), or --expect-cus was given and coverage stayed short.
#include <hip/hip_runtime.h>

#include <cinttypes>

#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "tool_common.h"

namespace {

using tool::parse_u64;
using tool::split;
static_assert(GSX_CUTEST_QUICK == 0 && GSX_CUTEST_FULL == 1, "tool::Common::level is the compute test's level");

struct Args : tool::Common {
  std::vector<uint32_t> mask;
  uint32_t expect = 0;
  bool have_expect = false;
  bool inject = false;
  gsx_cutest_inject inj{};
};

struct Result {
  int device = -1;
  std::string bdf;
  double seconds = 0;
  bool truncated = false;
  gsx_cutest_report rep;
};

std::string unit_names(uint32_t mask) {
  std::string s;
  for (int u = 0; u < GSX_CUTEST_UNITS; ++u) {
    if (!(mask >> u & 1)) continue;
    s += s.empty() ? "\"" : ",\"";
    s += gsx_cutest_unit_name(u);
    s += "\"";
  }
  return s;
}

int emit(const Args& a, const Result& r, const char* error, int rc) {
  std::string bad;
  uint32_t failed = 0;
  for (uint32_t k = 0; k < r.rep.n_bad; ++k) {
    const gsx_cutest_bad& b = r.rep.bad[k];
    std::string simds;
    for (int s = 0; s < 4; ++s)
      if (b.simds >> s & 1) simds += (simds.empty() ? "" : ",") + std::to_string(s);
    char buf[256];
    std::snprintf(buf, sizeof buf,
                  "%s{\"xcc\":%u,\"se\":%u,\"sh\":%u,\"cu\":%u,\"simds\":[%s],\"units\":[%s],\"unit\":\"%s\","
                  "\"seed\":%u,\"expected\":%" PRIu64 ",\"got\":%" PRIu64 "}",
                  k ? "," : "", b.xcc, b.se, b.sh, b.cu, simds.c_str(), unit_names(b.units).c_str(),
                  gsx_cutest_unit_name(b.unit), b.seed, b.expected, b.got);
    bad += buf;
  }
  for (const gsx_cutest_cu& c : r.rep.cu) failed |= c.fail_mask;
  std::printf("{\"device\":%d,\"bdf\":\"%s\",\"level\":\"%s\",\"launches\":%u,\"seconds\":%.6f,\"cus_seen\":%u,"
              "\"simds_seen\":%u,\"cus_covered\":%u,\"cus_expected\":%u,\"covered\":%s,\"waves\":%" PRIu64
              ",\"bad_waves\":%" PRIu64 ",\"bad_cu_count\":%u,\"bad_cus\":[%s],\"units_failed\":[%s],"
              "\"truncated\":%s,\"error\":%s}\n",
              r.device, r.bdf.c_str(), a.level_name.c_str(), r.rep.launches, r.seconds, r.rep.cus_seen,
              r.rep.simds_seen, r.rep.cus_covered, r.rep.cus_expected, r.rep.covered ? "true" : "false",
              static_cast<uint64_t>(r.rep.waves), static_cast<uint64_t>(r.rep.bad_waves), r.rep.bad_cus, bad.c_str(),
              unit_names(failed).c_str(), r.truncated ? "true" : "false", tool::json_string(error).c_str());
  std::fflush(stdout);
  return rc;
}

// nullptr, or what is wrong with the command line
const char* parse(int argc, char** argv, Args* a) {
  for (int i = 1; i < argc; i += 2) {
    const char* k = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    const char* why = nullptr;
    uint64_t u = 0;
    if (tool::parse_common(k, v, a, &why)) {
      if (why) return why;
    } else if (!std::strcmp(k, "--cu-mask")) {
      if (!v || !*v) return "--cu-mask needs 32-bit words W0,W1,...";
      uint32_t bits = 0;
      for (const std::string& w : split(v, ',')) {
        if (!parse_u64(w.c_str(), &u) || u > 0xFFFFFFFFull || a->mask.size() >= 32)
          return "--cu-mask needs 32-bit words W0,W1,...";
        a->mask.push_back(static_cast<uint32_t>(u));
        bits += static_cast<uint32_t>(__builtin_popcount(static_cast<uint32_t>(u)));
      }
      if (!bits) return "--cu-mask needs at least one CU";
    } else if (!std::strcmp(k, "--expect-cus")) {
      if (!v || !parse_u64(v, &u) || u == 0 || u > GSX_CUTEST_CU_SLOTS) return "--expect-cus needs a CU count";
      a->expect = static_cast<uint32_t>(u);
      a->have_expect = true;
    } else if (!std::strcmp(k, "--inject")) {
      static const char* bad = "--inject needs XCC:SE:SH:CU[:SIMD]:UNIT:XORMASK (a unit's name or number, a non-zero "
                               "32-bit mask)";
      if (!v) return bad;
      const std::vector<std::string> f = split(v, ':');
      if (f.size() != 6 && f.size() != 7) return bad;
      uint64_t n[4];
      static const uint64_t lim[4] = {15, 7, 1, 15};
      for (int j = 0; j < 4; ++j)
        if (!parse_u64(f[j].c_str(), &n[j]) || n[j] > lim[j]) return bad;
      a->inj.xcc = static_cast<int>(n[0]), a->inj.se = static_cast<int>(n[1]);
      a->inj.sh = static_cast<int>(n[2]), a->inj.cu = static_cast<int>(n[3]);
      a->inj.simd = -1;
      if (f.size() == 7) {
        if (!parse_u64(f[4].c_str(), &u) || u > 3) return bad;
        a->inj.simd = static_cast<int>(u);
      }
      const std::string& unit = f[f.size() - 2];
      a->inj.unit = -1;
      for (int j = 0; j < GSX_CUTEST_UNITS; ++j)
        if (unit == gsx_cutest_unit_name(j) || unit == std::to_string(j)) a->inj.unit = j;
      if (a->inj.unit < 0) return bad;
      if (!parse_u64(f.back().c_str(), &u) || u == 0 || u > 0xFFFFFFFFull) return bad;
      a->inj.xor_mask = static_cast<uint32_t>(u);
      a->inject = true;
    } else {
      return "unknown argument (see the head of tool_cutest.hip)";
    }
  }
  return tool::check_common(*a);
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  Result r;
  std::memset(&r.rep, 0, sizeof r.rep);
  if (const char* why = parse(argc, argv, &a)) return emit(a, r, why, 2);
  // from here on the device is touched
  if (const char* why = tool::open_target(a, &r.device, &r.bdf)) return emit(a, r, why, 2);
  void* st = nullptr;
  if (gsx_stream_create(r.device, a.mask.empty() ? nullptr : a.mask.data(), static_cast<int>(a.mask.size()), &st))
    return emit(a, r, gsx_last_error(), 2);
  // --max-seconds counts from here, the start of the run, when the device is open and the stream made.  The device
  // plugin passes 0.8 of the time it gives the process, as if the budget counted from the start of the process,
  // which gsx-memtest's does and this one does not.
  gsx::CutestOpts opts;
  opts.inject = a.inject ? &a.inj : nullptr;
  opts.max_seconds = a.max_seconds;
  const char* error = nullptr;
  if (gsx::cutest_run(st, a.level, a.expect, opts, &r.rep, &r.seconds, &r.truncated)) error = gsx_last_error();
  (void)gsx_stream_destroy(st);
  if (error) return emit(a, r, error, 2);
  if (r.rep.bad_waves) return emit(a, r, nullptr, 1);
  if (a.have_expect && !r.rep.covered && !r.truncated) return emit(a, r, "coverage stayed short of --expect-cus", 2);
  return emit(a, r, nullptr, 0);
}
