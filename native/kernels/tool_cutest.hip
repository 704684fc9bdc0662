// gsx-cutest: the compute pre-flight as an operator tool (kernel: cutest.hip).
//
//   gsx-cutest [--device N | --bdf DDDD:BB:DD.F] [--level quick|full] [--cu-mask W0,W1,...]
//              [--expect-cus N] [--max-seconds S] [--inject XCC:SE:SH:CU[:SIMD]:UNIT:XORMASK]
//
// Runs the level's launches (gsx_cutest_seeds; 4 workgroups per expected CU, each taking a CU's whole LDS) on the
// device, or on a stream restricted to --cu-mask (32-bit words, as hipExtStreamCreateWithCUMask takes them), and
// attributes every wave's answers to the physical CU and SIMD it ran on.  While fewer CUs than expected have had all
// four SIMDs run a wave, up to GSX_CUTEST_EXTRA_LAUNCHES more launches follow.  Expected CUs: --expect-cus, else the
// popcount of --cu-mask, else the device's CU count.
// --max-seconds is consulted between launches: the run ends early with "truncated": true, which is no failure.
// --inject (for tests) makes the waves on one physical CU (or one SIMD of it) flip bits of one result value of one
// unit (a name of the table in gsx_kernels.h, or its number).
//
// Prints one JSON line.  Exit 0: clean; 1: wrong answers; 2: the test could not run (bad arguments, which are
// rejected before any HIP call; no such device), or --expect-cus was given and coverage stayed short.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gsx_kernels.h"

namespace {

struct Args {
  int device = 0;
  std::string bdf;
  int level = GSX_CUTEST_QUICK;
  std::string level_name = "quick";
  std::vector<uint32_t> mask;
  uint32_t expect = 0;
  bool have_expect = false;
  double max_seconds = 0;
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

bool parse_u64(const char* s, uint64_t* out) {
  if (!*s || *s == '-') return false;
  char* end = nullptr;
  errno = 0;
  const unsigned long long v = std::strtoull(s, &end, 0);
  if (errno || !end || *end) return false;
  *out = v;
  return true;
}

std::vector<std::string> split(const char* s, char sep) {
  std::vector<std::string> out(1);
  for (; *s; ++s) {
    if (*s == sep) {
      out.emplace_back();
    } else {
      out.back() += *s;
    }
  }
  return out;
}

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
  std::string err = "null";
  if (error) {
    err = "\"";
    for (const char* c = error; *c; ++c) {
      if (*c == '"' || *c == '\\') err += '\\';
      err += static_cast<unsigned char>(*c) < 0x20 ? ' ' : *c;
    }
    err += "\"";
  }
  std::printf("{\"device\":%d,\"bdf\":\"%s\",\"level\":\"%s\",\"launches\":%u,\"seconds\":%.6f,\"cus_seen\":%u,"
              "\"simds_seen\":%u,\"cus_covered\":%u,\"cus_expected\":%u,\"covered\":%s,\"waves\":%" PRIu64
              ",\"bad_waves\":%" PRIu64 ",\"bad_cu_count\":%u,\"bad_cus\":[%s],\"units_failed\":[%s],"
              "\"truncated\":%s,\"error\":%s}\n",
              r.device, r.bdf.c_str(), a.level_name.c_str(), r.rep.launches, r.seconds, r.rep.cus_seen,
              r.rep.simds_seen, r.rep.cus_covered, r.rep.cus_expected, r.rep.covered ? "true" : "false",
              static_cast<uint64_t>(r.rep.waves), static_cast<uint64_t>(r.rep.bad_waves), r.rep.bad_cus, bad.c_str(),
              unit_names(failed).c_str(), r.truncated ? "true" : "false", err.c_str());
  std::fflush(stdout);
  return rc;
}

// nullptr, or what is wrong with the command line
const char* parse(int argc, char** argv, Args* a) {
  bool have_dev = false;
  for (int i = 1; i < argc; ++i) {
    const char* k = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    uint64_t u = 0;
    if (!std::strcmp(k, "--device")) {
      if (!v || !parse_u64(v, &u) || u > 1023) return "--device needs an index";
      a->device = static_cast<int>(u);
      have_dev = true;
    } else if (!std::strcmp(k, "--bdf")) {
      if (!v || !*v) return "--bdf needs DDDD:BB:DD.F";
      unsigned d, b, dv, f;
      char tail;
      if (std::sscanf(v, "%x:%x:%x.%x%c", &d, &b, &dv, &f, &tail) != 4) return "--bdf needs DDDD:BB:DD.F";
      a->bdf = v;
    } else if (!std::strcmp(k, "--level")) {
      if (!v || (std::strcmp(v, "quick") && std::strcmp(v, "full"))) return "--level needs quick or full";
      a->level_name = v;
      a->level = !std::strcmp(v, "full") ? GSX_CUTEST_FULL : GSX_CUTEST_QUICK;
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
    } else if (!std::strcmp(k, "--max-seconds")) {
      char* end = nullptr;
      a->max_seconds = v ? std::strtod(v, &end) : -1;
      if (!v || !*v || *end || !(a->max_seconds >= 0)) return "--max-seconds needs a number of seconds";
    } else if (!std::strcmp(k, "--inject")) {
      static const char* why = "--inject needs XCC:SE:SH:CU[:SIMD]:UNIT:XORMASK (a unit's name or number, a non-zero "
                               "32-bit mask)";
      if (!v) return why;
      const std::vector<std::string> f = split(v, ':');
      if (f.size() != 6 && f.size() != 7) return why;
      uint64_t n[4];
      static const uint64_t lim[4] = {15, 7, 1, 15};
      for (int j = 0; j < 4; ++j)
        if (!parse_u64(f[j].c_str(), &n[j]) || n[j] > lim[j]) return why;
      a->inj.xcc = static_cast<int>(n[0]), a->inj.se = static_cast<int>(n[1]);
      a->inj.sh = static_cast<int>(n[2]), a->inj.cu = static_cast<int>(n[3]);
      a->inj.simd = -1;
      if (f.size() == 7) {
        if (!parse_u64(f[4].c_str(), &u) || u > 3) return why;
        a->inj.simd = static_cast<int>(u);
      }
      const std::string& unit = f[f.size() - 2];
      a->inj.unit = -1;
      for (int j = 0; j < GSX_CUTEST_UNITS; ++j)
        if (unit == gsx_cutest_unit_name(j) || unit == std::to_string(j)) a->inj.unit = j;
      if (a->inj.unit < 0) return why;
      if (!parse_u64(f.back().c_str(), &u) || u == 0 || u > 0xFFFFFFFFull) return why;
      a->inj.xor_mask = static_cast<uint32_t>(u);
      a->inject = true;
    } else {
      return "unknown argument (see the head of tool_cutest.hip)";
    }
    ++i;
  }
  if (have_dev && !a->bdf.empty()) return "--device and --bdf exclude each other";
  return nullptr;
}

double since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  Result r;
  std::memset(&r.rep, 0, sizeof r.rep);
  if (const char* why = parse(argc, argv, &a)) return emit(a, r, why, 2);
  // from here on the device is touched
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return emit(a, r, "no HIP device", 2);
  int dev = a.device;
  if (!a.bdf.empty() && hipDeviceGetByPCIBusId(&dev, a.bdf.c_str()) != hipSuccess)
    return emit(a, r, "no device with this --bdf", 2);
  if (dev < 0 || dev >= ndev || hipSetDevice(dev) != hipSuccess) return emit(a, r, "no such device", 2);
  r.device = dev;
  char bdf[32] = "";
  if (hipDeviceGetPCIBusId(bdf, sizeof bdf, dev) == hipSuccess) r.bdf = bdf;
  void* st = nullptr;
  if (gsx_stream_create(dev, a.mask.empty() ? nullptr : a.mask.data(), static_cast<int>(a.mask.size()), &st))
    return emit(a, r, gsx_last_error(), 2);
  uint32_t expect = a.expect;
  if (!expect && gsx_cutest_stream_cus(st, &expect)) {
    (void)gsx_stream_destroy(st);
    return emit(a, r, gsx_last_error(), 2);
  }
  r.rep.cus_expected = expect;
  const uint32_t want = 4u * expect;
  const int blocks = static_cast<int>(want < GSX_CUTEST_MAX_BLOCKS ? want : GSX_CUTEST_MAX_BLOCKS);
  std::vector<gsx_cutest_record> recs(4u * static_cast<size_t>(blocks));
  const uint32_t seeds = gsx_cutest_seeds(a.level);
  const auto t0 = std::chrono::steady_clock::now();
  const char* error = nullptr;
  // gsx_cutest_run's loop, with the clock looked at between launches and the injection passed on
  for (uint32_t k = 0; k < seeds || (r.rep.cus_covered < expect && k < seeds + GSX_CUTEST_EXTRA_LAUNCHES); ++k) {
    if (a.max_seconds > 0 && since(t0) >= a.max_seconds) {
      r.truncated = true;
      break;
    }
    const uint32_t n = static_cast<uint32_t>(recs.size());
    if (gsx_cutest_launch(st, k, blocks, a.inject ? &a.inj : nullptr, recs.data(), n) ||
        gsx_cutest_aggregate(recs.data(), n, &r.rep)) {
      error = gsx_last_error();
      break;
    }
    ++r.rep.launches;
  }
  r.rep.covered = r.rep.cus_covered >= expect;
  r.seconds = since(t0);
  (void)gsx_stream_destroy(st);
  if (error) return emit(a, r, error, 2);
  if (r.rep.bad_waves) return emit(a, r, nullptr, 1);
  if (a.have_expect && !r.rep.covered && !r.truncated) return emit(a, r, "coverage stayed short of --expect-cus", 2);
  return emit(a, r, nullptr, 0);
}
