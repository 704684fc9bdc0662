// gsx-memtest: the HBM pre-flight memory test as an operator tool (kernels: memtest.hip).
//
//   gsx-memtest [--device N | --bdf DDDD:BB:DD.F] [--bytes N|all] [--reserve BYTES] [--chunk BYTES]
//               [--level quick|full] [--max-seconds S] [--inject OFFSET:XORMASK]
//
// --bytes all (the default) tests hipMemGetInfo's free memory minus --reserve (default 1 GiB).  Inside a pod the
// isolation library reports the pod's share as the pool, so `all` tests the share.  The memory is allocated in
// chunks (--chunk, default 8 GiB, at least 1 GiB; the last chunk is what remains), all held at once so that no
// two chunks are the same physical memory, and tested chunk by chunk with the level's pass sequence
// (gsx_memtest_pass).  A chunk is far larger than the 256 MiB Infinity Cache and every pass sweeps it in ascending
// order, so a check reads what the pass before it left in HBM, not in a cache; a --bytes below the cache size
// does not have that property.
// --max-seconds is consulted between passes: the run ends early with "truncated": true, which is no failure.  It
// counts from the start of the process, as the timeout of whoever started the tool does: opening the device and
// allocating the chunks use it up too.  "seconds" and "gbps" cover the passes alone.
// --inject (for tests) XORs one dword of the tool's own buffer, through a host copy, after the first write pass
// of the chunk that holds it.
//
// Prints one JSON line.  Exit 0: clean; 1: memory errors found; 2: the test could not run (bad arguments, which
// are rejected before any HIP call; no such device; allocation failure).
#include <hip/hip_runtime.h>

#include <algorithm>
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
  bool all = true;
  uint64_t bytes = 0, reserve = 1ull << 30, chunk = 8ull << 30;
  int level = GSX_MEMTEST_QUICK;
  std::string level_name = "quick";
  double max_seconds = 0;
  bool inject = false;
  uint64_t inject_off = 0;
  uint32_t inject_mask = 0;
};

struct Result {
  int device = -1;
  std::string bdf;
  uint64_t bytes_tested = 0, bytes_moved = 0;
  uint32_t passes = 0, chunks = 0;
  double seconds = 0;
  bool truncated = false;
  gsx_memtest_report rep;
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

int emit(const Args& a, const Result& r, const char* error, int rc) {
  std::string errs;
  for (uint32_t k = 0; k < r.rep.n_errs; ++k) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s{\"offset\":%" PRIu64 ",\"expected\":%u,\"actual\":%u}", k ? "," : "",
                  r.rep.errs[k].offset, r.rep.errs[k].expected, r.rep.errs[k].actual);
    errs += buf;
  }
  std::string err = "null";
  if (error) {
    err = "\"";
    for (const char* c = error; *c; ++c) {
      if (*c == '"' || *c == '\\') err += '\\';
      err += static_cast<unsigned char>(*c) < 0x20 ? ' ' : *c;
    }
    err += "\"";
  }
  std::printf("{\"device\":%d,\"bdf\":\"%s\",\"level\":\"%s\",\"bytes_tested\":%" PRIu64 ",\"bytes_moved\":%" PRIu64
              ",\"passes\":%u,\"chunks\":%u,\"seconds\":%.6f,\"gbps\":%.1f,\"bad_dwords\":%" PRIu64
              ",\"flipped_or\":%u,\"errors\":[%s],\"truncated\":%s,\"error\":%s}\n",
              r.device, r.bdf.c_str(), a.level_name.c_str(), r.bytes_tested, r.bytes_moved, r.passes, r.chunks,
              r.seconds, r.seconds > 0 ? static_cast<double>(r.bytes_moved) / r.seconds / 1e9 : 0.0,
              static_cast<uint64_t>(r.rep.bad_dwords), r.rep.flipped_or, errs.c_str(), r.truncated ? "true" : "false",
              err.c_str());
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
    } else if (!std::strcmp(k, "--bytes")) {
      if (!v) return "--bytes needs N or all";
      a->all = !std::strcmp(v, "all");
      if (!a->all && (!parse_u64(v, &a->bytes) || a->bytes == 0 || a->bytes % 16))
        return "--bytes needs a positive multiple of 16, or all";
    } else if (!std::strcmp(k, "--reserve")) {
      if (!v || !parse_u64(v, &a->reserve)) return "--reserve needs a byte count";
    } else if (!std::strcmp(k, "--chunk")) {
      if (!v || !parse_u64(v, &a->chunk) || a->chunk < (1ull << 30) || a->chunk % 16)
        return "--chunk needs a multiple of 16 of at least 1 GiB";
    } else if (!std::strcmp(k, "--level")) {
      if (!v || (std::strcmp(v, "quick") && std::strcmp(v, "full"))) return "--level needs quick or full";
      a->level_name = v;
      a->level = !std::strcmp(v, "full") ? GSX_MEMTEST_FULL : GSX_MEMTEST_QUICK;
    } else if (!std::strcmp(k, "--max-seconds")) {
      char* end = nullptr;
      a->max_seconds = v ? std::strtod(v, &end) : -1;
      if (!v || !*v || *end || !(a->max_seconds >= 0)) return "--max-seconds needs a number of seconds";
    } else if (!std::strcmp(k, "--inject")) {
      const char* colon = v ? std::strchr(v, ':') : nullptr;
      uint64_t m = 0;
      if (!colon || !parse_u64(std::string(v, colon - v).c_str(), &a->inject_off) || !parse_u64(colon + 1, &m) ||
          m == 0 || m > 0xFFFFFFFFull || a->inject_off % 4)
        return "--inject needs OFFSET:XORMASK (a dword offset, a non-zero 32-bit mask)";
      a->inject = true;
      a->inject_mask = static_cast<uint32_t>(m);
    } else {
      return "unknown argument (see the head of tool_memtest.hip)";
    }
    ++i;
  }
  if (have_dev && !a->bdf.empty()) return "--device and --bdf exclude each other";
  if (a->inject && !a->all && a->inject_off >= a->bytes) return "--inject offset beyond --bytes";
  return nullptr;
}

double since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char** argv) {
  const auto started = std::chrono::steady_clock::now();  // what --max-seconds counts from
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
  uint64_t bytes = a.bytes;
  if (a.all) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return emit(a, r, "hipMemGetInfo failed", 2);
    if (free_b <= a.reserve + 16) return emit(a, r, "no free memory beyond --reserve", 2);
    bytes = (free_b - a.reserve) / 16 * 16;
  }
  if (a.inject && a.inject_off >= bytes) return emit(a, r, "--inject offset beyond the tested bytes", 2);
  // every chunk is held until the end: two chunks are never the same physical memory
  std::vector<std::pair<void*, uint64_t>> chunks;
  auto release = [&] {
    for (auto& c : chunks) (void)hipFree(c.first);
  };
  for (uint64_t done = 0; done < bytes;) {
    const uint64_t n = std::min<uint64_t>(a.chunk, bytes - done);
    void* p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess || !p) {
      (void)hipGetLastError();
      release();
      return emit(a, r, "device allocation failed", 2);
    }
    chunks.emplace_back(p, n);
    done += n;
  }
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
    release();
    return emit(a, r, "stream creation failed", 2);
  }
  const auto t0 = std::chrono::steady_clock::now();
  const char* error = nullptr;
  uint64_t origin = 0;
  for (size_t c = 0; c < chunks.size() && !error && !r.truncated; ++c) {
    void* base = chunks[c].first;
    const uint64_t n = chunks[c].second;
    bool inject = a.inject && a.inject_off >= origin && a.inject_off < origin + n;
    gsx_memtest_pass_t ps;
    bool complete = true;
    for (uint32_t k = 0; gsx_memtest_pass(a.level, k, &ps) == 0; ++k) {
      if (a.max_seconds > 0 && since(started) >= a.max_seconds) {
        r.truncated = true;
        complete = false;
        break;
      }
      int rc;
      if (ps.write) {
        rc = gsx_memtest_write(st, base, n, origin, ps.pattern, ps.seed, ps.invert);
        if (!rc && inject) {
          // one dword of our own buffer, flipped through the host: a data mismatch for the check to find
          inject = false;
          uint32_t w = 0;
          char* at = static_cast<char*>(base) + (a.inject_off - origin);
          if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(&w, at, 4, hipMemcpyDeviceToHost) != hipSuccess) {
            error = "--inject: reading the dword failed";
            break;
          }
          w ^= a.inject_mask;
          if (hipMemcpy(at, &w, 4, hipMemcpyHostToDevice) != hipSuccess) {
            error = "--inject: writing the dword failed";
            break;
          }
        }
      } else {
        rc = gsx_memtest_check(st, base, n, origin, ps.pattern, ps.seed, ps.invert, ps.rewrite, &r.rep);
      }
      if (rc) {
        error = gsx_last_error();
        complete = false;
        break;
      }
      ++r.passes;
      r.bytes_moved += n * (ps.rewrite ? 2 : 1);
    }
    if (error) break;
    if (complete) {
      r.bytes_tested += n;
      ++r.chunks;
    }
    origin += n;
  }
  if (hipStreamSynchronize(st) != hipSuccess && !error) error = "stream synchronisation failed";
  r.seconds = since(t0);
  (void)hipStreamDestroy(st);
  release();
  if (error) return emit(a, r, error, 2);
  return emit(a, r, nullptr, r.rep.bad_dwords ? 1 : 0);
}
