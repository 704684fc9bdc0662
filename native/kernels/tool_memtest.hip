// gsx-memtest: the HBM pre-flight memory test as an operator tool (kernels: memtest.hip).
//
//   gsx-memtest [--device N | --bdf DDDD:BB:DD.F] [--bytes N|all] [--reserve BYTES] [--chunk BYTES]
//               [--level quick|full] [--max-seconds S] [--inject OFFSET:XORMASK]
//
// --bytes all (the default) tests hipMemGetInfo's free memory minus --reserve (default 1 GiB).  Inside a pod the
// isolation library reports the pod's share as the pool, so `all` tests the share.  The memory is allocated in
// chunks (--chunk, default 8 GiB, at least 1 GiB; the last chunk is what remains), all held at once so that no
// two chunks are the same physical memory, and tested chunk by chunk with the level's pass sequence
// (gsx::memtest_run, the loop of gsx_memtest_run).  A chunk is far larger than the 256 MiB Infinity Cache and every
// pass sweeps it in ascending order, so a check reads what the pass before it left in HBM, not in a cache; a
// --bytes below the cache size does not have that property.
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
#include <cinttypes>

#include "gsx_internal.h"
#include "gsx_kernels.h"
#include "tool_common.h"

namespace {

using tool::parse_u64;
using tool::since;
static_assert(GSX_MEMTEST_QUICK == 0 && GSX_MEMTEST_FULL == 1, "tool::Common::level is the memory test's level");

struct Args : tool::Common {
  bool all = true;
  uint64_t bytes = 0, reserve = 1ull << 30, chunk = 8ull << 30;
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

int emit(const Args& a, const Result& r, const char* error, int rc) {
  std::string errs;
  for (uint32_t k = 0; k < r.rep.n_errs; ++k) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s{\"offset\":%" PRIu64 ",\"expected\":%u,\"actual\":%u}", k ? "," : "",
                  r.rep.errs[k].offset, r.rep.errs[k].expected, r.rep.errs[k].actual);
    errs += buf;
  }
  std::printf("{\"device\":%d,\"bdf\":\"%s\",\"level\":\"%s\",\"bytes_tested\":%" PRIu64 ",\"bytes_moved\":%" PRIu64
              ",\"passes\":%u,\"chunks\":%u,\"seconds\":%.6f,\"gbps\":%.1f,\"bad_dwords\":%" PRIu64
              ",\"flipped_or\":%u,\"errors\":[%s],\"truncated\":%s,\"error\":%s}\n",
              r.device, r.bdf.c_str(), a.level_name.c_str(), r.bytes_tested, r.bytes_moved, r.passes, r.chunks,
              r.seconds, r.seconds > 0 ? static_cast<double>(r.bytes_moved) / r.seconds / 1e9 : 0.0,
              static_cast<uint64_t>(r.rep.bad_dwords), r.rep.flipped_or, errs.c_str(), r.truncated ? "true" : "false",
              tool::json_string(error).c_str());
  std::fflush(stdout);
  return rc;
}

// nullptr, or what is wrong with the command line
const char* parse(int argc, char** argv, Args* a) {
  for (int i = 1; i < argc; i += 2) {
    const char* k = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    const char* why = nullptr;
    if (tool::parse_common(k, v, a, &why)) {
      if (why) return why;
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
  }
  if (const char* why = tool::check_common(*a)) return why;
  if (a->inject && !a->all && a->inject_off >= a->bytes) return "--inject offset beyond --bytes";
  return nullptr;
}

}  // namespace

int main(int argc, char** argv) {
  const auto started = std::chrono::steady_clock::now();  // what --max-seconds counts from
  Args a;
  Result r;
  std::memset(&r.rep, 0, sizeof r.rep);
  if (const char* why = parse(argc, argv, &a)) return emit(a, r, why, 2);
  // from here on the device is touched
  if (const char* why = tool::open_target(a, &r.device, &r.bdf)) return emit(a, r, why, 2);
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
  // (a budget of more than 1e9 s is none, and would not fit the clock's ticks)
  const auto deadline = started + std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                      std::chrono::duration<double>(std::min(a.max_seconds, 1e9)));
  const auto t0 = std::chrono::steady_clock::now();
  const char* error = nullptr;
  uint64_t origin = 0;
  for (size_t c = 0; c < chunks.size() && !r.truncated; ++c) {
    const uint64_t n = chunks[c].second;
    gsx::MemtestOpts opts;
    if (a.max_seconds > 0) opts.deadline = &deadline;
    if (a.inject && a.inject_off >= origin && a.inject_off < origin + n)
      opts.flip_offset = a.inject_off - origin, opts.flip_mask = a.inject_mask;
    if (gsx::memtest_run(st, chunks[c].first, n, origin, a.level, opts, &r.rep, &r.passes, &r.bytes_moved,
                         &r.truncated)) {
      error = gsx_last_error();
      break;
    }
    if (!r.truncated) {  // only complete chunks count
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
