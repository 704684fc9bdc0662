// What gsx-memtest and gsx-cutest share: number and list parsing, the options both have, the JSON form of the error
// text, and opening the device.  Plain functions; each tool keeps its own Args, Result and emit.
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace tool {

inline bool parse_u64(const char* s, uint64_t* out) {
  if (!*s || *s == '-') return false;
  char* end = nullptr;
  errno = 0;
  const unsigned long long v = std::strtoull(s, &end, 0);
  if (errno || !end || *end) return false;
  *out = v;
  return true;
}

inline std::vector<std::string> split(const char* s, char sep) {
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

// null, or the text quoted: quotes and backslashes escaped, control characters blanked
inline std::string json_string(const char* s) {
  if (!s) return "null";
  std::string out = "\"";
  for (; *s; ++s) {
    if (*s == '"' || *s == '\\') out += '\\';
    out += static_cast<unsigned char>(*s) < 0x20 ? ' ' : *s;
  }
  return out + "\"";
}

inline double since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The options both tools have.  level: 0 quick, 1 full, which is GSX_MEMTEST_* and GSX_CUTEST_* alike.
struct Common {
  int device = 0;
  bool have_device = false;
  std::string bdf;
  int level = 0;
  std::string level_name = "quick";
  double max_seconds = 0;
};

// false: `k` is none of them.  true: it is, and *why is nullptr or what is wrong with its value `v` (nullptr: none)
inline bool parse_common(const char* k, const char* v, Common* c, const char** why) {
  *why = nullptr;
  if (!std::strcmp(k, "--device")) {
    uint64_t u = 0;
    if (!v || !parse_u64(v, &u) || u > 1023) {
      *why = "--device needs an index";
    } else {
      c->device = static_cast<int>(u);
      c->have_device = true;
    }
  } else if (!std::strcmp(k, "--bdf")) {
    unsigned d, b, dv, f;
    char tail;
    if (!v || !*v || std::sscanf(v, "%x:%x:%x.%x%c", &d, &b, &dv, &f, &tail) != 4) {
      *why = "--bdf needs DDDD:BB:DD.F";
    } else {
      c->bdf = v;
    }
  } else if (!std::strcmp(k, "--level")) {
    if (!v || (std::strcmp(v, "quick") && std::strcmp(v, "full"))) {
      *why = "--level needs quick or full";
    } else {
      c->level_name = v;
      c->level = !std::strcmp(v, "full");
    }
  } else if (!std::strcmp(k, "--max-seconds")) {
    char* end = nullptr;
    c->max_seconds = v ? std::strtod(v, &end) : -1;
    if (!v || !*v || *end || !(c->max_seconds >= 0)) *why = "--max-seconds needs a number of seconds";
  } else {
    return false;
  }
  return true;
}

// after the last argument
inline const char* check_common(const Common& c) {
  return c.have_device && !c.bdf.empty() ? "--device and --bdf exclude each other" : nullptr;
}

// Makes the device of --device / --bdf current: nullptr, with its index and bus id in *device and *bdf, or why not.
// The first HIP call of a tool.
inline const char* open_target(const Common& c, int* device, std::string* bdf) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return "no HIP device";
  int dev = c.device;
  if (!c.bdf.empty() && hipDeviceGetByPCIBusId(&dev, c.bdf.c_str()) != hipSuccess) return "no device with this --bdf";
  if (dev < 0 || dev >= ndev || hipSetDevice(dev) != hipSuccess) return "no such device";
  *device = dev;
  char id[32] = "";
  if (hipDeviceGetPCIBusId(id, sizeof id, dev) == hipSuccess) *bdf = id;
  return nullptr;
}

}  // namespace tool
