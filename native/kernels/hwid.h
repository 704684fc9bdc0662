// Where a wave ran: the fields of gfx9's HW_REG_HW_ID and HW_REG_XCC_ID that name a physical CU and a SIMD of it, and
// a CU's slot in gsx_cutest_report.cu[].  The one native definition, for kernels and host code; its Python twin is
// ops/hip.py (decode_hw_id, cu_slot, slot_cu).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsx {

#define GSX_HWID_FN __host__ __device__ __forceinline__

// the two registers as a wave read them; a field is decoded where it is asked for
struct HwId {
  uint32_t hw_id, xcc_id;
  GSX_HWID_FN uint32_t xcc() const { return xcc_id & 0xF; }
  GSX_HWID_FN uint32_t se() const { return (hw_id >> 13) & 0x7; }
  GSX_HWID_FN uint32_t sh() const { return (hw_id >> 12) & 0x1; }
  GSX_HWID_FN uint32_t cu() const { return (hw_id >> 8) & 0xF; }
  GSX_HWID_FN uint32_t simd() const { return (hw_id >> 4) & 0x3; }
};

// GSX_CUTEST_CU_SLOTS of them
GSX_HWID_FN uint32_t cu_slot(HwId w) { return w.xcc() << 8 | w.se() << 5 | w.sh() << 4 | w.cu(); }

// the inverse: a wave (slot 0 of SIMD 0) on that CU
GSX_HWID_FN HwId slot_cu(uint32_t slot) {
  return {((slot >> 5) & 0x7) << 13 | ((slot >> 4) & 0x1) << 12 | (slot & 0xF) << 8, slot >> 8};
}

#undef GSX_HWID_FN

}  // namespace gsx
