// stage_plan.h — the carve of one staging allocation (host_stage.h): regions
// are added in order as (element size, element count); each add returns the
// region with its offset.  A region of zero bytes takes no space; every other
// one starts on a 256-byte boundary; the total is the padded sum.  Every
// product and sum is checked: a plan that would overflow is marked invalid
// (the caller returns PXB_E_INVAL) instead of wrapping.  The plan keeps only
// the running total; a region carries its own offset and size.
//
// Pure arithmetic with no HIP in it: the .hip units and the host test
// (tests/native/stage_plan_host.cpp) compile the same text.
#pragma once
#include <stdint.h>

namespace pxb {

constexpr uint64_t STAGE_ALIGN = 256;

struct StageRegion {
  uint64_t offset;                  // from the allocation's base
  uint64_t elem;                    // bytes per element
  uint64_t count;                   // elements (of an invalid plan: 0)
  bool late;                        // host_stage.h: in the late allocation, not the plan's
  uint64_t bytes() const { return elem * count; }
};

struct StagePlan {
  uint64_t total = 0;               // bytes to allocate: the padded end of the last region
  bool valid = true;

  StageRegion add(uint64_t elem, uint64_t count) {
    uint64_t bytes = 0, end = 0, padded = 0;
    const bool fits = !__builtin_mul_overflow(elem, count, &bytes) && !__builtin_add_overflow(total, bytes, &end) &&
                      !__builtin_add_overflow(end, STAGE_ALIGN - 1, &padded) && padded <= (uint64_t)SIZE_MAX;
    if (!valid || !fits) {
      valid = false;
      return StageRegion{0, elem, 0, false};
    }
    const StageRegion r{total, elem, count, false};
    total = padded & ~(STAGE_ALIGN - 1);          // (total stays a multiple of the alignment)
    return r;
  }
};

}  // namespace pxb
