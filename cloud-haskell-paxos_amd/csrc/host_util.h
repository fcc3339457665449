// host_util.h — what the entry points of the tool families (trace batch,
// scripted schedules, shrinker, explorer, query, wire codec) share on the host
// side on top of host_stage.h (the error mapping and the host buffers' staging):
// the scratch padding, the device checks, the per-call scratch pool's
// declaration and the uint32 -> uint64 widening iterator that hipCUB's
// exclusive sums read counts through.  Internal to the library's
// .hip units; a unit built per proposer count includes it only where its entry
// points are (hipCUB is slow to compile).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "host_stage.h"

namespace pxw {
// paxos_wire.hip: per-call scratch from the device's stream-ordered pool
// (allocated and freed on the caller's stream; pxb_shutdown destroys the pool)
int scratch(int dev, size_t bytes, hipStream_t st, void** p);
}  // namespace pxw

namespace pxb {
namespace host {

constexpr uint64_t MAX_COUNT = 1ull << 30;        // rows, ids or parents of one call

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// the current device (< 64: pxw::scratch keeps one pool per device in an array of 64)
inline int current_device(int* dev) {
  return (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= 64) ? PXB_E_NODEV : PXB_OK;
}

struct Widen {
  __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& c) const { return c; }
};
typedef hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*> widen_iter;

}  // namespace host
}  // namespace pxb
