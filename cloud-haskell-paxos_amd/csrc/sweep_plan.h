// sweep_plan.h — the chunk arithmetic of pxb_sweep (paxos_batch.hip), host only
// and free of HIP so that it is unit-tested on the CPU
// (tests/native/sweep_plan_host.cpp): chunk k of a sweep of n instances from
// global id `first` covers ids [first + k * chunk, ...) and is `chunk` long
// except for a ragged last one; n == 0 has no chunks.  Ids are 64-bit
// throughout (a sweep may cross 2^32).
#pragma once
#include <stdint.h>

namespace pxb {

constexpr uint64_t SWEEP_CHUNK_DEFAULT = 1ull << 24;        // 256 MiB of results
constexpr uint64_t SWEEP_CHUNK_MAX = (1ull << 30) - 1;      // one pxb_run_device chunk

// PXB_SWEEP_CHUNK as read from the environment (absent: the default)
inline uint64_t sweep_clamp_chunk(long long v) {
  if (v < 1) return 1;
  return ((uint64_t)v > SWEEP_CHUNK_MAX) ? SWEEP_CHUNK_MAX : (uint64_t)v;
}

struct SweepChunk {
  uint64_t first, count;
};

inline uint64_t sweep_n_chunks(uint64_t n, uint64_t chunk) { return n / chunk + (n % chunk ? 1u : 0u); }

inline SweepChunk sweep_chunk_at(uint64_t first, uint64_t n, uint64_t chunk, uint64_t k) {
  const uint64_t done = k * chunk;
  const uint64_t left = n - done;
  return SweepChunk{first + done, left < chunk ? left : chunk};
}

}  // namespace pxb
