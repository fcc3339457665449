// explore_host.h — TEST ONLY: what explore_host.cpp and explore_cover_host.cpp
// do per parent once its T candidates have run: the sequential statement of
// explore_driver.h's minimal kernel and list.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../cloud-haskell-paxos_amd/csrc/explore_core.h"

// a call's outputs behind the flag bytes (every pointer but pos nullable, ids
// with capacity 0); *pos: the list's cursor, which the parents advance
struct ExploreHostOut {
  uint64_t first_parent;
  uint64_t* ids;
  uint64_t capacity;
  uint64_t* pos;
  uint32_t* counts;
  uint32_t* status;
  uint8_t* bytes;
};

// Parent i (its row, of P proposers' space e) with its candidates' flag bytes
// f[0..T): the minimal bits into f, the 12 counts, the listing of the `sel`
// bit from *o.pos, the status and the copy of the bytes.
inline void explore_host_parent(const pxb::ev::ExploreSpace& e, uint32_t P, const uint8_t* row, uint64_t i, uint32_t sel,
                                uint8_t* f, const ExploreHostOut& o) {
  using namespace pxb::ev;
  uint32_t cnt[12] = {0u};
  for (uint64_t c = 0; c < e.T; ++c) {
    const ExploreCand k = explore_unrank(e, c);
    if ((f[c] & EXP_HELD) && explore_is_minimal(e, k, f)) f[c] |= (uint8_t)EXP_MINIMAL;
    for (uint32_t b = 0; b < 3u; ++b) cnt[k.r * 3u + b] += (f[c] >> b) & 1u;
    if (f[c] & sel) {
      if (*o.pos < o.capacity) o.ids[*o.pos] = (o.first_parent + i) * e.T + c;
      ++*o.pos;
    }
  }
  if (o.counts) memcpy(o.counts + i * 12u, cnt, sizeof(cnt));
  if (o.status) o.status[i] = explore_parent_bad(row, P) ? PXB_SCRIPT_BAD : PXB_TRACE_OK;
  if (o.bytes) memcpy(o.bytes + i * e.T, f, (size_t)e.T);
}
