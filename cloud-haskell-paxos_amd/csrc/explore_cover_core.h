// explore_cover_core.h — coverage of the candidates of an exploration
// (include/paxos_batch.h: pxb_explore_cover, docs/SEMANTICS.md §15): what the
// kernels (paxos_explore_cover.hip) and the host unit test
// (tests/native/explore_cover_host.cpp) share, as plain C++ over explore_core.h
// (the space, ExploreByte) and cover_core.h (CoverLane over the tapped draws).
//
//   ExploreEventDraws   EventDraws whose link bytes go through ExploreByte: the
//                       ExploreDraws pattern on the tapped base, so that
//                       CoverLane folds a candidate no row of which exists;
//   explore_cover_begin script_begin for such a candidate;
//   explore_cover_flags the flag byte: EXP_RAN as §12, EXP_HELD by §15's
//                       predicate (ran OK, the outcome flags unless flag_mask is
//                       0, and the coverage query).
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "cover_core.h"
#include "explore_core.h"

namespace pxb {
namespace ev {

static_assert(sizeof(pxb_explore_reach) == 4 * 32 * 4 + 32 * 4 + 8, "pxb_explore_reach: 648 bytes");
static_assert(sizeof(pxb_explore_cover_space) == 32, "pxb_explore_cover_space: 32 bytes");

struct ExploreEventDraws : EventDraws {
  ExploreByte x_byte;
  __host__ __device__ __forceinline__ uint4 source_draw(uint32_t lo, uint32_t hi, uint32_t c2, uint32_t c3,
                                                        const uint32_t (&rk)[20]) const {
    return source_draw_over(lo, hi, c2, c3, rk, x_byte);
  }
};

// script_begin for the candidate `x` of the parent `row`
template <class Lane>
__host__ __device__ __forceinline__ uint32_t explore_cover_begin(Lane& L, const EvParams& kp, uint32_t depth,
                                                                 const uint8_t* row, const ExploreByte& x) {
  ExploreEventDraws& D = L;
  D.x_byte = x;
  return script_begin(L, kp, depth, row);
}

// the flag byte of a candidate that ended with status PXB_TRACE_OK and mask m
__host__ __device__ __forceinline__ uint32_t explore_cover_flags(uint32_t flags, uint32_t m, const uint16_t* sent,
                                                                 uint32_t n_links, uint32_t depth, uint32_t flag_mask,
                                                                 const pxb_cover_query& q) {
  uint32_t mx = 0u;
  for (uint32_t i = 0; i < n_links; ++i) mx = sent[i] > mx ? sent[i] : mx;
  const bool ran = mx <= depth;
  const bool held = ran & ((flag_mask == 0u) | ((flags & 0xFFu & flag_mask) != 0u)) &
                    cover_match(m, q.all_mask, q.any_mask, q.none_mask);
  return (ran ? EXP_RAN : 0u) | (held ? EXP_HELD : 0u);
}

}  // namespace ev
}  // namespace pxb
