// shrink_cover_core.h — the batched shrinker over a coverage predicate
// (include/paxos_batch.h: pxb_shrink_cover_batch, docs/SEMANTICS.md §16): what
// the candidate kernel (paxos_shrink_cover.hip) and the host unit test
// (tests/native/shrink_cover_host.cpp) share, as plain C++ over shrink_core.h
// (the rank tables, ShrParams) and cover_core.h (CoverLane over the tapped
// draws).
//
//   ShrinkEventDraws    EventDraws whose link bytes go through the rank test:
//                       the ShrinkDraws pattern on the tapped base, so that
//                       CoverLane folds a candidate no row of which exists;
//   shrink_cover_holds  §16's predicate: shrink_holds' conditions with the
//                       outcome one dropped when flag_mask is 0, and the
//                       coverage query;
//   ShcParams           the candidate kernel's parameters, with what one lane
//                       does before its run (begin: ShrParams::start on the
//                       tapped draws under CoverLane).
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "cover_core.h"
#include "shrink_core.h"

namespace pxb {
namespace ev {

static_assert(sizeof(pxb_shrink_pred) == 32, "pxb_shrink_pred: 32 bytes");

typedef ShrinkDrawsOver<EventDraws> ShrinkEventDraws;

// the predicate of an ended candidate: status, the result's flags word, its
// coverage mask and its send counts (script_sent's 2 P N halfwords)
__host__ __device__ inline bool shrink_cover_holds(uint32_t status, uint32_t flags, uint32_t m, const uint16_t* sent,
                                                   uint32_t n_links, uint32_t depth, uint32_t flag_mask,
                                                   const pxb_cover_query& q) {
  uint32_t mx = 0u;
  for (uint32_t i = 0; i < n_links; ++i) mx = sent[i] > mx ? sent[i] : mx;
  return (status == PXB_TRACE_OK) & ((flag_mask == 0u) | ((flags & 0xFFu & flag_mask) != 0u)) &
         cover_match(m, q.all_mask, q.any_mask, q.none_mask) & (mx <= depth);
}

// ---- the candidate kernel's parameters: job c is candidate c of the launch ----
struct ShcParams {
  ShrParams s;                      // (flag_mask may be 0 here)
  pxb_cover_query q;
  uint32_t* cmask;                  // total (nullable): the candidates' coverage masks

  template <class Lane, class Cover>
  __host__ __device__ __forceinline__ bool begin(Lane& L, Cover& E, uint64_t c) const {
    L.e_acc = L.e_pin = false;      // (an iteration without an acceptor op or a proposer op leaves its taps)
    E.begin();
    bool run = c < s.total;
    if (run) {
      const uint32_t st = s.template start<ShrinkEventDraws>(L, c);
      if (st != PXB_TRACE_OK) {     // a malformed row: not run
        E.status = st;
        run = false;
      }
    }
    return run;
  }
};

}  // namespace ev
}  // namespace pxb
