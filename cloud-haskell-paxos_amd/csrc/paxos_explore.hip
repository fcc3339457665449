// paxos_explore.hip — bounded exhaustive exploration (include/paxos_batch.h,
// docs/SEMANTICS.md §12): pxb_explore, pxb_explore_device, pxb_explore_row and
// pxb_explore_total.
//
// Every schedule within `radius` changed link entries of each parent row, run
// on the device.  Candidate g of a call is candidate g % T of parent g / T (T is
// the same for every parent: no search), and no candidate row exists: a
// candidate is its parent's row read through ExploreByte (explore_core.h).
// Four kernels and hipCUB's exclusive sum:
//   the candidate kernel: paxos_shrink_kernel's shape over ExploreDraws.  Lane l
//     of block b is candidate 64 b + l; it unranks its changes, tests its at
//     most three site bytes for keep entries, runs to its end under TraceLane
//     with the empty record window and writes ONE flag byte (ran OK, held);
//   the minimal kernel, one thread per candidate: a held candidate ranks its at
//     most 6 proper non-empty subsets and candidate 0, reads their bytes and
//     sets the minimal bit; the wave adds its per-(parent, radius) counts with
//     integer atomics (one add per distinct key and column); the block writes
//     the number of candidates it lists;
//   the cursor kernel and the scatter kernel of paxos_query.hip's list, over
//     the flag bytes: ascending g from the caller's cursor, below `capacity`.
// Everything is sized from count x T: the device form never synchronises.  No
// block waits for another; plain vector stores only.  All but the candidate
// kernel, and the host side of both calls, live in explore_driver.h over the
// link space's policy (explore_core.h: ExploreLinkX), which pxb_explore_cover
// and pxb_explore_win share.
//
// Built as three units by proposer count (-DPXB_EXP_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the other kernels and
// the entry points.  The shapes are lane_shapes.h's.  (The kernel spells out
// what its lane does before and after the run, and tests/native/explore_host.cpp
// spells it again: moved into shared members the same text compiled to other
// register counts)
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "explore_core.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXP_P
#error "PXB_EXP_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct ExpParams {
  EvParams p;
  ExploreSpace x;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  uint64_t total;                   // candidates of this call (count * T <= 2^32)
  uint32_t depth, site_depth, flag_mask;
  uint8_t* bytes;                   // total flag bytes
};

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_kernel(ExpParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ExploreDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 64u + lane;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  TraceLane<Lane> T;
  T.begin_count(1u, 0u);            // (an empty window: no records are counted)
  bool run = g < k.total;
  if (run) {
    const uint32_t tt = (uint32_t)k.x.T, i = (uint32_t)g / tt, c = (uint32_t)g - i * tt;   // (g < 2^32)
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.x, explore_unrank(k.x, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
  }
  const bool started = run;
  script_run(L, T, k.p, run);
  if (g < k.total) {
    uint32_t f = 0u;
    if (started && T.status == PXB_TRACE_OK) {
      uint16_t snt[NL];
      script_sent(L, snt);
      f = explore_flags(T.status, T.res[3], snt, NL, k.depth, k.flag_mask);
    }
    k.bytes[g] = (uint8_t)f;
  }
}

typedef void (*exp_ptr)(ExpParams);
struct ExpFamily {                  // (lane_shapes.h)
  typedef exp_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_explore_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ExpFamily, PXB_EXP_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EXP_P == 1
#include "explore_driver.h"

namespace pxx {

// explore_driver.h's rules and pxb_explore's own: an outcome condition; *fn: the shape's kernel
static int validate(const ExpArgs& a, const pxb_explore_space* sp, ExploreSpace* e, exp_ptr* fn) {
  if (!sp) return PXB_E_INVAL;
  if (int rc = validate_space_of(a.cfg, a.depth, sp->site_depth, sp->radius, e)) return rc;
  if (int rc = explore_validate<ExploreLinkX>(a, sp)) return rc;
  if ((sp->flag_mask & 0xFFu) == 0u) return PXB_E_INVAL;
  *fn = lane_kernel<ExpFamily>(a.cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxx

extern "C" {

uint64_t pxb_explore_total(uint32_t P, uint32_t N, uint32_t delay_max, uint32_t site_depth, uint32_t radius) {
  using namespace pxb::ev;
  return explore_space(explore_sites(P, N, site_depth), delay_max, radius).T;
}

int pxb_explore_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_space* space, const uint8_t* parent,
                    uint64_t c, uint8_t* out_row) {
  using namespace pxx;
  ExploreSpace e;
  if (!space) return PXB_E_INVAL;
  if (int rc = validate_space_of(cfg, depth, space->site_depth, space->radius, &e)) return rc;
  if (!parent || !out_row || c >= e.T) return PXB_E_INVAL;
  return explore_row_links(cfg, depth, space->site_depth, e, parent, c, out_row);
}

int pxb_explore_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                       const pxb_explore_space* space, uint64_t first_parent, uint64_t* d_ids, uint64_t capacity,
                       uint64_t* d_n_matches, uint32_t* d_counts, uint32_t* d_status, void* stream) {
  using namespace pxx;
  const ExpArgs a{cfg, d_rows, count, depth, first_parent, d_ids, capacity, d_n_matches, d_counts, d_status};
  ExploreSpace e;
  exp_ptr fn = nullptr;
  if (int rc = validate(a, space, &e, &fn)) return rc;
  ExpParams c{};
  return explore_device<ExploreLinkX>(a, space, e, (hipStream_t)stream, fn, c, ExploreNoHooks{});
}

int pxb_explore(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                const pxb_explore_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                uint32_t* counts, uint32_t* status) {
  using namespace pxx;
  const ExpArgs h{cfg, rows, count, depth, 0, ids, capacity, n_matches, counts, status};
  ExploreSpace e;
  exp_ptr fn = nullptr;
  if (int rc = validate(h, space, &e, &fn)) return rc;
  return explore_staged<ExploreLinkX>(h, e, nullptr, 0, [&](const ExpArgs& d, void*) {
    return pxb_explore_device(cfg, d.rows, d.count, depth, space, d.first_parent, d.ids, d.capacity, d.n_matches,
                              d.counts, d.status, nullptr);
  });
}

}  // extern "C"
#endif  // PXB_EXP_P == 1
