// paxos_explore_cover.hip — which handler classes lie within k faults of a row
// (include/paxos_batch.h, docs/SEMANTICS.md §15): pxb_explore_cover,
// pxb_explore_cover_device.
//
// pxb_explore's space and list with pxb_cover's fold.  The candidate kernel is
// paxos_explore_kernel's with CoverLane (cover_core.h) in TraceLane's place over
// ExploreEventDraws (explore_cover_core.h): lane l of block b is candidate
// 64 b + l of the call, which unranks its changes, tests its site bytes for keep
// entries, runs to its end folding its events into its mask in registers and
// writes ONE flag byte (ran OK, held by §15's predicate).  No candidate row, no
// event and no per-candidate mask is ever stored.  The wave then reduces into
// the parents' reach records by its (parent, radius) keys: reach_reduce
// (explore_reach.h, with the kernels that set and finish the records) over the
// link space's policy (explore_core.h: ExploreLinkX; one first[b] a record).
// The list, the device form and the host side are explore_driver.h's over the
// same policy.  No block waits for another; plain vector stores only.
//
// Built as three units by proposer count (-DPXB_EXC_P=1|2|3); the unit of P = 1
// also holds the other kernels and the entry points.
#include <hip/hip_runtime.h>

#include "../../include/paxos_batch.h"
#include "explore_reach.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXC_P
#error "PXB_EXC_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

typedef ReachParams<ExploreLinkX> ExcParams;

// (what the lane does around the run is spelled out here and in
// paxos_explore_win_kernel, as in paxos_explore_kernel: shared, the same text
// compiled to other register counts)
template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_cover_kernel(ExcParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ExploreEventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 64u + lane;
  const bool in = g < k.total;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  bool run = in;
  if (run) {
    const uint32_t tt = (uint32_t)k.x.T, i = (uint32_t)g / tt, c = (uint32_t)g - i * tt;   // (g < 2^32)
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.x, explore_unrank(k.x, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_cover_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
  }
  const bool started = run;
  script_run(L, E, k.p, run);
  uint32_t f = 0u, m = 0u;
  if (started && E.status == PXB_TRACE_OK) {
    uint16_t snt[NL];
    script_sent(L, snt);
    f = explore_cover_flags(E.res[3], E.mask, snt, NL, k.depth, k.flag_mask, k.q);
    m = (f & EXP_RAN) ? E.mask : 0u;
  }
  if (in) k.bytes[g] = (uint8_t)f;
  if (k.reach == nullptr) return;   // (wave-uniform)
  uint32_t key = 0u, c = 0u;
  if (in) {
    const uint32_t tt = (uint32_t)k.x.T, i = (uint32_t)g / tt;
    c = (uint32_t)g - i * tt;
    key = i * 4u + explore_radius(k.x, c);
    if (c == 0u) k.reach[i].parent_mask = m;
  }
  reach_reduce<ExploreLinkX>(k.reach, lane, m, key, c);
}

typedef void (*exc_ptr)(ExcParams);
struct ExcFamily {                  // (lane_shapes.h)
  typedef exc_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_explore_cover_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ExcFamily, PXB_EXC_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EXC_P == 1
#include "explore_driver.h"

namespace pxx {

// explore_driver.h's rules and pxb_explore_cover's own: no outcome condition, or
// one over the outcome bits; no reserved word; no production draws (the event
// lanes have none); *fn: the shape's kernel
static int validate(const ExpArgs& a, const pxb_explore_cover_space* sp, ExploreSpace* e, ExcFamily::ptr* fn) {
  if (!sp) return PXB_E_INVAL;
  if (int rc = validate_space_of(a.cfg, a.depth, sp->site_depth, sp->radius, e)) return rc;
  if (int rc = explore_validate<ExploreLinkX>(a, sp)) return rc;
  if ((sp->flag_mask != 0u && (sp->flag_mask & 0xFFu) == 0u) || sp->q.reserved != 0u) return PXB_E_INVAL;
  if (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<ExcFamily>(a.cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxx

extern "C" {

int pxb_explore_cover_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                             const pxb_explore_cover_space* space, uint64_t first_parent, uint64_t* d_ids,
                             uint64_t capacity, uint64_t* d_n_matches, uint32_t* d_counts, pxb_explore_reach* d_reach,
                             uint32_t* d_status, void* stream) {
  using namespace pxx;
  const ExpArgs a{cfg, d_rows, count, depth, first_parent, d_ids, capacity, d_n_matches, d_counts, d_status};
  ExploreSpace e;
  ExcFamily::ptr fn = nullptr;
  if (int rc = validate(a, space, &e, &fn)) return rc;
  ExcParams c{};
  c.q = space->q;
  c.reach = d_reach;
  return explore_device<ExploreLinkX>(a, space, e, (hipStream_t)stream, fn, c, ReachHooks<ExploreLinkX>{d_reach, count});
}

int pxb_explore_cover(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                      const pxb_explore_cover_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                      uint32_t* counts, pxb_explore_reach* reach, uint32_t* status) {
  using namespace pxx;
  const ExpArgs h{cfg, rows, count, depth, 0, ids, capacity, n_matches, counts, status};
  ExploreSpace e;
  ExcFamily::ptr fn = nullptr;
  if (int rc = validate(h, space, &e, &fn)) return rc;
  return explore_staged<ExploreLinkX>(h, e, reach, sizeof(pxb_explore_reach), [&](const ExpArgs& d, void* d_reach) {
    return pxb_explore_cover_device(cfg, d.rows, d.count, depth, space, d.first_parent, d.ids, d.capacity,
                                    d.n_matches, d.counts, static_cast<pxb_explore_reach*>(d_reach), d.status,
                                    nullptr);
  });
}

}  // extern "C"
#endif  // PXB_EXC_P == 1
