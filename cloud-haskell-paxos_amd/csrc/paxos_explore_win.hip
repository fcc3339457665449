// paxos_explore_win.hip — isolation windows as sites of the exploration
// (include/paxos_batch.h, docs/SEMANTICS.md §17): pxb_explore_win,
// pxb_explore_win_device, pxb_explore_win_row and pxb_explore_win_total.
//
// pxb_explore_cover over a larger space: the joint space's policy
// (explore_win_core.h: ExploreWinX) in the link space's place.  The candidate
// kernel is paxos_explore_cover_kernel's with three changes: candidate g of the
// call is g = i T_w + h T + c, and its lane unranks the link part c as there and
// the window choice h into at most two (acceptor, digit) pairs in registers;
// behind explore_cover_begin it overwrites the lane's windows of the changed
// acceptors (an unrolled walk with selects); and its keys for reach_reduce
// (explore_reach.h) are (parent, r_w, r_l), 12 per parent in place of 4, with
// first[r_w][r_l][b] per cell.  Everything else is shared: the record kernels
// (explore_reach.h), and the minimal kernel with the two-axis subset rule and
// the 12-cell counts, the list, the device form and the host side
// (explore_driver.h).  Here: how the joint space is made, the family's own
// rules, its kernel and its entry points.
//
// Built as three units by proposer count (-DPXB_EXW_P=1|2|3); the unit of P = 1
// also holds the other kernels and the entry points.
#include <hip/hip_runtime.h>

#include "../../include/paxos_batch.h"
#include "explore_reach.h"
#include "explore_win_core.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXW_P
#error "PXB_EXW_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

typedef ReachParams<ExploreWinX> ExwParams;

// (what the lane does around the run is spelled out here and in
// paxos_explore_cover_kernel, as in paxos_explore_kernel: shared, the same text
// compiled to other register counts)
template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_win_kernel(ExwParams k) {
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
    const uint32_t tw = (uint32_t)k.x.Tw, tt = (uint32_t)k.x.e.T;   // (g < 2^32)
    const uint32_t i = (uint32_t)g / tw, cw = (uint32_t)g - i * tw, h = cw / tt, c = cw - h * tt;
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.x.e, explore_unrank(k.x.e, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_cover_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
    if (run) explore_win_apply(L, k.x.w, explore_win_unrank(k.x.w, h));
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
  // (the key is worked out again here, as the coverage kernel does)
  uint32_t key = 0u, cw = 0u;
  if (in) {
    const uint32_t tw = (uint32_t)k.x.Tw, tt = (uint32_t)k.x.e.T, i = (uint32_t)g / tw;
    cw = (uint32_t)g - i * tw;
    const uint32_t h = cw / tt;
    key = i * EXW_CELLS + explore_win_cell(k.x, h, cw - h * tt);
    if (cw == 0u) k.reach[i].parent_mask = m;
  }
  reach_reduce<ExploreWinX>(k.reach, lane, m, key, cw);
}

typedef void (*exw_ptr)(ExwParams);
struct ExwFamily {                  // (lane_shapes.h)
  typedef exw_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_explore_win_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ExwFamily, PXB_EXW_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EXW_P == 1
#include "explore_driver.h"

namespace pxx {

// the joint space of a call (Tw = 0: none); the link part's rules are validate_space_of's
static int win_space_of(const pxb_config* cfg, uint32_t depth, const pxb_explore_win_space* sp, ExploreWin* x) {
  if (!sp) return PXB_E_INVAL;
  ExploreSpace e;
  if (int rc = validate_space_of(cfg, depth, sp->site_depth, sp->radius, &e)) return rc;
  *x = explore_win_make(e, explore_win_space(cfg->n_acceptors, sp->win_radius, sp->win_first, sp->win_starts,
                                             sp->win_lens, (sp->flags & PXB_EXPLORE_WIN_OPEN) != 0u));
  return x->Tw ? PXB_OK : PXB_E_INVAL;
}

// pxb_explore_cover's rules over the joint space; *fn: the shape's kernel
static int validate(const ExpArgs& a, const pxb_explore_win_space* sp, ExploreWin* x, ExwFamily::ptr* fn) {
  if (int rc = win_space_of(a.cfg, a.depth, sp, x)) return rc;
  if (int rc = explore_validate<ExploreWinX>(a, sp)) return rc;
  if ((sp->flag_mask != 0u && (sp->flag_mask & 0xFFu) == 0u) || sp->q.reserved != 0u) return PXB_E_INVAL;
  if (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<ExwFamily>(a.cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxx

extern "C" {

uint64_t pxb_explore_win_total(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp) {
  using namespace pxb::ev;
  if (!sp) return 0ull;
  return explore_win_make(explore_space(explore_sites(P, N, sp->site_depth), delay_max, sp->radius),
                          explore_win_space(N, sp->win_radius, sp->win_first, sp->win_starts, sp->win_lens,
                                            (sp->flags & PXB_EXPLORE_WIN_OPEN) != 0u))
      .Tw;
}

int pxb_explore_win_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_win_space* space,
                        const uint8_t* parent, uint64_t c, uint8_t* out_row) {
  using namespace pxx;
  ExploreWin x;
  if (int rc = win_space_of(cfg, depth, space, &x)) return rc;
  if (!parent || !out_row || c >= x.Tw) return PXB_E_INVAL;
  const uint64_t h = c / x.e.T;
  if (int rc = explore_row_links(cfg, depth, space->site_depth, x.e, parent, c - h * x.e.T, out_row)) return rc;
  const WinCand k = explore_win_unrank(x.w, h);
  for (uint32_t i = 0; i < k.r; ++i) {
    uint32_t c0, c1;
    explore_win_bounds(x.w, k.digit[i], &c0, &c1);
    uint8_t* const o = out_row + SCR_HDR + 4u * k.acc[i];
    o[0] = (uint8_t)c0, o[1] = (uint8_t)(c0 >> 8), o[2] = (uint8_t)c1, o[3] = (uint8_t)(c1 >> 8);
  }
  return PXB_OK;
}

int pxb_explore_win_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                           const pxb_explore_win_space* space, uint64_t first_parent, uint64_t* d_ids,
                           uint64_t capacity, uint64_t* d_n_matches, uint32_t* d_counts,
                           pxb_explore_win_reach* d_reach, uint32_t* d_status, void* stream) {
  using namespace pxx;
  const ExpArgs a{cfg, d_rows, count, depth, first_parent, d_ids, capacity, d_n_matches, d_counts, d_status};
  ExploreWin x;
  ExwFamily::ptr fn = nullptr;
  if (int rc = validate(a, space, &x, &fn)) return rc;
  ExwParams c{};
  c.q = space->q;
  c.reach = d_reach;
  return explore_device<ExploreWinX>(a, space, x, (hipStream_t)stream, fn, c, ReachHooks<ExploreWinX>{d_reach, count});
}

int pxb_explore_win(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                    const pxb_explore_win_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                    uint32_t* counts, pxb_explore_win_reach* reach, uint32_t* status) {
  using namespace pxx;
  const ExpArgs h{cfg, rows, count, depth, 0, ids, capacity, n_matches, counts, status};
  ExploreWin x;
  ExwFamily::ptr fn = nullptr;
  if (int rc = validate(h, space, &x, &fn)) return rc;
  return explore_staged<ExploreWinX>(h, x, reach, sizeof(pxb_explore_win_reach), [&](const ExpArgs& d, void* d_reach) {
    return pxb_explore_win_device(cfg, d.rows, d.count, depth, space, d.first_parent, d.ids, d.capacity, d.n_matches,
                                  d.counts, static_cast<pxb_explore_win_reach*>(d_reach), d.status, nullptr);
  });
}

}  // extern "C"
#endif  // PXB_EXW_P == 1
