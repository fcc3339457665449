// explore_host.h — TEST ONLY: what explore_host.cpp, explore_cover_host.cpp and
// explore_win_host.cpp share, over a space policy X (explore_core.h:
// ExploreLinkX; explore_win_core.h: ExploreWinX).
//   explore_host_parent<X>  what follows a parent's candidates: the sequential
//                           statement of explore_driver.h's minimal kernel and list;
//   explore_host_reach<X>   a parent's reach record: the sequential statement of
//                           explore_reach.h's wave reduction and record kernels;
//   CoverCand<X>, cover_run_shape, cover_dispatch
//                           one candidate of a covering family: what one lane of
//                           its candidate kernel does before its wave's reduction;
//   explore_cover_host_run<X>
//                           a covering family's device form on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/explore_cover_core.h"
#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/script_lane.h"
#include "host_lane.h"

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

// Parent i (its row, of P proposers' space x) with its candidates' flag bytes
// f[0..total): the minimal bits into f (the held bits are final before any is
// set), the CELLS x 3 counts, the listing of the `sel` bit from *o.pos, the
// status and the copy of the bytes.
template <class X>
inline void explore_host_parent(const typename X::Space& x, uint32_t P, const uint8_t* row, uint64_t i, uint32_t sel,
                                uint8_t* f, const ExploreHostOut& o) {
  using namespace pxb::ev;
  const uint64_t T = X::total(x);
  uint32_t cnt[X::CELLS * 3u] = {0u};
  for (uint64_t cw = 0; cw < T; ++cw) {
    const ExploreSplit s = X::split(x, (uint32_t)cw);
    if ((f[cw] & EXP_HELD) && X::is_minimal(x, s.h, s.c, f)) f[cw] |= (uint8_t)EXP_MINIMAL;
    for (uint32_t b = 0; b < 3u; ++b) cnt[X::cell(x, s.h, s.c) * 3u + b] += (f[cw] >> b) & 1u;
    if (f[cw] & sel) {
      if (*o.pos < o.capacity) o.ids[*o.pos] = (o.first_parent + i) * T + cw;
      ++*o.pos;
    }
  }
  if (o.counts) memcpy(o.counts + i * X::CELLS * 3u, cnt, sizeof(cnt));
  if (o.status) o.status[i] = explore_parent_bad(row, P) ? PXB_SCRIPT_BAD : PXB_TRACE_OK;
  if (o.bytes) memcpy(o.bytes + i * T, f, (size_t)T);
}

// the reach record of a parent from its candidates' masks m[0..total), folded by cell and class
template <class X>
inline typename X::Reach explore_host_reach(const typename X::Space& x, const uint32_t* m) {
  using namespace pxb::ev;
  typename X::Reach r;
  memset(&r, 0, sizeof r);
  memset(r.first, 0xFF, sizeof r.first);
  r.parent_mask = m[0];
  for (uint64_t cw = 0; cw < X::total(x); ++cw) {
    const ExploreSplit s = X::split(x, (uint32_t)cw);
    const uint32_t cell = X::cell(x, s.h, s.c);
    for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b)
      if ((m[cw] >> b) & 1u) {
        X::count(&r, cell)[b] += 1u;
        if ((uint32_t)cw < X::first(&r, cell)[b]) X::first(&r, cell)[b] = (uint32_t)cw;
        r.union_mask |= 1u << b;
      }
  }
  return r;
}

// one candidate of a covering family
template <class X>
struct CoverCand {
  const pxb_config* cfg;
  const typename X::Space* x;
  const uint8_t* row;
  uint32_t depth, site_depth, cw, flag_mask;
  const pxb_cover_query* q;
  uint8_t* flags;
  uint32_t* mask;
};

template <class X, int PM, int N, int W, bool LG>
int cover_run_shape(const CoverCand<X>& a) {
  using namespace pxb;
  using namespace pxb::ev;
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ExploreEventDraws>::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  *a.flags = 0u;
  *a.mask = 0u;
  const ExploreSplit s = X::split(*a.x, a.cw);
  const ExploreSpace& e = X::links(*a.x);
  const ExploreByte x = explore_byte(e, explore_unrank(e, s.c), a.row, N, a.site_depth, a.depth);
  if (explore_parent_bad(a.row, PM) || explore_changes_keep(x)) return 0;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  uint64_t guard = 0;
  if (explore_cover_begin(L, p, a.depth, a.row, x) != PXB_TRACE_OK) return 0;
  X::apply(L, *a.x, s.h);
  while (E.iter(L, p))
    if (++guard > guard_max) return -100;
  if (E.status != PXB_TRACE_OK) return 0;
  uint16_t snt[NL];
  script_sent(L, snt);
  const uint32_t f = explore_cover_flags(E.res[3], E.mask, snt, NL, a.depth, a.flag_mask, *a.q);
  *a.flags = (uint8_t)f;
  *a.mask = (f & EXP_RAN) ? E.mask : 0u;
  return 0;
}

#if defined(PXB_EXPLORE_COVER_HOST_MAIN) || defined(PXB_EXPLORE_WIN_HOST_MAIN)
// (the sanitizer builds: one shape, P = 1, N = 3 on the 8-step wheel)
template <class X>
int cover_dispatch(const CoverCand<X>& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 1 || c->n_acceptors != 3 || pxb::ev::wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return cover_run_shape<X, 1, 3, 8, false>(a);
}
#else
// (the shapes of lane_shapes.h; -1: none)
template <class X>
struct CoverRun {
  const CoverCand<X>& a;
  template <int PM, int N, int W, bool LG>
  int run() const { return cover_run_shape<X, PM, N, W, LG>(a); }
};
template <class X>
int cover_dispatch(const CoverCand<X>& a) { return host_lane_shape(a.cfg, CoverRun<X>{a}, -1); }
#endif

// A covering family's device form on the host over the space x (0 candidates:
// none), sp: its space struct; `reach` (nullable); `bytes` (nullable): count *
// total flag bytes, what the kernels keep in scratch; `masks` (nullable): count
// * total masks, which the kernels keep nowhere.
template <class X, class Space>
int explore_cover_host_run(const pxb_config* cfg, const typename X::Space& x, const uint8_t* rows, uint64_t count,
                           uint32_t depth, const Space* sp, const ExploreHostOut& out, uint64_t* n_matches,
                           typename X::Reach* reach, uint32_t* masks) {
  using namespace pxb::ev;
  if (!n_matches || (count && !rows) || (sp->flag_mask && !(sp->flag_mask & 0xFFu)) || (sp->flags & ~X::FLAGS) ||
      sp->q.reserved || (out.capacity && !out.ids) || (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return PXB_E_INVAL;
  const uint64_t T = X::total(x);
  if (!T || count * T > (1ull << 32)) return PXB_E_INVAL;
  const uint32_t P = cfg->n_proposers;
  const uint64_t stride = script_stride(P, cfg->n_acceptors, depth);
  const uint32_t sel = (sp->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  uint64_t pos = *n_matches;
  ExploreHostOut o = out;
  o.pos = &pos;
  std::vector<uint8_t> f((size_t)T);
  std::vector<uint32_t> m((size_t)T);
  for (uint64_t i = 0; i < count; ++i) {
    const uint8_t* const row = rows + i * stride;
    for (uint64_t cw = 0; cw < T; ++cw)
      if (int rc = cover_dispatch(CoverCand<X>{cfg, &x, row, depth, sp->site_depth, (uint32_t)cw, sp->flag_mask, &sp->q,
                                               &f[(size_t)cw], &m[(size_t)cw]}))
        return rc;
    explore_host_parent<X>(x, P, row, i, sel, f.data(), o);
    const typename X::Reach r = explore_host_reach<X>(x, m.data());
    if (reach) memcpy(reinterpret_cast<unsigned char*>(reach) + i * sizeof r, &r, sizeof r);
    if (masks) memcpy(masks + i * T, m.data(), (size_t)T * 4u);
  }
  *n_matches = pos;
  return 0;
}

// the rules of a call's link space, which every host form tests first
template <class Space>
inline bool explore_host_link_rules(const pxb_config* cfg, uint32_t depth, const Space* sp) {
  return cfg && sp && depth <= PXB_SCRIPT_MAX_DEPTH && sp->site_depth != 0u && sp->site_depth <= depth &&
         sp->radius <= PXB_EXPLORE_MAX_RADIUS && pxb::ev::trace_config_ok(cfg);
}
