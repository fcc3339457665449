// lane_shapes.h — the shapes the lane kernels exist in, once.  pxb_trace_instance
// (paxos_trace.hip), the nine families built as one unit per proposer count
// (paxos_trace_batch, paxos_script, paxos_shrink, paxos_explore, paxos_events,
// paxos_cover, paxos_explore_cover, paxos_explore_win and paxos_shrink_cover .hip) and the host
// builds of their lanes (tests/native/host_lane.h) all pick an instantiation
// here.
//
//   N acceptors in 2..9; the timing wheel W = 8 or 16 steps from
//   wheel_for(delay_max); log mode (n_ticks > 1) on the 8-step wheel only, as
//   the batch kernels' LG shape; one proposer count P in 1..3 per unit.
//
// A caller hands a functor with a `template <int N, int W, bool LG> shape()`
// member (a kernel's address, or a host run of that shape) and what stands for
// "no such shape".  A family of units hands only its description to
// lane_kernel and PXB_LANE_UNIT (below).  Host only and free of HIP.
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "ev_layouts.h"

namespace pxb {
namespace ev {

template <int W, bool LG, class F, class R>
inline R lane_shape_n(uint32_t n, const F& f, R none) {
  switch (n) {
    case 2: return f.template shape<2, W, LG>();
    case 3: return f.template shape<3, W, LG>();
    case 4: return f.template shape<4, W, LG>();
    case 5: return f.template shape<5, W, LG>();
    case 6: return f.template shape<6, W, LG>();
    case 7: return f.template shape<7, W, LG>();
    case 8: return f.template shape<8, W, LG>();
    case 9: return f.template shape<9, W, LG>();
  }
  return none;
}

// f.shape<N, W, LG>() of the config's shape, or `none`
template <class F, class R>
inline R lane_shape(const pxb_config* cfg, const F& f, R none) {
  const int w = wheel_for(cfg->delay_max);
  if (cfg->n_ticks > 1) return w == 8 ? lane_shape_n<8, true>(cfg->n_acceptors, f, none) : none;
  return w == 8    ? lane_shape_n<8, false>(cfg->n_acceptors, f, none)
         : w == 16 ? lane_shape_n<16, false>(cfg->n_acceptors, f, none)
                   : none;
}

// f.proposers<P>() of the config's proposer count, or `none`
template <class F, class R>
inline R lane_proposers(const pxb_config* cfg, const F& f, R none) {
  switch (cfg->n_proposers) {
    case 1: return f.template proposers<1>();
    case 2: return f.template proposers<2>();
    case 3: return f.template proposers<3>();
  }
  return none;
}

// ---- a family built as one unit per proposer count ----
// Its description, the same type in its three units:
//   struct Fam {
//     typedef void (*ptr)(Params);
//     template <int PM, int N, int W, bool LG> static ptr kernel();
//   };
// Each unit says PXB_LANE_UNIT(Fam, P) once, in namespace pxb::ev behind the
// kernel and Fam: it declares lane_unit_pick's three specialisations before any
// use, so that no unit instantiates another's kernels, and defines that of its
// own P.  lane_kernel<Fam>(cfg), anywhere behind that, is the kernel of the
// config's shape among the three units', or null.
template <class Fam, int PM>
typename Fam::ptr lane_unit_pick(const pxb_config* cfg);

template <class Fam, int PM>
struct LaneUnitShape {
  template <int N, int W, bool LG>
  typename Fam::ptr shape() const { return Fam::template kernel<PM, N, W, LG>(); }
};
template <class Fam>
struct LaneUnitPick {
  const pxb_config* cfg;
  template <int PM>
  typename Fam::ptr proposers() const { return lane_unit_pick<Fam, PM>(cfg); }
};
template <class Fam>
inline typename Fam::ptr lane_kernel(const pxb_config* cfg) {
  return lane_proposers(cfg, LaneUnitPick<Fam>{cfg}, (typename Fam::ptr) nullptr);
}

#define PXB_LANE_UNIT(Fam, P)                                                          \
  template <> Fam::ptr lane_unit_pick<Fam, 1>(const pxb_config* cfg);                  \
  template <> Fam::ptr lane_unit_pick<Fam, 2>(const pxb_config* cfg);                  \
  template <> Fam::ptr lane_unit_pick<Fam, 3>(const pxb_config* cfg);                  \
  template <> Fam::ptr lane_unit_pick<Fam, P>(const pxb_config* cfg) {                 \
    return lane_shape(cfg, LaneUnitShape<Fam, P>{}, (Fam::ptr) nullptr);               \
  }

}  // namespace ev
}  // namespace pxb
