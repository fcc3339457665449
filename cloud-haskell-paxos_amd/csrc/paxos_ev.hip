// paxos_ev.hip — explicit instantiations of the per-lane kernel
// (paxos_ev_kernel.h) for one proposer count (-DPXB_EV_P=1|2|3): every layout
// of ev_layouts.h built for that count, over the 8 acceptor counts.  Split by P
// and by part (-DPXB_EV_PART=0|1; neither: both) -- two units per proposer
// count, so that each builds in parallel and takes its own scheduler flags,
// __graft_entry__.py.
#include "paxos_ev_kernel.h"

#if !defined(PXB_EV_P)
#error "compile with -DPXB_EV_P=1|2|3"
#endif

namespace pxb {
namespace ev {
#define PXB_EV_INST(N, W, C, L, S, SP) template __global__ void paxos_ev_kernel<PXB_EV_P, N, W, C, L, S, SP>(EvKParams);
#define PXB_EV_FOR_N(W, C, L, S, SP) PXB_EV_INST(2, W, C, L, S, SP) PXB_EV_INST(3, W, C, L, S, SP) \
  PXB_EV_INST(4, W, C, L, S, SP) PXB_EV_INST(5, W, C, L, S, SP) PXB_EV_INST(6, W, C, L, S, SP) \
  PXB_EV_INST(7, W, C, L, S, SP) PXB_EV_INST(8, W, C, L, S, SP) PXB_EV_INST(9, W, C, L, S, SP)
// a row's instantiations, when this unit is its part and its proposer count is built
#define PXB_EV_IF_ALL(...) __VA_ARGS__
#if PXB_EV_P == 2
#define PXB_EV_IF_P2(...) __VA_ARGS__
#else
#define PXB_EV_IF_P2(...)
#endif
#if !defined(PXB_EV_PART) || PXB_EV_PART == 0
#define PXB_EV_IF_PART0(...) __VA_ARGS__
#else
#define PXB_EV_IF_PART0(...)
#endif
#if !defined(PXB_EV_PART) || PXB_EV_PART == 1
#define PXB_EV_IF_PART1(...) __VA_ARGS__
#else
#define PXB_EV_IF_PART1(...)
#endif
#define PXB_EV_ROW(ID, W, C, L, S, SP, PART, BUILT) PXB_EV_IF_PART##PART(PXB_EV_IF_##BUILT(PXB_EV_FOR_N(W, C, L, S, SP)))
PXB_EV_LAYOUTS(PXB_EV_ROW)
}  // namespace ev
}  // namespace pxb
