// ev_layouts.h — the per-lane kernel's layouts, once: which template arguments
// of ev::paxos_ev_kernel a layout index stands for, which unit of paxos_ev.hip
// builds it, for which proposer counts, and which configs it may run.  Host
// only and free of HIP, so that the table and the rules are unit-tested on the
// CPU (tests/native/route_plan_host.cpp, tests/native/ev_host.cpp).
//
// paxos_ev.hip's instantiations, paxos_batch.hip's extern declarations and
// dispatch, and ev_host.cpp's dispatch are all expansions of PXB_EV_LAYOUTS.
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"

// One row per layout: X(id, W, CMP, LG, SL, SP, part, built)
//   W     timing-wheel steps (it must outlast the longest delay: wheel_for)
//   CMP   compact links (Shape::CMP), LG log-mode fields, SL slim (byte reply
//         seqs in registers), SP simple schedule (1) / tight (2)
//   part  the unit of paxos_ev.hip (-DPXB_EV_PART) that instantiates it: 0 the
//         wide, compact and simple-schedule shapes, 1 the log-mode and slim ones
//   built the proposer counts it is built for: ALL (1, 2, 3) or P2
// Rows are in instantiation order, unit by unit.
#define PXB_EV_LAYOUTS(X)                                                                          \
  /* 0: 8-step wheel, 4-entry FIFOs */                                                             \
  X(0, 8, false, false, false, 0, 0, ALL)                                                          \
  /* 1: 16-step wheel (delays above 8) */                                                          \
  X(1, 16, false, false, false, 0, 0, ALL)                                                         \
  /* 2: compact links (3-entry request FIFOs sharing a word with the reply seq, a 24-word          \
     response pool), 8-step wheel */                                                               \
  X(2, 8, true, false, false, 0, 0, ALL)                                                           \
  /* 3: compact links on the 4-step wheel (delays up to 4: BASELINE configs 3 and 4), 4 words      \
     per lane fewer */                                                                             \
  X(3, 4, true, false, false, 0, 0, ALL)                                                           \
  /* 6: layout 3 for simple schedules (no loss, no Tick skew, single decree: layout_for) */        \
  X(6, 4, true, false, false, 1, 0, ALL)                                                           \
  /* 7: layout 6 with halfword response FIFOs (tight: the first launch of the two-proposer         \
     simple schedules, P = 2 only) */                                                              \
  X(7, 4, true, false, false, 2, 0, P2)                                                            \
  /* 4: log mode (8-step wheel, 4-entry FIFOs, LG fields) */                                       \
  X(4, 8, false, true, false, 0, 1, ALL)                                                           \
  /* 8: log mode on the 16-step wheel with its topology's larger pool (the second stage behind     \
     layouts 4 and 9 over <= 10 links) */                                                          \
  X(8, 16, false, true, false, 0, 1, ALL)                                                          \
  /* 5: layout 0 slimmed (byte reply seqs) for runs of at most 512 steps (BASELINE config 5) */    \
  X(5, 8, false, false, true, 0, 1, ALL)                                                           \
  /* 9: layout 4 slimmed (byte reply seqs in registers) on the 4-step wheel (the first stage of    \
     log mode over <= 10 links with delays <= 4) */                                                \
  X(9, 4, false, true, true, 0, 1, ALL)

// M(pm, ...) for every proposer count of a row's `built` column
#define PXB_EV_BUILT_ALL(M, ...) M(1, __VA_ARGS__) M(2, __VA_ARGS__) M(3, __VA_ARGS__)
#define PXB_EV_BUILT_P2(M, ...) M(2, __VA_ARGS__)
#define PXB_EV_PMASK_ALL 0xEu
#define PXB_EV_PMASK_P2 0x4u

namespace pxb {
namespace ev {

constexpr uint32_t MAX_STEP_CAP = 4095;   // 12-bit tickets (tickets <= step_cap, SEMANTICS §6)
static_assert(MAX_STEP_CAP < PXB_TICKET_LIMIT, "EV tickets never reach the overflow limit");

struct Layout {
  int wheel;                          // 0: no such layout
  bool compact, log, slim;
  int simple;                         // Shape's SP
  int part;
  uint32_t pmask;                     // bit pm: built for pm proposers
};

inline Layout layout_row(int layout) {
  switch (layout) {
#define PXB_EV_ROW(ID, W, C, L, S, SP, PART, BUILT) \
  case ID: return Layout{W, C, L, S, SP, PART, PXB_EV_PMASK_##BUILT};
    PXB_EV_LAYOUTS(PXB_EV_ROW)
#undef PXB_EV_ROW
  }
  return Layout{0, false, false, false, 0, 0, 0u};
}
inline int layout_wheel(int layout) { return layout_row(layout).wheel; }
inline bool layout_compact(int layout) { return layout_row(layout).compact; }
inline bool layout_simple(int layout) { return layout_row(layout).simple != 0; }
inline bool layout_log(int layout) { return layout_row(layout).log; }
inline bool layout_built(int layout, uint32_t pm) { return pm < 32u && ((layout_row(layout).pmask >> pm) & 1u); }

// EV eligibility of a launch: faulty, 12-bit tickets, delays inside the
// 16-step wheel (log mode: inside the 8-step one, its first stage's).
// Fault-free batches keep the paxos_ff1.h / paxos_ffp.h / paxos_kernel.h kernels.
inline bool eligible(const pxb_config* c) {
  return c->step_cap <= MAX_STEP_CAP && c->delay_max <= (c->n_ticks > 1 ? 8u : 15u);
}

// the timing wheel must outlast the longest delay: sends at step s (or s - 1
// for a carried-over copy) fall due in [s, s + delay_max] (a link's FIFO tail
// is at most its last send step + delay_max), the slot of s is emptied on
// entering s and a copy due at s goes straight to the step's due links, so
// the wheel holds dues in [s + 1, s + delay_max]: 8 slots serve delays up to 8
// (4 slots up to 4)
inline int wheel_for(uint32_t delay_max) { return delay_max <= 8 ? 8 : 16; }

// Kernel layout of a launch (its only, or its chunk-wide, stage; route_plan.h
// adds the stages of the two-stage routings).  Short delays keep FIFOs short
// (BASELINE config 4: 0.9 % of instances ever hold a fourth request on one
// link, config 3: 0.02 %; those are bailed to the general kernel), so they take
// the compact layout, which fits more resident waves; fuzzed or long-delay
// schedules keep 4-entry FIFOs.  The compact reply seq has 9 bits (config 4
// reaches 68 in 256 steps), so long runs keep the separate 16-bit one; three
// duelling proposers over 9 acceptors overflow the 3-entry FIFOs too often
// (25 % of instances at 10 % loss), so the compact layout is kept to
// topologies of <= 16 links.
inline int layout_for(const pxb_config* c) {
  if (c->n_ticks > 1) return 4;                      // log mode: 8-step wheel, 4-entry FIFOs, LG fields
  if (!(c->flags & PXB_CFG_RANDOMIZE) && c->delay_max <= 4 && c->step_cap <= 512 &&
      c->n_proposers * c->n_acceptors <= 16)
    return (c->loss_ppm == 0 && c->skew_max == 0) ? 6 : 3;   // 6: layout 3, simple schedule (Shape::SP)
  if (wheel_for(c->delay_max) != 8) return 1;
#ifndef PXB_EV_NO_SLIM
  if (c->step_cap <= 512) return 5;                  // slim: byte reply seqs suffice
#endif
  return 0;
}

// Whether `layout` may run an eligible config: its wheel outlasts the delays,
// the log-mode fields run log mode and nothing else, and the simple layouts
// run only what they assume (no loss draw, every proposer's one Tick at step 0)
inline bool layout_serves(int layout, const pxb_config* c) {
  const Layout r = layout_row(layout);
  if (!r.wheel || (uint32_t)r.wheel < c->delay_max) return false;
  if (r.log != (c->n_ticks > 1)) return false;
  if (r.simple && (c->loss_ppm || c->skew_max || (c->flags & PXB_CFG_RANDOMIZE) || c->n_ticks > 1)) return false;
  return true;
}

}  // namespace ev
}  // namespace pxb
