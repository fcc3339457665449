// route_plan.h — which kernels pxb_run_device (paxos_batch.hip) launches for a
// config, as a pure function of the config and the routing hooks.  Host only
// and free of HIP, so that every rule is unit-tested on the CPU
// (tests/native/route_plan_host.cpp, tests/test_route_plan.py).
//
//   route_plan(cfg, hooks)          the plan, before any device query
//   route_resolve(plan, occ1, occ2) the plan once the occupancy of its two
//                                   per-lane stages is known
//   route_chunk_max(plan, ...)      instances per chunk
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "ev_layouts.h"

namespace pxb {

// queue words of a launch slot: [0] the general kernel's work queue, [1] the
// per-lane kernel's, [2] its bailed-instance count; two-stage routings: [3] the
// second per-lane kernel's queue, [4] its bailed-instance count
[[maybe_unused]] constexpr uint32_t Q_GEN = 0, Q_EV = 1, Q_BAIL = 2, Q_EV2 = 3, Q_BAIL2 = 4;   // (Q_GEN: kp.queue itself)

// Per-lane kernel: one launch per EV_CHUNK instances; its bailed ids go to a
// list of EV_BAIL_CAP entries (16 MB) kept per (device, stream): launches of
// one stream run in order, so they can share it.  Bails are rare
// (BASELINE configs: <= 1.5 %); a chunk whose list overflows is re-run whole
// by the general kernel (finalize_kernel then drops the per-lane totals).
// Big chunks matter: each one ends with a tail (the slowest instances of the
// last waves, then of the bailed ones on the general kernel); config 4 at 2^26
// on one GPU: 2^24-instance chunks 1292.6 ms, 2^25 1283.8, 2^26 1277.3.  The
// list holds 1/16 of a chunk (16 MB per slot).
constexpr uint64_t EV_CHUNK = 1ull << 26;
constexpr uint32_t EV_BAIL_CAP = 1u << 22;
// split routing (fuzzed P = 3 batches, config 5): the per-lane kernel of a
// two-proposer shape takes the instances that drew P <= 2 and lists the P = 3
// ones (a third) with its bails for the three-proposer shape, so that list
// holds half a chunk; split chunks are 2^25 instances (64 MB lists, allocated
// for the slots two-stage launches use; config 5 at 2^25: 34.9 M/s with 2^24
// chunks, 36.2 with 2^25)
constexpr uint64_t EV_SPLIT_CHUNK = 1ull << 25;
constexpr uint32_t EV_SPLIT_CAP = (uint32_t)(EV_SPLIT_CHUNK / 2);

// the routing subset of the test and A/B hooks (paxos_batch.hip's Hooks)
struct RouteHooks {
  bool no_ev, no_ff1, no_ffp, no_split, no_tight, no_lg2, no_lgs;
  int bail_cap;                   // PXB_EV_BAIL_CAP (-1: the default)
};

enum RouteKind { ROUTE_GENERAL, ROUTE_FF1, ROUTE_FFP, ROUTE_EV };
enum RouteTwoStage { TWO_NONE, TWO_SPLIT, TWO_TIGHT, TWO_LG2 };

struct RouteStage {
  uint32_t pm;                    // the shape's proposer capacity
  int layout;                     // ev_layouts.h
};

struct RoutePlan {
  RouteKind kind;
  // the general kernel's template arguments: it runs the whole chunk
  // (ROUTE_GENERAL) or the last list of bailed ids (every other kind)
  bool logm, ff;
  // ROUTE_EV: `second` over the chunk, or (two_stage) `first` over the chunk
  // and `second` over the ids it lists
  RouteTwoStage two_stage;
  RouteStage first, second;
  // two_stage is taken only when the first stage fits more blocks per CU than
  // the second (route_resolve); false: whenever it is planned
  bool conditional;
  uint64_t chunk;                 // ROUTE_EV: instances per chunk
  uint32_t first_cap, cap;        // capacities of the first stage's id list and of the last one
  uint32_t bail_word;             // the queue word finalize_kernel reads: the last list's count
};

inline RoutePlan route_plan(const pxb_config* c, const RouteHooks& hk) {
  RoutePlan r{};
  const uint32_t P = c->n_proposers, N = c->n_acceptors;
  r.logm = c->n_ticks > 1;              // log mode: several Ticks per proposer
  // fault-free schedule: no message is lost, delayed past the next step or sent
  // to an isolated acceptor (Tick skew is allowed)
  const bool ff = !(c->flags & PXB_CFG_RANDOMIZE) && c->loss_ppm == 0 && c->delay_max == 1 && c->crash_ppm == 0;
  // tests: a smaller bailed-id list, to exercise its overflow path
  r.cap = r.first_cap = hk.bail_cap >= 0 && (uint32_t)hk.bail_cap < EV_BAIL_CAP ? (uint32_t)hk.bail_cap : EV_BAIL_CAP;
  r.bail_word = Q_BAIL;
  r.chunk = EV_CHUNK;
  if (ff) {
    // fault-free single-proposer batches (configs 1, 2) run one instance per
    // lane on paxos_ff1_kernel, the other fault-free batches (duelling
    // proposers, log mode) on paxos_ffp_kernel; either's (never expected)
    // bails on the general faulty kernel.  PXB_NO_FF1=1 / PXB_NO_FFP=1 turn
    // one off; with neither, the general fault-free kernel runs the chunk
    const bool ff1 = !r.logm && P == 1 && !hk.no_ff1;
    r.kind = ff1 ? ROUTE_FF1 : !hk.no_ffp ? ROUTE_FFP : ROUTE_GENERAL;
    r.ff = r.kind == ROUTE_GENERAL;
    return r;
  }
  // faulty batches run on the per-lane kernel (paxos_ev.h), its bailed
  // instances on the general faulty kernel.  Per-lane beats the general
  // kernel on every topology, even where its layout fits 3 waves per CU
  // (MI355X, 2^22 instances, ms: config 5 148 vs 247; P = 3, N = 9 with delays
  // to 12: 347 vs 689; P = 2, N = 9, delays to 12: 97 vs 247).
  // PXB_NO_EV=1 forces the general kernel.
  if (!ev::eligible(c) || hk.no_ev) return r;       // (ROUTE_GENERAL)
  r.kind = ROUTE_EV;
  const int layout = ev::layout_for(c);
  const bool small_log = layout == 4 && P * N <= 10;
  // Faulty log mode over <= 10 links with delays <= 4 runs layout 9 where it
  // would run layout 4: its reply seqs as bytes in registers, the 4-step wheel
  // and its canonical log packed (14 words), the same 19-word pool: 75 LDS
  // words, 8 waves per CU instead of 7 (residency sweep, faulty log mode at
  // 2^22, PXB_BLOCKS_PER_CU 5 / 6 / 7: 32.7 / 29.6 / 27.5 ms; layout 9: 2^22
  // +5.6 %, 2^20 +2.5 %, profiles/r06_notes/ab_lg_layout9.txt).
  // PXB_NO_LGS=1 keeps layout 4.
  const int log_layout = (small_log && c->delay_max <= 4 && !hk.no_lgs) ? 9 : layout;
  r.second = RouteStage{P, log_layout};
  // the first stage's list holds a large share of the chunk (see EV_SPLIT_CAP)
  const uint32_t big_cap = r.cap == EV_BAIL_CAP ? EV_SPLIT_CAP : r.cap;
  if ((c->flags & PXB_CFG_RANDOMIZE) && P == 3 && !hk.no_split) {
    // Split routing of fuzzed three-proposer batches (config 5): the
    // two-proposer shape's layout fits more waves (config 5: 6 vs 4 per CU), so
    // it runs first, over the chunk, and lists the instances that drew P = 3
    // (bailed at init) for the three-proposer shape, whose own bails go to the
    // general kernel.  PXB_NO_SPLIT=1 turns it off.
    // (It comes before the log-mode routing below: a third of the chunk goes
    // through the list, so the chunk and the list must be the split's.)
    r.two_stage = TWO_SPLIT;
    r.first = RouteStage{2, layout};
    r.conditional = true;
    r.chunk = EV_SPLIT_CHUNK;
  } else if (layout == 6 && P == 2 && N >= 6 && N <= 7 && !hk.no_tight) {
    // Tight routing of two-proposer simple schedules whose layout-6 lane takes
    // more than 52 LDS words (config 4: 60 words, 10 waves per CU, so half the
    // SIMDs run 2 waves and half 3): layout 7 (52 words, 12 waves per CU)
    // runs over the chunk first and lists its bails (config 4: 0.5 %, nearly all
    // a full 3-deep response FIFO) for layout 6 over that list, whose own bails
    // go to the general kernel.  PXB_NO_TIGHT=1 turns it off.
    // Only where its hand-off rate is measured small: N = 6, 7 (host model,
    // tools/wave_model.cpp NACC=6/7/8 TIGHT=1 on config 4's schedule: 0.11 %,
    // 0.76 %, 2.8 %; at N = 8 the tight lane has 53 words, so it would not reach
    // 12 waves per CU anyway, and its 21-word pool serves 16 response links).
    // A list that overflowed (above a quarter of the chunk) would have the
    // general kernel re-run the whole chunk: exact, but slow.
    // (bails are rare, so whole chunks)
    r.two_stage = TWO_TIGHT;
    r.first = RouteStage{2, 7};
    r.conditional = true;
  } else if (small_log && !hk.no_lg2) {
    // Two-stage faulty log mode over <= 10 links: the log-mode shape (layout 4
    // or 9, a 19-word response pool: 86 words, 7 waves per CU) over the chunk,
    // the same shape on the 16-step wheel with a 32-word pool (layout 8) over
    // what it hands on (pool overflows: none in 4 million instances of
    // extra.log_mode_faulty, host model; 2 per million with an 18-word pool),
    // the general log-mode kernel over that one's.  A handed-on instance is one
    // of the longest; on the general kernel it held a 2^20-instance call 4-5 ms
    // and a 2^22 one up to 22 ms after the per-lane kernel, on layout 8 0.9-6 ms
    // (kernel traces, profiles/r06_notes/lg_kernel_trace.txt,
    // lg2_kernel_trace_2p20.txt).  PXB_NO_LG2=1 turns it off.
    r.two_stage = TWO_LG2;
    r.first = r.second;
    r.second = RouteStage{P, 8};
  }
  if (r.two_stage != TWO_NONE) {
    r.first_cap = big_cap;
    r.bail_word = Q_BAIL2;
  }
  return r;
}

// The plan to launch, given the blocks per CU that fit of its first and second
// stage's kernels: a conditional two-stage routing whose first stage fits no
// more than its second runs the second over whole EV_CHUNK chunks instead
inline RoutePlan route_resolve(RoutePlan r, int occ_first, int occ_second) {
  if (r.two_stage != TWO_NONE && r.conditional && !(occ_first > occ_second)) {
    r.two_stage = TWO_NONE;
    r.chunk = EV_CHUNK;
    r.first_cap = r.cap;
    r.bail_word = Q_BAIL;
  }
  return r;
}

// Instances per chunk.  `resident` blocks of the general kernel, `wpb` waves
// each, `group` instances per wave.  A launch must not give any slot 65536
// instances (16-bit packed run totals): on average 30000 per slot for the
// block-queue kernels (uniform instance lengths), 60000 for the work-queue
// kernels (which also flush mid-run); epoch tags (idx + 1 under the work queue)
// stay below 2^30.  Per-lane chunks are bounded by the bailed-id lists.
inline uint64_t route_chunk_max(const RoutePlan& r, uint64_t resident, uint64_t wpb, uint64_t group) {
  auto lower = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  if (r.kind == ROUTE_EV) return r.chunk;
  // fault-free log mode: 16-bit epochs, so every block's range (static slices:
  // every wave's) stays below 2^16 instances
  if (r.kind == ROUTE_GENERAL && r.ff)
    return r.logm ? lower(resident * wpb * group * 30000ull, resident * 60000ull)
                  : lower(1ull << 31, resident * wpb * group * 30000ull);
  // (fault-free per-lane kernels too: as few launches as the general faulty
  // kernel allows -- it may have to re-run a whole chunk; A/B on config 2 at
  // 2^26: 2^24-instance launches 2 % slower, 2^22 10 %, 2^20 33 %)
  return lower((1ull << 30) - 1, resident * wpb * group * 60000ull);
}

}  // namespace pxb
