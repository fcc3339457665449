// paxos_trace_core.h — what the trace kernels share, as plain C++ over the
// per-lane state machine (paxos_ev.h): the record of one step (trace_record,
// used by pxb_trace_instance and pxb_trace_batch) and the per-lane core of the
// batched trace (TraceLane: one instance, one iteration at a time, counting or
// writing the records a selection keeps), and the form every lane kernel of
// the tool families has (the lane jobs: TrbParams::begin / finish here).  The
// host unit test
// (tests/native/trace_host.cpp) compiles the same code over a host accessor.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "paxos_ev.h"

namespace pxb {
namespace ev {

// proposer p's packed words (pw0, pw1, pw2: paxos_ev.h) as the record's pxb_trace_prop;
// from the words, so that a caller may select them by a per-lane index
template <class Lane>
__host__ __device__ __forceinline__ void trace_prop(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t p,
                                                    pxb_trace_prop& q) {
  q.ticket = (int32_t)Lane::w_ticket(w0);
  q.acks = Lane::w_acks(w0);
  q.state = Lane::w_state(w0);
  q.mr_t = (int32_t)Lane::w_mr_t(w0);
  q.pending = Lane::w_pending(w0);
  if constexpr (Lane::S::LG) {
    // log mode: 14-bit commands id [13:12] | t [11:0] (mr_v | r2_v << 14 in
    // pw1), the proposer's own command c<p+1>.<t> with t in pw2 (0: Nothing)
    const uint32_t mv = w1 & 0x3FFFu, rv = (w1 >> 14) & 0x3FFFu, ct = w2;
    q.cmd = ct ? ((p + 1u) << 24) | ct : 0u;
    q.mr_v = mv ? Lane::code_of(mv) : 0u;
    q.r2_v = rv ? Lane::code_of(rv) : 0u;
  } else {
    const uint32_t code = 1u;   // every command is c<id>.1 (docs/SEMANTICS.md §2)
    q.cmd = Lane::w_cmd(w1) ? ((Lane::w_cmd(w1) << 24) | code) : 0u;
    q.mr_v = Lane::w_mr_v(w1) ? ((Lane::w_mr_v(w1) << 24) | code) : 0u;
    q.r2_v = Lane::w_r2_v(w1) ? ((Lane::w_r2_v(w1) << 24) | code) : 0u;
  }
}

template <class Lane>
__host__ __device__ void trace_record(const Lane& L, uint32_t step, pxb_trace_step* r) {
  constexpr int PM = Lane::S::PM, N = Lane::S::N;
  constexpr bool EARLY = Lane::kEarly;
  r->step = step;
  // (production variant: copies of a broadcast still to send are not on the
  // links yet, so the count is not the oracle's end-of-step one)
  r->in_flight = (EARLY && L.pq_len != 0u) ? PXB_TRACE_IN_FLIGHT_UNKNOWN : L.links_in_flight();
  r->n_acceptors = N;
  r->n_proposers = L.P;
  for (int a = 0; a < PXB_MAX_ACCEPTORS; ++a) {
    uint32_t rec[4] = {0, 0, 0, 0};
    if (a < N) L.record_of(a, rec);
    r->acc[a].t_max = (int32_t)rec[0];
    r->acc[a].t_store = (int32_t)rec[1];
    r->acc[a].val = rec[2];
    r->acc[a].meta = rec[3];
    r->log_digest[a] = a < N ? L.digest_of(a) : 0u;
  }
  for (int p = 0; p < PXB_MAX_PROPOSERS; ++p) {
    pxb_trace_prop q = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p < PM && (uint32_t)p < L.P) trace_prop<Lane>(L.pw0[p], L.pw1[p], L.pw2[p], (uint32_t)p, q);
    r->prop[p] = q;
  }
}

// the records a selection keeps of `cnt` in-window ones: all, or the last `tail`
__host__ __device__ inline uint32_t trace_kept(uint32_t cnt, uint32_t tail) {
  return (tail != 0u && cnt > tail) ? tail : cnt;
}

// true when an iteration ended the instance at the step cap from a visited
// step s0 below its final step (s = step_cap - 1): the next message fell due
// past the cap.  The trace then records s0 and the final step, so that the step
// in which the final state was reached is told (o is set only when done).
__host__ __device__ __forceinline__ bool trace_cap_jump(bool done, const EvOut& o, int32_t s, int32_t s0) {
  return done && (o.flags & PXB_F_STEP_CAP) != 0u && s > s0;
}

// One instance of the batched trace on one lane.  The caller runs
//   begin_count / begin_write;  L.init(...);  while (T.iter(L, p)) {}
// (on the device with the wave's ballot as the loop's back edge).
//
// Count pass: runs the instance to its end; n = the visited steps inside
// [smin, smax], status and the result are the instance's.
// Write pass (the state machine is deterministic: the same steps again):
// in-window record j goes to out[j - skip] when j >= skip and j - skip < room
// (skip: the in-window records a tail drops; room: the caller's capacity left
// from this instance's offset), and the lane stops once no later record can be
// kept.
//
// The loop is paxos_trace_kernel's: a step is visited when the instance ended
// in it or the lane moved on to another; the production variant (EARLY) may
// record the step it ends in a second time (a carried step that held only lost
// copies ends at the step before it): that record is rewritten, counted once.
template <class Lane>
struct TraceLane {
  static constexpr bool EARLY = Lane::kEarly;
  static constexpr uint32_t NO_STEP = 0xFFFFFFFFu;   // (steps are < 4095)
  uint32_t smin, smax;
  uint32_t n;                       // in-window records so far
  uint32_t last_step;               // the last visited step (in the window or not)
  pxb_trace_step* out;              // write pass: this instance's first kept record (count pass: null)
  uint32_t skip, total;             // write pass: records the tail drops, the count pass's n
  uint64_t room;
  uint32_t status;
  uint32_t res[4];

  __host__ __device__ void begin_count(uint32_t step_min, uint32_t step_max) {
    smin = step_min;
    smax = step_max;
    n = 0u;
    last_step = NO_STEP;
    out = nullptr;
    skip = total = 0u;
    room = 0ull;
    status = PXB_TRACE_OK;
    res[0] = res[1] = res[2] = res[3] = 0u;
  }
  // cnt: the count pass's n of this instance (> 0), tail: the selection's, o:
  // where its first kept record goes, room_: records that fit from there (> 0)
  __host__ __device__ void begin_write(uint32_t step_min, uint32_t step_max, uint32_t cnt, uint32_t tail,
                                       pxb_trace_step* o, uint64_t room_) {
    begin_count(step_min, step_max);
    out = o;
    total = cnt;
    skip = cnt - trace_kept(cnt, tail);
    room = room_;
  }

  // a visited step's record: counted, and written where the selection keeps it;
  // false once the lane has nothing left to do (write pass only)
  __host__ __device__ __forceinline__ bool visit(const Lane& L, uint32_t step, bool again) {
    // write pass: a new record that is past the window, the count or the room: nothing later is kept
    if (out && !again && (n == total || step > smax || (n >= skip && (uint64_t)(n - skip) >= room))) return false;
    last_step = step;
    if (step >= smin && step <= smax) {
      const uint32_t j = again ? n - 1u : n;         // (again: the window held the first one too, n >= 1)
      if (out && j >= skip && (uint64_t)(j - skip) < room) trace_record(L, step, out + (j - skip));
      n = j + 1u;
      // (the default variant never rewrites: the last kept record ends the lane)
      if (!EARLY && out && n == total) return false;
    }
    return true;
  }

  // one iteration of the state machine; false once the lane has nothing left to do
  __host__ __device__ __forceinline__ bool iter(Lane& L, const EvParams& p) {
    const int32_t s0 = L.s;
    EvOut o;
    const bool done = L.step(p, o);
    if (L.bailed) {                 // beyond the link capacities: no records, a zeroed result
      status = PXB_TRACE_BAILED;
      n = 0u;
      return false;
    }
    if (done || L.s != s0) {
      // an instance that ends at the step cap ends from its last visited step,
      // s0, and its final step is step_cap - 1: both are recorded (the same state)
      if (trace_cap_jump(done, o, L.s, s0) && !visit(L, (uint32_t)s0, false)) return false;
      const uint32_t step = (uint32_t)(done ? L.s : s0);
      if (!visit(L, step, EARLY && done && last_step == step)) return false;
    }
    if (done) {
      res[0] = o.res[0];
      res[1] = o.res[1];
      res[2] = o.res[2];
      res[3] = o.res[3];
      return false;
    }
    return true;
  }
};

// four result words to an output: one 16-byte store on the device (hipMalloc'ed
// and checked by the entry points); on the host the caller's buffer, of which
// no alignment is known
__host__ __device__ __forceinline__ void store4(uint4* o, const uint32_t (&r)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  *o = make_uint4(r[0], r[1], r[2], r[3]);
#else
  memcpy(reinterpret_cast<unsigned char*>(o), r, 16);
#endif
}

// ---- the lane jobs ----
// Every lane kernel of the tool families (paxos_trace_batch_kernel,
// paxos_script_kernel, paxos_shrink_kernel, paxos_explore_kernel) is one shape:
//   L.m = its LDS words;  L.set_keys(k.p);
//   what job g is and how its lane starts  (-> run)
//   the wave's lanes to their ends under TraceLane
//   every store to the job's outputs
// with k the kernel's parameter struct.  Where it leaves the compiled kernel as
// it was, the text before and after the loop is a plain C++ member of that
// struct, begin(L, T, g) -> run and finish(L, T, g), which the host build of the
// lane (tests/native/*_host.cpp) runs over host pointers with its own guarded
// loop in between: both here, begin alone for the shrinker (shrink_core.h).
// The script and the explore kernels spell theirs out (DESIGN.md §3 has the
// register counts and timings that decided each).

// pxb_trace_batch: job i is ids[i]
struct TrbParams {
  EvParams p;
  const uint64_t* ids;
  uint64_t count;
  uint32_t smin, smax, tail;
  uint32_t* cnt;                    // in-window records per instance (count pass: out; write pass: in)
  const uint64_t* offsets;          // write pass: d_offsets
  pxb_trace_step* out;              // write pass: d_records (count pass: null)
  uint64_t capacity;
  uint32_t* status;                 // count pass, nullable
  uint4* res;                       // count pass, nullable

  // the count pass or the write pass of instance i (out: which); true: the lane runs
  template <class Lane>
  __host__ __device__ __forceinline__ bool begin(Lane& L, TraceLane<Lane>& T, uint64_t i) const {
    const bool write = out != nullptr;
    T.begin_count(smin, smax);
    bool run = i < count;
    if (run && write) {
      const uint32_t c = cnt[i];
      const uint64_t base = offsets[i];
      run = (c != 0u) & (base < capacity);
      if (run) T.begin_write(smin, smax, c, tail, out + base, capacity - base);
    }
    if (run) {
      EvParams pl = p;             // (the lane's own id: init takes first_instance + g)
      pl.first_instance = ids[i];
      L.init(pl, 0u);
    }
    return run;
  }
  template <class Lane>
  __host__ __device__ __forceinline__ void finish(const Lane&, const TraceLane<Lane>& T, uint64_t i) const {
    if (out == nullptr && i < count) {
      cnt[i] = T.n;
      if (status) status[i] = T.status;
      if (res) store4(res + i, T.res);
    }
  }
};

// the config checks of pxb_trace_instance (host side), shared by pxb_trace_batch
__host__ inline bool trace_config_ok(const pxb_config* cfg) {
  if (cfg->n_proposers < 1 || cfg->n_proposers > PXB_MAX_PROPOSERS || cfg->n_acceptors < PXB_MIN_ACCEPTORS ||
      cfg->n_acceptors > PXB_MAX_ACCEPTORS || cfg->delay_max < 1 || cfg->delay_max > PXB_MAX_DELAY ||
      cfg->step_cap < 1 || !eligible(cfg))
    return false;
  // log mode (n_ticks > 1): eligible() holds its delays to the 8-step wheel
  if (cfg->n_ticks > PXB_MAX_TICKS || (cfg->n_ticks > 1 && (cfg->tick_period < 1 || cfg->tick_period > PXB_MAX_STEP_CAP)))
    return false;
  return true;
}

}  // namespace ev
}  // namespace pxb
