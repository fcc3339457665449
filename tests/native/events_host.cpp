// events_host.cpp — TEST ONLY: the event lane (cloud-haskell-paxos_amd/csrc/
// events_core.h: EventDraws, EventLane over the scripted lane) and the reorder
// step (event_place) on the host, one row and one staged event at a time, so
// tests/test_events_host.py can check them against the reference model without a
// GPU.  The product runs the same code on the device (paxos_events.hip);
// nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/events_core.h"
#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

// the header's event is the 24 words the lane code writes
static_assert(offsetof(pxb_trace_event, actor) == 4 && offsetof(pxb_trace_event, index) == 5 &&
                  offsetof(pxb_trace_event, peer) == 6 && offsetof(pxb_trace_event, fate) == 7 &&
                  offsetof(pxb_trace_event, n_out) == 8 && offsetof(pxb_trace_event, reserved) == 12 &&
                  offsetof(pxb_trace_event, in) == 16 && offsetof(pxb_trace_event, out) == 32 &&
                  offsetof(pxb_trace_event, after) == 64 && alignof(pxb_trace_event) <= 16,
              "event fields");

namespace {

// one pass of one row: the count pass (out == nullptr), or the write pass to out
struct Args {
  const pxb_config* cfg;
  const uint8_t* row;
  uint32_t depth, smin, smax;
  uint32_t cnt;                     // write pass: the count pass's
  pxb_trace_event* out;
  uint64_t room;
  uint32_t* n;
  uint32_t* status;
  uint32_t* res;
};

// what one lane of paxos_events_kernel does for its row
template <int PM, int N, int W, bool LG>
int run_shape(const Args& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, EventDraws>::Lane;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  L.e_acc = L.e_pin = false;
  EventLane<Lane> E;
  E.begin_count(a.smin, a.smax);
  if (a.out) E.begin_write(a.smin, a.smax, a.cnt, a.out, a.room);
  const uint32_t st = script_begin(L, p, a.depth, a.row);
  if (st != PXB_TRACE_OK) {
    E.status = st;
  } else {
    const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
    uint64_t guard = 0;
    while (E.iter(L, p))
      if (++guard > guard_max) return -100;
  }
  if (a.n) *a.n = E.n;
  if (a.status) *a.status = E.status;
  if (a.res) memcpy(a.res, E.res, 16);
  return 0;
}

#ifdef PXB_EVENTS_HOST_MAIN
// (the sanitizer build: the shapes of the step KATs, N = 3 on the 8-step wheel)
int dispatch(const Args& a) {
  const pxb_config* c = a.cfg;
  if (c->n_acceptors != 3 || wheel_for(c->delay_max) != 8) return -1;
  if (c->n_ticks > 1) return c->n_proposers == 1 ? run_shape<1, 3, 8, true>(a) : -1;
  switch (c->n_proposers) {
    case 1: return run_shape<1, 3, 8, false>(a);
    case 2: return run_shape<2, 3, 8, false>(a);
    case 3: return run_shape<3, 3, 8, false>(a);
  }
  return -1;
}
#else
struct Run {
  const Args& a;
  template <int PM, int N, int W, bool LG>
  int run() const { return run_shape<PM, N, W, LG>(a); }
};
int dispatch(const Args& a) { return host_lane_shape(a.cfg, Run{a}, -1); }
#endif

}  // namespace

// pxb_trace_events as the device runs it, pass by pass: the count pass of every
// row, the exclusive sum, the write pass into a staging buffer of
// min(total, capacity + EVT_SEG_MAX) events, the reorder of every staged event.
// Return codes as the library's (PXB_E_INVAL for what it refuses), -100 a hang.
extern "C" int events_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                               const pxb_trace_sel* sel, pxb_trace_event* events, uint64_t capacity,
                               uint64_t* offsets, uint32_t* status, pxb_result* results, uint64_t* n_events) {
  if (!cfg || (count && !rows) || depth > PXB_SCRIPT_MAX_DEPTH || !trace_config_ok(cfg) || !offsets ||
      (sel && (sel->reserved || sel->tail)) || (!events && capacity) || (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return PXB_E_INVAL;
  const uint32_t smin = sel ? sel->step_min : 0u, smax = sel ? sel->step_max : 0xFFFFFFFFu;
  const uint64_t stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  std::vector<uint32_t> cnt(count);
  offsets[0] = 0;
  for (uint64_t i = 0; i < count; ++i) {
    uint32_t res[4];
    uint32_t st = 0;
    Args a{cfg, rows + i * stride, depth, smin, smax, 0u, nullptr, 0, &cnt[i], &st, res};
    if (int rc = dispatch(a)) return rc < -1 ? rc : PXB_E_INVAL;
    if (status) status[i] = st;
    if (results) memcpy(results + i, res, 16);
    offsets[i + 1] = offsets[i] + cnt[i];
  }
  const uint64_t total = offsets[count];
  if (n_events) *n_events = total;
  if (!capacity || !events || !count) return PXB_OK;
  const uint64_t room = capacity + EVT_SEG_MAX, staged = total < room ? total : room;
  std::vector<pxb_trace_event> staging(staged);           // exactly what the write pass may fill
  for (uint64_t i = 0; i < count; ++i) {
    if (cnt[i] == 0u || offsets[i] >= staged) continue;
    Args a{cfg, rows + i * stride, depth, smin, smax, cnt[i], staging.data() + offsets[i], staged - offsets[i],
           nullptr, nullptr, nullptr};
    if (int rc = dispatch(a)) return rc < -1 ? rc : PXB_E_INVAL;
  }
  for (uint64_t t = 0; t < staged; ++t) event_place(staging.data(), staged, offsets, count, t, events, capacity);
  return PXB_OK;
}

#ifdef PXB_EVENTS_HOST_MAIN
// Sanitizer-build driver (tests/test_events_host.py).  argv: in out.  The input
// file: a pxb_config, then little-endian uint32 depth, uint32 step_min, uint32
// step_max, uint64 count, uint64 capacity, then the rows.  Every buffer holds
// exactly what the call may write (so that the sanitizer sees a write past it).
// The output file: uint64 n_events, the offsets, the status words, the results,
// then the min(n_events, capacity) events.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  pxb_config c{};
  uint32_t h[3];
  uint64_t g[2];
  if (fread(&c, sizeof c, 1, f) != 1 || fread(h, 4, 3, f) != 3 || fread(g, 8, 2, f) != 2) return 3;
  const uint64_t count = g[0], capacity = g[1];
  if (count > (1u << 20) || capacity > (1u << 24) || h[0] > PXB_SCRIPT_MAX_DEPTH || c.n_proposers > 3 ||
      c.n_acceptors > 9)
    return 3;
  const uint64_t stride = script_stride(c.n_proposers, c.n_acceptors, h[0]);
  std::vector<uint8_t> rows(count * stride);
  if (count && fread(rows.data(), 1, rows.size(), f) != rows.size()) return 3;
  fclose(f);
  pxb_trace_sel sel{h[1], h[2], 0u, 0u};
  std::vector<uint64_t> offs(count + 1);
  std::vector<uint32_t> st(count);
  std::vector<pxb_result> res(count);
  uint64_t total = 0;
  // the sizing call, then the call with exactly min(total, capacity) events
  int rc = events_host_run(&c, rows.data(), count, h[0], &sel, nullptr, 0, offs.data(), st.data(), res.data(), &total);
  if (rc != 0) return 4;
  const uint64_t m = total < capacity ? total : capacity;
  std::vector<pxb_trace_event> ev(m);
  if (m) rc = events_host_run(&c, rows.data(), count, h[0], &sel, ev.data(), m, offs.data(), st.data(), res.data(), &total);
  if (rc != 0) return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  fwrite(&total, 8, 1, o);
  fwrite(offs.data(), 8, offs.size(), o);
  fwrite(st.data(), 4, st.size(), o);
  fwrite(res.data(), sizeof(pxb_result), res.size(), o);
  fwrite(ev.data(), sizeof(pxb_trace_event), ev.size(), o);
  fclose(o);
  return 0;
}
#endif
