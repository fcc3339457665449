// trace_host.cpp — TEST ONLY: the batched trace's per-lane core
// (cloud-haskell-paxos_amd/csrc/paxos_trace_core.h: TraceLane and trace_record)
// over the per-lane state machine (paxos_ev.h) on the host, one instance at a
// time, so tests/test_trace_batch_host.py can diff its records against the
// Python reference model step by step without a GPU.  The product runs the
// same code on the device (paxos_trace_batch.hip); nothing here is linked into
// libpaxos_batch.so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/paxos_ev_kernel.h"
#include "../../cloud-haskell-paxos_amd/csrc/paxos_trace_core.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

namespace {

struct Args {
  const pxb_config* cfg;
  uint64_t id;
  uint32_t smin, smax, tail;
  pxb_trace_step* records;
  uint64_t capacity;
  uint32_t* n_window;
  uint32_t* n_kept;
  uint32_t* status;
  pxb_result* result;
};

// Instance `a.id` as paxos_trace_batch_kernel runs it (TrbParams over one id):
// the count pass, then (records kept and room for some) the write pass from
// offset 0
template <int PM, int N, int W, bool EARLY, bool LG>
int run_shape(const Args& a) {
  constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using Lane = EvLane<PM, N, POOL, W, false, HostMem, EARLY, LG>;
  const uint64_t offset0 = 0u;
  TrbParams k{};
  k.p = make_params(a.cfg);
  k.p.first_instance = 0;
  k.ids = &a.id;
  k.count = 1u;
  k.smin = a.smin, k.smax = a.smax, k.tail = a.tail;
  k.cnt = a.n_window;
  k.offsets = &offset0;
  k.capacity = a.capacity;
  k.status = a.status;
  k.res = reinterpret_cast<uint4*>(a.result);
  HostLane<Lane> H(k.p);
  TraceLane<Lane> T;
  if (!host_run(k, H.L, T, 0u, a.cfg->step_cap)) return -100;
  k.finish(H.L, T, 0u);
  // (the scan's part: what the selection keeps of the instance's count)
  const uint32_t kept = trace_kept(*a.n_window, a.tail);
  *a.n_kept = kept;
  if (kept == 0u || a.capacity == 0u || !a.records) return 0;
  std::fill(H.buf.begin(), H.buf.end(), 0xDEADBEEFu);
  k.out = a.records;
  if (!host_run(k, H.L, T, 0u, a.cfg->step_cap)) return -100;
  k.finish(H.L, T, 0u);
  return 0;
}

#ifdef PXB_TRACE_HOST_MAIN
// (the sanitizer build: one shape, config 3's)
int dispatch(const Args& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 2 || c->n_acceptors != 5 || wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return (c->flags & PXB_CFG_TRACE_PRODUCTION) ? run_shape<2, 5, 8, true, false>(a) : run_shape<2, 5, 8, false, false>(a);
}
#else
// (the shapes of lane_shapes.h; -1: none)
struct Run {
  const Args& a;
  template <int PM, int N, int W, bool LG>
  int run() const {
    return (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) ? run_shape<PM, N, W, true, LG>(a) : run_shape<PM, N, W, false, LG>(a);
  }
};
int dispatch(const Args& a) { return host_lane_shape(a.cfg, Run{a}, -1); }
#endif

}  // namespace

// One instance as the batched trace runs it.  records holds `capacity` entries
// (nothing at or past them is written); *n_window = its visited steps inside the
// window, *n_kept = those the tail keeps (what its d_offsets entry grows by).
extern "C" int trace_host_run(const pxb_config* cfg, uint64_t id, const pxb_trace_sel* sel, pxb_trace_step* records,
                              uint64_t capacity, uint32_t* n_window, uint32_t* n_kept, uint32_t* status,
                              pxb_result* result) {
  if (!cfg || !trace_config_ok(cfg) || (sel && sel->reserved)) return -1;
  Args a{cfg, id, sel ? sel->step_min : 0u, sel ? sel->step_max : 0xFFFFFFFFu, sel ? sel->tail : 0u,
         records, capacity, n_window, n_kept, status, result};
  return dispatch(a);
}

#ifdef PXB_TRACE_HOST_MAIN
// Sanitizer-build driver (tests/test_trace_batch_host.py): instances first ..
// first + n - 1 of config 3's shape with one selection, every record buffer
// sized exactly (so that the sanitizer sees a write past it), to a file of raw
// little-endian words per instance: n_window, n_kept, status, result x 4, then
// the written records.
// argv: out seed first n loss delay skew cap flags step_min step_max tail capacity
int main(int argc, char** argv) {
  if (argc != 14) {
    fprintf(stderr, "usage: %s out seed first n loss delay skew cap flags step_min step_max tail capacity\n", argv[0]);
    return 2;
  }
  pxb_config c{};
  c.seed = strtoull(argv[2], nullptr, 0);
  const uint64_t first = strtoull(argv[3], nullptr, 0), n = strtoull(argv[4], nullptr, 0);
  c.n_proposers = 2;
  c.n_acceptors = 5;
  c.n_ticks = 1;
  c.tick_period = 1;
  c.crash_len_max = 1;
  uint32_t* f[] = {&c.loss_ppm, &c.delay_max, &c.skew_max, &c.step_cap, &c.flags};
  for (int i = 0; i < 5; ++i) *f[i] = (uint32_t)strtoul(argv[5 + i], nullptr, 0);
  pxb_trace_sel sel{(uint32_t)strtoul(argv[10], nullptr, 0), (uint32_t)strtoul(argv[11], nullptr, 0),
                    (uint32_t)strtoul(argv[12], nullptr, 0), 0u};
  const uint64_t capacity = strtoull(argv[13], nullptr, 0);
  FILE* o = fopen(argv[1], "wb");
  if (!o) return 3;
  for (uint64_t g = 0; g < n; ++g) {
    std::vector<pxb_trace_step> rec(capacity);               // exactly `capacity` entries
    uint32_t hdr[7] = {0, 0, 0, 0, 0, 0, 0};
    const int rc = trace_host_run(&c, first + g, &sel, rec.data(), capacity, &hdr[0], &hdr[1], &hdr[2],
                                  reinterpret_cast<pxb_result*>(&hdr[3]));
    if (rc != 0) {
      fclose(o);
      return 4;
    }
    const uint64_t m = hdr[1] < capacity ? hdr[1] : capacity;
    fwrite(hdr, 4, 7, o);
    fwrite(rec.data(), sizeof(pxb_trace_step), m, o);
  }
  fclose(o);
  return 0;
}
#endif
