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

#include "../../cloud-haskell-paxos_amd/csrc/paxos_ev_kernel.h"
#include "../../cloud-haskell-paxos_amd/csrc/paxos_trace_core.h"

using namespace pxb;
using namespace pxb::ev;

namespace {

#define PXB_HCHK(c)                                                                                        \
  do {                                                                                                   \
    if (!(c)) {                                                                                          \
      fprintf(stderr, "trace_host: LDS access out of the shape's words: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      abort();                                                                                           \
    }                                                                                                    \
  } while (0)
// one lane's words, every access checked against the shape's S::WORDS (as ev_host.cpp's checked accessor)
struct HostMem {
  uint32_t* w;
  uint32_t n;
  uint32_t ld(uint32_t i) const { PXB_HCHK(i < n); return w[i]; }
  void st(uint32_t i, uint32_t v) const { PXB_HCHK(i < n); w[i] = v; }
  uint32_t ld16(uint32_t base, uint32_t i) const {
    PXB_HCHK(2u * base + i < 2u * n);
    return reinterpret_cast<const uint16_t*>(w + base)[i];
  }
  void st16(uint32_t base, uint32_t i, uint32_t v) const {
    PXB_HCHK(2u * base + i < 2u * n);
    reinterpret_cast<uint16_t*>(w + base)[i] = (uint16_t)v;
  }
  uint32_t ld16h(uint32_t i, uint32_t half) const {
    PXB_HCHK(i < n && half < 2u);
    return reinterpret_cast<const uint16_t*>(w + i)[half];
  }
  void st16h(uint32_t i, uint32_t half, uint32_t v) const {
    PXB_HCHK(i < n && half < 2u);
    reinterpret_cast<uint16_t*>(w + i)[half] = (uint16_t)v;
  }
  uint32_t ldh(uint32_t base, uint32_t i) const { return ld16(base, i); }
  void sth(uint32_t base, uint32_t i, uint32_t v) const { st16(base, i, v); }
  void orw(uint32_t i, uint32_t v) const { PXB_HCHK(i < n); w[i] |= v; }
};

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

// what one lane of paxos_trace_batch_kernel does for its instance: the count
// pass, then (records kept and room for some) the write pass from offset 0
template <int PM, int N, int W, bool EARLY, bool LG>
int run_shape(const Args& a) {
  constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using S = Shape<PM, N, POOL, W, false, LG>;
  using Lane = EvLane<PM, N, POOL, W, false, HostMem, EARLY, LG>;
  std::vector<uint32_t> buf(S::WORDS, 0xDEADBEEFu);      // garbage: init must set what it reads
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  EvParams pl = p;
  pl.first_instance = a.id;
  Lane L;
  L.m = HostMem{buf.data(), (uint32_t)S::WORDS};
  L.set_keys(p);
  TraceLane<Lane> T;
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  uint64_t guard = 0;
  T.begin_count(a.smin, a.smax);
  L.init(pl, 0u);
  while (T.iter(L, p))
    if (++guard > guard_max) return -100;
  const uint32_t cnt = T.n, kept = trace_kept(cnt, a.tail);
  *a.n_window = cnt;
  *a.n_kept = kept;
  *a.status = T.status;
  memcpy(a.result, T.res, 16);
  if (kept == 0u || a.capacity == 0u || !a.records) return 0;
  std::fill(buf.begin(), buf.end(), 0xDEADBEEFu);
  T.begin_write(a.smin, a.smax, cnt, a.tail, a.records, a.capacity);
  L.init(pl, 0u);
  guard = 0;
  while (T.iter(L, p))
    if (++guard > guard_max) return -100;
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
template <int PM, int W, bool E, bool LG>
int run_n(const Args& a) {
  switch (a.cfg->n_acceptors) {
    case 2: return run_shape<PM, 2, W, E, LG>(a);
    case 3: return run_shape<PM, 3, W, E, LG>(a);
    case 4: return run_shape<PM, 4, W, E, LG>(a);
    case 5: return run_shape<PM, 5, W, E, LG>(a);
    case 6: return run_shape<PM, 6, W, E, LG>(a);
    case 7: return run_shape<PM, 7, W, E, LG>(a);
    case 8: return run_shape<PM, 8, W, E, LG>(a);
    case 9: return run_shape<PM, 9, W, E, LG>(a);
  }
  return -1;
}
template <int PM, bool E>
int run_w(const Args& a) {
  const int w = wheel_for(a.cfg->delay_max);
  if (a.cfg->n_ticks > 1) return w == 8 ? run_n<PM, 8, E, true>(a) : -1;
  return w == 8 ? run_n<PM, 8, E, false>(a) : run_n<PM, 16, E, false>(a);
}
template <bool E>
int run_p(const Args& a) {
  switch (a.cfg->n_proposers) {
    case 1: return run_w<1, E>(a);
    case 2: return run_w<2, E>(a);
    case 3: return run_w<3, E>(a);
  }
  return -1;
}
int dispatch(const Args& a) {
  return (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) ? run_p<true>(a) : run_p<false>(a);
}
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
