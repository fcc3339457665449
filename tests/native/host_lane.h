// host_lane.h — TEST ONLY: what the host builds of the lane jobs ({trace,
// script, shrink, explore, events, cover, explore_cover, shrink_cover}_host.cpp)
// share: one lane's words behind a checked accessor, the guarded loop that
// stands where the kernels have the wave's (script_run), and the run of a
// functor at a config's shape (host_lane_shape: the mirror of lane_shapes.h's
// lane_kernel).  Around the loop trace_host.cpp calls the kernel's own
// TrbParams::begin / finish and shrink_host.cpp the kernel's own
// ShrParams::begin, over host pointers (host_run); the others spell their
// lane's text out, as their kernels do.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/paxos_trace_core.h"

#define PXB_HCHK(c)                                                                                       \
  do {                                                                                                   \
    if (!(c)) {                                                                                          \
      fprintf(stderr, "host lane: LDS access out of the shape's words: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
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

// A lane of the shape's words, filled with garbage (init must set what it reads), keys set
template <class Lane>
struct HostLane {
  std::vector<uint32_t> buf;
  Lane L;
  explicit HostLane(const pxb::ev::EvParams& p) : buf(Lane::S::WORDS, 0xDEADBEEFu) {
    L.m = HostMem{buf.data(), (uint32_t)Lane::S::WORDS};
    L.set_keys(p);
  }
};

// f.run<PM, N, W, LG>() at the config's shape (lane_shapes.h), or `none`
template <class F, class R, int PM>
struct HostLaneShape {
  const F& f;
  template <int N, int W, bool LG>
  R shape() const { return f.template run<PM, N, W, LG>(); }
};
template <class F, class R>
struct HostLaneProposers {
  const pxb_config* cfg;
  const F& f;
  R none;
  template <int PM>
  R proposers() const { return pxb::ev::lane_shape(cfg, HostLaneShape<F, R, PM>{f}, none); }
};
template <class F, class R>
R host_lane_shape(const pxb_config* cfg, const F& f, R none) {
  return pxb::ev::lane_proposers(cfg, HostLaneProposers<F, R>{cfg, f, none}, none);
}

// Job g as its kernel runs it up to k.finish, which the caller calls: k.begin
// (*started: its answer), then the started lane to its end.  False: the lane did
// not end (a hang is a test failure, not a hang).
template <class K, class Lane>
bool host_run(const K& k, Lane& L, pxb::ev::TraceLane<Lane>& T, uint64_t g, uint32_t step_cap, bool* started = nullptr) {
  bool run = k.begin(L, T, g);
  if (started) *started = run;
  const uint64_t guard_max = 100000ull * step_cap;
  for (uint64_t guard = 0; run;) {
    run = T.iter(L, k.p);
    if (run && ++guard > guard_max) return false;
  }
  return true;
}
