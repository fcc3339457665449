// win_host.cpp — TEST ONLY: the window pre-pass's words (ev::crash_of and
// ev::window_word, what paxos_win.hip stores) against the windows that
// EvLane::init draws, on the host, and EvLane::init loading a pre-drawn row
// (tests/test_win_prepass.py).  Nothing here is linked into libpaxos_batch.so.
#include <stdint.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/paxos_ev_kernel.h"

using namespace pxb;
using namespace pxb::ev;

namespace {

struct HostMem {
  uint32_t* w;
  uint32_t ld(uint32_t i) const { return w[i]; }
  void st(uint32_t i, uint32_t v) const { w[i] = v; }
  uint32_t ld16(uint32_t base, uint32_t i) const { return reinterpret_cast<const uint16_t*>(w + base)[i]; }
  void st16(uint32_t base, uint32_t i, uint32_t v) const { reinterpret_cast<uint16_t*>(w + base)[i] = (uint16_t)v; }
  uint32_t ld16h(uint32_t i, uint32_t half) const { return reinterpret_cast<const uint16_t*>(w + i)[half]; }
  void st16h(uint32_t i, uint32_t half, uint32_t v) const { reinterpret_cast<uint16_t*>(w + i)[half] = (uint16_t)v; }
  uint32_t ldh(uint32_t base, uint32_t i) const { return ld16(base, i); }
  void sth(uint32_t base, uint32_t i, uint32_t v) const { st16(base, i, v); }
  void orw(uint32_t i, uint32_t v) const { w[i] |= v; }
};

// the generic layout (0) at three proposers: init keeps every fuzzed instance
template <int N>
int check_n(const pxb_config* cfg, uint32_t* rows, uint32_t* drawn) {
  constexpr int POOL = EvPool<3, N, false>::value;
  using S = Shape<3, N, POOL, 8, false>;
  std::vector<uint32_t> buf(S::WORDS + 1, 0xDEADBEEFu);
  const EvParams p = make_params(cfg);
  EvLane<3, N, POOL, 8, false, HostMem> L;
  L.m = HostMem{buf.data()};
  L.set_keys(p);
  const uint32_t n = (uint32_t)cfg->n_instances;
  for (uint32_t g = 0; g < n; ++g) {                     // the pre-pass, as paxos_win_kernel maps it
    uint32_t crash_m1;
    const bool crashy = crash_of(p, p.first_instance + g, crash_m1);
    for (uint32_t a = 0; a < (uint32_t)N; ++a) rows[(uint64_t)g * N + a] = window_word(p, p.first_instance + g, a, crashy, crash_m1);
  }
  int bad = 0;
  for (uint32_t g = 0; g < n; ++g) {
    L.init(p, g);                                        // draws
    for (int a = 0; a < N; ++a) {
      drawn[(uint64_t)g * N + a] = L.win[a];
      bad += L.win[a] != rows[(uint64_t)g * N + a];
    }
    const uint32_t P = L.P, dmax = L.dmax, loss_m1 = L.loss_m1;
    L.init(p, g, rows);                                  // loads row g
    for (int a = 0; a < N; ++a) bad += L.win[a] != rows[(uint64_t)g * N + a];
    bad += L.P != P || L.dmax != dmax || L.loss_m1 != loss_m1;
  }
  return bad;
}

}  // namespace

// rows, drawn: n_instances x n_acceptors words (the pre-pass's, init's own);
// returns the number of differing words (< 0: unsupported acceptor count)
extern "C" int win_host_check(const pxb_config* cfg, uint32_t* rows, uint32_t* drawn) {
  switch (cfg->n_acceptors) {
    case 2: return check_n<2>(cfg, rows, drawn);
    case 5: return check_n<5>(cfg, rows, drawn);
    case 7: return check_n<7>(cfg, rows, drawn);
    case 9: return check_n<9>(cfg, rows, drawn);
  }
  return -1;
}
