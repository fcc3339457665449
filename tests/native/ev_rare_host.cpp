// ev_rare_host.cpp — TEST ONLY: runs the per-lane kernel's state machine
// (cloud-haskell-paxos_amd/csrc/paxos_ev.h) on the host, one listed instance
// at a time, and reports what the rarely-needed regions of an iteration leave
// behind (tests/test_ev_rare_paths.py): the per-instance results the Execute
// branch and finish() keep (decision, round and Execute counts, canonical
// bytes, the panic flag), the bail flag as seen from outside at the entry of
// every iteration, and which rare regions the instance went through (the
// header's host-only probes).  Nothing here is linked into libpaxos_batch.so.
#include <stdint.h>
#include <string.h>

#include <vector>

#define PXB_EV_PROBES 1
#include "../../cloud-haskell-paxos_amd/csrc/paxos_ev_kernel.h"

namespace pxb { namespace ev { thread_local uint32_t ev_probe_bits = 0; } }

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

// one record per instance: RW_N words, then the N log digests
enum {
  RW_RES = 0,        // 4 words: pxb_result
  RW_ROUNDS = 4,
  RW_EXECS,
  RW_MSGS,
  RW_CANON,
  RW_BAILED,         // 1: handed on (no outputs)
  RW_PROBES,         // OR of the probe bits of every iteration (a bailed instance: of its last one)
  RW_ITERS,          // iterations run
  RW_ENTRY_BAILED,   // iterations entered with the bail flag already set
  RW_FLAGS,          // EvOut.flags
  RW_STEPS,          // EvOut.steps
  RW_TWO_BCAST,      // handlers that queued two broadcasts (Execute + the restart's AskForTicket)
  RW_BAIL_AT_INIT,   // 1: bailed by init (a fuzzed P above the shape's)
  RW_N
};

template <int PM, int N, int W, bool CMP, bool LG, bool SL, int SP>
int run_shape(const pxb_config* cfg, const uint32_t* ids, uint32_t n_ids, uint32_t* rec) {
  constexpr int POOL = EvPool<PM, N, CMP, LG, SL, SP, W>::value;
  using S = Shape<PM, N, POOL, W, CMP, LG, SL, SP>;
  using Lane = EvLane<PM, N, POOL, W, CMP, HostMem, true, LG, SL, SP>;
  std::vector<uint32_t> buf(S::WORDS + 1, 0xDEADBEEFu);
  const EvParams p = make_params(cfg);
  Lane L;
  L.m = HostMem{buf.data()};
  L.set_keys(p);
  for (uint32_t i = 0; i < n_ids; ++i) {
    uint32_t* r = rec + (size_t)i * (RW_N + N);
    memset(r, 0, sizeof(uint32_t) * (RW_N + N));
    L.bailed = false;
    L.init(p, ids[i]);
    if (L.bailed) {
      r[RW_BAILED] = r[RW_BAIL_AT_INIT] = 1u;
      continue;
    }
    EvOut o{};
    uint64_t guard = 0;
    for (;;) {
      r[RW_ENTRY_BAILED] += L.bailed ? 1u : 0u;        // (seen from outside, before the iteration)
      const uint32_t rounds0 = L.rounds, execs0 = L.execs;
      ev_probe_bits = 0;
      const bool done = L.step(p, o);
      r[RW_ITERS] += 1u;
      if (++guard > 100000ull * cfg->step_cap) return -100;
      if (L.bailed) {
        r[RW_BAILED] = 1u;
        r[RW_PROBES] = ev_probe_bits;
        break;
      }
      r[RW_PROBES] |= ev_probe_bits;
      r[RW_TWO_BCAST] += (L.execs == execs0 + 1u && L.rounds == rounds0 + 1u) ? 1u : 0u;
      if (done) {
        memcpy(r + RW_RES, o.res, 16);
        r[RW_ROUNDS] = L.rounds;
        r[RW_EXECS] = L.execs;
        r[RW_MSGS] = L.msgs_sent();
        r[RW_CANON] = L.canon;
        r[RW_FLAGS] = o.flags;
        r[RW_STEPS] = o.steps;
        for (int a = 0; a < N; ++a) r[RW_N + a] = L.digest_of(a);
        break;
      }
    }
  }
  return 0;
}

template <int ID>
struct Row;
#define PXB_EV_ROW(ID, W_, C_, L_, S_, SP_, PART, BUILT) \
  template <>                                            \
  struct Row<ID> {                                       \
    static constexpr int W = W_, SP = SP_;               \
    static constexpr bool C = C_, L = L_, S = S_;        \
  };
PXB_EV_LAYOUTS(PXB_EV_ROW)
#undef PXB_EV_ROW

}  // namespace

// The listed instances (ids relative to cfg->first_instance) on the shape
// (layout, pm proposers, cfg->n_acceptors); rec: n_ids records of RW_N +
// n_acceptors words.  -1: not one of the shapes built here.
extern "C" int ev_rare_run(const pxb_config* cfg, int layout, uint32_t pm, const uint32_t* ids, uint32_t n_ids,
                           uint32_t* rec) {
  if (!cfg || !eligible(cfg) || !layout_serves(layout, cfg)) return -1;
  if (pm > cfg->n_proposers || (pm < cfg->n_proposers && !(cfg->flags & PXB_CFG_RANDOMIZE))) return -1;
#define SHAPE(ID, PMv, Nv)                                                                                    \
  if (layout == ID && pm == PMv && cfg->n_acceptors == Nv)                                                    \
    return run_shape<PMv, Nv, Row<ID>::W, Row<ID>::C, Row<ID>::L, Row<ID>::S, Row<ID>::SP>(cfg, ids, n_ids, rec);
  SHAPE(7, 2, 7)   // tight
  SHAPE(6, 2, 7)   // its second stage
  SHAPE(5, 2, 9)   // slim, two proposers
  SHAPE(5, 3, 9)   // slim, three proposers
  SHAPE(4, 2, 5)   // log mode
#undef SHAPE
  return -1;
}

extern "C" int ev_rare_words(void) { return RW_N; }
