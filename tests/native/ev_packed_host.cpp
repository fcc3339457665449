// ev_packed_host.cpp — TEST ONLY: runs the per-lane kernel's state machine
// (cloud-haskell-paxos_amd/csrc/paxos_ev.h) on the host as ev_host.cpp does,
// and watches the packed per-proposer state from outside while it runs
// (tests/test_ev_packed_state.py): the pending-broadcast queue around every
// insert, the broadcast counters' 16-bit fields, the ring index.  Nothing here
// is linked into libpaxos_batch.so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

// stats words (uint64 each)
enum {
  ST_INS2_LEN0 = 0,   // two-broadcast inserts (Execute + restart) into a queue of 0, 1, 2 entries
  ST_INS2_LEN1,
  ST_INS2_LEN2,
  ST_MAX_BCAST,       // most broadcasts one proposer of one finished instance made
  ST_OVER_256,        // finished instances with a proposer above 256 broadcasts
  ST_BAD_QUEUE,       // steps after which the pending queue was not what its inserts and pops make it
  ST_BAD_COUNT,       // finished instances whose counters disagree (queued != sent)
  ST_PACKED,          // 1: the shape packs its counters
  ST_RING_SLOTS,      // the shape's ring slots per proposer
  ST_N
};

template <int PM, int N, int W, bool CMP, bool LG, bool SL, int SP>
int run_shape(const pxb_config* cfg, pxb_result* out, uint32_t* dig, pxb_acceptor_rec* acc, int64_t* tot,
              uint32_t* bail_ids, uint32_t* n_bail, uint64_t* st) {
  constexpr int POOL = EvPool<PM, N, CMP, LG, SL, SP, W>::value;
  using S = Shape<PM, N, POOL, W, CMP, LG, SL, SP>;
  using Lane = EvLane<PM, N, POOL, W, CMP, HostMem, true, LG, SL, SP>;
  std::vector<uint32_t> buf(S::WORDS + 1, 0xDEADBEEFu);
  const EvParams p = make_params(cfg);
  Lane L;
  L.m = HostMem{buf.data()};
  L.set_keys(p);
  st[ST_PACKED] = Lane::CPK ? 1u : 0u;
  st[ST_RING_SLOTS] = S::BR;
  uint32_t nb = 0;
  for (uint32_t g = 0; g < (uint32_t)cfg->n_instances; ++g) {
    L.init(p, g);
    EvOut o;
    uint64_t guard = 0;
    if (L.bailed) {
      bail_ids[nb++] = g;
      continue;
    }
    for (;;) {
      const uint32_t pq0 = L.pq, len0 = L.pq_len, rounds0 = L.rounds, execs0 = L.execs;
      const bool done = L.step(p, o);
      if (++guard > 100000ull * cfg->step_cap) return -100;
      if (L.bailed) {
        bail_ids[nb++] = g;
        break;
      }
      // ---- the pending queue after the step: 5-bit entries (q << 3 | slot),
      // nothing above its length; what was queued before, less the broadcasts
      // whose last copy went, plus what the proposer op queued ----
      bool bad = L.pq_len > PQ_CAP || (L.pq_len < 6u && (L.pq >> (5u * L.pq_len)) != 0u);
      const bool two = L.execs == execs0 + 1u && L.rounds == rounds0 + 1u;   // Execute + restart: one handler
      if (two) {
        if (len0 > 2u) bad = true;
        else st[ST_INS2_LEN0 + len0] += 1;
        const uint32_t pops = len0 + 2u - L.pq_len;                          // (a send per copy slot: <= 2)
        if (pops > 2u || L.pq_len < 2u) {
          bad = true;
        } else {
          const uint32_t kept = L.pq_len - 2u;                               // entries from before the step
          const uint32_t e0 = (L.pq >> (5u * kept)) & 31u, e1 = (L.pq >> (5u * kept + 5u)) & 31u;
          const uint32_t q = e0 >> 3;
          bad |= q >= (uint32_t)PM || (e1 >> 3) != q || (e0 & 7u) >= S::BR ||
                 (e1 & 7u) != (((e0 & 7u) + 1u) & (S::BR - 1u));
          bad |= (L.pq & ((1u << (5u * kept)) - 1u)) != ((pq0 >> (5u * pops)) & ((1u << (5u * kept)) - 1u));
          if (q < (uint32_t)PM) bad |= L.p_state((int)q) != ROUND1;          // (restarted)
        }
      }
      st[ST_BAD_QUEUE] += bad ? 1u : 0u;
      if (done) {
        if (out) memcpy(&out[g], o.res, 16);
        for (int a = 0; a < N; ++a) {
          if (dig) dig[(uint64_t)g * N + a] = L.digest_of(a);
          if (acc) {
            uint32_t r[4];
            L.record_of(a, r);
            memcpy(&acc[(uint64_t)g * N + a], r, 16);
          }
        }
        // an ended instance has sent every broadcast it queued: both counters
        // agree, proposer by proposer, and sum to rounds + proposals + executes
        uint32_t sum = 0, mx = 0;
        for (uint32_t q = 0; q < (uint32_t)PM; ++q) {
          const uint32_t k = L.nsent_of(q);
          sum += k;
          mx = k > mx ? k : mx;
          if (L.bslot_of(q) != (k & (S::BR - 1u))) st[ST_BAD_COUNT] += 1;
        }
        if (L.pq_len != 0u || L.msgs_sent() != L.msgs + sum * (uint32_t)N || sum < L.rounds + L.execs)
          st[ST_BAD_COUNT] += 1;
        st[ST_MAX_BCAST] = mx > st[ST_MAX_BCAST] ? mx : st[ST_MAX_BCAST];
        st[ST_OVER_256] += mx > 256u ? 1u : 0u;
        const uint32_t f = o.flags;
        tot[PXB_C_INSTANCES] += 1;
        tot[PXB_C_DECIDED] += !(f & PXB_F_UNDECIDED);
        tot[PXB_C_UNDECIDED] += !!(f & PXB_F_UNDECIDED);
        tot[PXB_C_STUCK] += !!(f & PXB_F_STUCK);
        tot[PXB_C_PANIC] += !!(f & PXB_F_PANIC);
        tot[PXB_C_DIVERGENCE] += !!(f & PXB_F_LOG_DIVERGENCE);
        tot[PXB_C_STEP_CAP] += !!(f & PXB_F_STEP_CAP);
        tot[PXB_C_ROUNDS] += L.rounds;
        tot[PXB_C_STEPS] += o.steps;
        tot[PXB_C_MESSAGES] += L.msgs_sent();
        tot[PXB_C_EXECUTES] += L.execs;
        tot[PXB_C_LOG_TRUNC] += !!(f & PXB_F_LOG_TRUNC);
        tot[PXB_C_CANON_BYTES] += L.canon;
        break;
      }
    }
  }
  *n_bail = nb;
  return 0;
}

// a layout's template arguments, from the table
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

// One batch on the shape (layout, pm proposers, cfg->n_acceptors), outputs as
// ev_host_run's; stats: ST_N words.  -1: not one of the shapes built here.
extern "C" int ev_packed_run(const pxb_config* cfg, int layout, uint32_t pm, pxb_result* out, uint32_t* dig,
                             pxb_acceptor_rec* acc, int64_t* totals, uint32_t* bail_ids, uint32_t* n_bail,
                             uint64_t* stats) {
  if (!cfg || !eligible(cfg) || !layout_serves(layout, cfg)) return -1;
  if (pm > cfg->n_proposers || (pm < cfg->n_proposers && !(cfg->flags & PXB_CFG_RANDOMIZE))) return -1;
  memset(stats, 0, ST_N * sizeof(uint64_t));
#define SHAPE(ID, PMv, Nv)                                                                                   \
  if (layout == ID && pm == PMv && cfg->n_acceptors == Nv)                                                   \
    return run_shape<PMv, Nv, Row<ID>::W, Row<ID>::C, Row<ID>::L, Row<ID>::S, Row<ID>::SP>(cfg, out, dig, acc, \
                                                                                         totals, bail_ids, n_bail, stats);
  SHAPE(7, 2, 7)   // tight
  SHAPE(6, 2, 7)   // its second stage
  SHAPE(6, 1, 7)   // one proposer: the counters are the words themselves
  SHAPE(5, 2, 9)   // slim, two proposers
  SHAPE(5, 3, 9)   // slim, three proposers: a word per proposer
  SHAPE(4, 2, 5)   // log mode
  SHAPE(9, 2, 5)   // slim log mode, 4-step wheel
  SHAPE(0, 2, 7)   // 4-entry FIFOs, 16-bit reply seqs: long runs
  SHAPE(0, 3, 5)
#undef SHAPE
  return -1;
}
