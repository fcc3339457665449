// ev_valu_host.cpp — TEST ONLY: runs the per-lane kernel's state machine
// (cloud-haskell-paxos_amd/csrc/paxos_ev.h) on the host, one listed instance
// at a time, and watches the acceptor registers from outside
// (tests/test_ev_valu_forms.py): which acceptor index a request changed the
// ticket or the stored ticket of (it answered that request) and which one's
// log grew (it took an Execute), so that the test can tell that the selects
// over the acceptor arrays were exercised at every index.  Also runs the
// kernel driver's packed 0 / 1 sums (paxos_ev_kernel.h EvFlagSums) beside
// plain sums.  Nothing here is linked into libpaxos_batch.so.
#include <stdint.h>
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

// one record per instance: VW_N words, then the N log digests
enum {
  VW_RES = 0,        // 4 words: pxb_result
  VW_ROUNDS = 4,
  VW_EXECS,
  VW_MSGS,
  VW_CANON,
  VW_BAILED,         // 1: handed on (no outputs)
  VW_FLAGS,          // EvOut.flags
  VW_STEPS,          // EvOut.steps
  VW_ANSWERED,       // bit a: a request changed acceptor a's ticket or stored ticket (granted or accepted)
  VW_EXECUTED,       // bit a: acceptor a's log grew (an Execute at its ticket)
  VW_OTHERS,         // iterations in which more than one acceptor's registers changed (never)
  VW_GID,            // the lane's own index of the instance (gid_of)
  VW_N
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
    uint32_t* r = rec + (size_t)i * (VW_N + N);
    memset(r, 0, sizeof(uint32_t) * (VW_N + N));
    L.bailed = false;
    L.init(p, ids[i]);
    r[VW_GID] = L.gid_of(p);
    if (L.bailed) {
      r[VW_BAILED] = 1u;
      continue;
    }
    EvOut o{};
    uint64_t guard = 0;
    for (;;) {
      uint32_t tick0[N], len0[N];
      for (int a = 0; a < N; ++a) tick0[a] = L.accw[a] & 0xFFFFFFu, len0[a] = L.log_len_of(a);
      const bool done = L.step(p, o);
      if (++guard > 100000ull * cfg->step_cap) return -100;
      if (L.bailed) {
        r[VW_BAILED] = 1u;
        break;
      }
      uint32_t changed = 0u;
      for (int a = 0; a < N; ++a) {
        const bool ex = L.log_len_of(a) != len0[a];
        const bool tk = (L.accw[a] & 0xFFFFFFu) != tick0[a];
        r[VW_EXECUTED] |= ex ? 1u << a : 0u;
        r[VW_ANSWERED] |= (tk && !ex) ? 1u << a : 0u;
        changed += (ex || tk) ? 1u : 0u;
      }
      r[VW_OTHERS] += changed > 1u ? 1u : 0u;          // (one acceptor op per iteration)
      if (done) {
        memcpy(r + VW_RES, o.res, 16);
        r[VW_ROUNDS] = L.rounds;
        r[VW_EXECS] = L.execs;
        r[VW_MSGS] = L.msgs_sent();
        r[VW_CANON] = L.canon;
        r[VW_FLAGS] = o.flags;
        r[VW_STEPS] = o.steps;
        for (int a = 0; a < N; ++a) r[VW_N + a] = L.digest_of(a);
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

template <bool LG>
void flag_sums(uint32_t n, uint32_t flags, uint32_t* out) {
  EvFlagSums<LG> s;
  s.clear();
  for (uint32_t i = 0; i < n; ++i) s.add(flags);
  for (int k = 0; k < 7; ++k) out[k] = s.get(k);
  out[7] = s.instances();
  out[8] = (uint32_t)EvFlagSums<LG>::NW;
}

}  // namespace

// The listed instances (ids relative to cfg->first_instance) on the shape
// (layout, pm proposers, cfg->n_acceptors); rec: n_ids records of VW_N +
// n_acceptors words.  -1: not one of the shapes built here.
extern "C" int ev_valu_run(const pxb_config* cfg, int layout, uint32_t pm, const uint32_t* ids, uint32_t n_ids,
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
  SHAPE(0, 1, 1)   // one proposer, one acceptor: arrays of one element
  SHAPE(0, 1, 2)   // one proposer, two acceptors
  SHAPE(6, 1, 2)   // the same on the simple schedule
#undef SHAPE
  return -1;
}

extern "C" int ev_valu_words(void) { return VW_N; }

// n finished instances, each with the PXB_F_* flags `flags`, into the packed
// sums (log: the log-mode form, with the log-trunc field); out[0 .. 6]: the
// sums in tot_slot order, out[7]: instances(), out[8]: the words used
extern "C" void ev_valu_flag_sums(int log, uint32_t n, uint32_t flags, uint32_t* out) {
  if (log) flag_sums<true>(n, flags, out);
  else flag_sums<false>(n, flags, out);
}

// mixed: instance i has the flags fl[i]
extern "C" void ev_valu_flag_sums_list(int log, const uint32_t* fl, uint32_t n, uint32_t* out) {
  EvFlagSums<true> a;
  EvFlagSums<false> b;
  a.clear();
  b.clear();
  for (uint32_t i = 0; i < n; ++i) a.add(fl[i]), b.add(fl[i]);
  for (int k = 0; k < 7; ++k) out[k] = log ? a.get(k) : b.get(k);
}

extern "C" uint32_t ev_valu_flush_bound(void) { return EV_FLUSH; }
