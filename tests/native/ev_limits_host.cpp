// ev_limits_host.cpp — TEST ONLY: runs the per-lane kernel's state machine
// (cloud-haskell-paxos_amd/csrc/paxos_ev.h) on the host, one listed instance
// at a time, at the limits of its packed fields (tests/test_ev_limits.py,
// tests/ev_limits.py): per instance the bail flag and the header's host-only
// probe bits (which limit handed it on), the outputs an instance that ends
// keeps, and the high-water mark of every narrow field, read after every
// iteration the lane keeps running after.  Nothing here is linked into
// libpaxos_batch.so.
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

// one record per instance: LW_N words, then the N log digests
enum {
  LW_RES = 0,        // 4 words: pxb_result
  LW_ROUNDS = 4,
  LW_EXECS,
  LW_MSGS,
  LW_CANON,
  LW_BAILED,         // 1: handed on (no outputs)
  LW_PROBES,         // OR of the probe bits of every iteration (a bailed instance: of its last one)
  LW_ITERS,          // iterations run
  LW_FLAGS,          // EvOut.flags
  LW_STEPS,          // EvOut.steps
  LW_BAIL_AT_INIT,   // 1: bailed by init
  // high-water marks over the iterations that did not bail
  LW_HW_TICKET,      // a proposer's ticket or mr_t (pw0 [11:0], [23:12]), an acceptor's t_max or t_store
  LW_HW_NSP,         // a proposer's sent-broadcast counter (nsp's field, or nsent[p])
  LW_HW_BCP,         // a proposer's queued-broadcast counter (bcp's field; three proposers: not kept, 0)
  LW_HW_ACKS,        // pw0 [27:24]
  LW_HW_REF,         // a ring slot's reference nibble
  LW_HW_LOG,         // an acceptor's log length
  LW_HW_RSEQ,        // a link's reply seq
  LW_N
};

template <class Lane>
void high_water(const Lane& L, uint32_t* r) {
  using S = typename Lane::S;
  auto up = [&](int k, uint32_t v) { r[k] = v > r[k] ? v : r[k]; };
  for (uint32_t q = 0; q < (uint32_t)S::PM; ++q) {
    up(LW_HW_TICKET, L.pw0[q] & 0xFFFu);
    up(LW_HW_TICKET, (L.pw0[q] >> 12) & 0xFFFu);
    up(LW_HW_ACKS, (L.pw0[q] >> 24) & 15u);
    up(LW_HW_NSP, L.nsent_of(q));
    if (Lane::CPK) up(LW_HW_BCP, S::PM == 1 ? L.bcp : (L.bcp >> Lane::fld_sh(q)) & 0xFFFFu);
    for (uint32_t k = 0; k < S::BR; ++k) up(LW_HW_REF, L.ref_nib(q, k));
  }
  for (uint32_t a = 0; a < (uint32_t)S::N; ++a) {
    up(LW_HW_TICKET, L.accw[a] & 0xFFFu);
    up(LW_HW_TICKET, (L.accw[a] >> 12) & 0xFFFu);
    up(LW_HW_LOG, (S::LG ? L.accv[S::LG ? a : 0] : L.accw[a]) >> Lane::A_LEN);
    for (uint32_t p = 0; p < (uint32_t)S::PM; ++p) {
      const uint32_t Lq = a * (uint32_t)S::PM + p;
      uint32_t k;
      if (S::CMP) k = L.m.ld(S::REQ + Lq) >> S::KSH;
      else if (S::SL) k = (L.rseqv[S::SL ? (Lane::RSA ? a : Lq >> 2) : 0] >> (8u * (Lane::RSA ? p : (Lq & 3u)))) & 0xFFu;
      else k = L.m.ld16(S::RSEQ, Lq);
      up(LW_HW_RSEQ, k);
    }
  }
}

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
    uint32_t* r = rec + (size_t)i * (LW_N + N);
    memset(r, 0, sizeof(uint32_t) * (LW_N + N));
    L.bailed = false;
    L.init(p, ids[i]);
    if (L.bailed) {
      r[LW_BAILED] = r[LW_BAIL_AT_INIT] = 1u;
      continue;
    }
    high_water(L, r);
    EvOut o{};
    uint64_t guard = 0;
    for (;;) {
      ev_probe_bits = 0;
      const bool done = L.step(p, o);
      r[LW_ITERS] += 1u;
      if (++guard > 100000ull * cfg->step_cap) return -100;
      if (L.bailed) {                                    // (its fields may be past their limits: not read)
        r[LW_BAILED] = 1u;
        r[LW_PROBES] = ev_probe_bits;
        break;
      }
      r[LW_PROBES] |= ev_probe_bits;
      high_water(L, r);
      if (done) {
        memcpy(r + LW_RES, o.res, 16);
        r[LW_ROUNDS] = L.rounds;
        r[LW_EXECS] = L.execs;
        r[LW_MSGS] = L.msgs_sent();
        r[LW_CANON] = L.canon;
        r[LW_FLAGS] = o.flags;
        r[LW_STEPS] = o.steps;
        for (int a = 0; a < N; ++a) r[LW_N + a] = L.digest_of(a);
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

// The shapes built here, X(layout, proposers, acceptors): those of the cells of
// tests/ev_limits.py (PXB_EV_LIMITS_SHAPES: another list, for a search by hand)
#ifndef PXB_EV_LIMITS_SHAPES
#define PXB_EV_LIMITS_SHAPES(X) \
  X(5, 3, 6)                    \
  X(9, 2, 5)                    \
  X(8, 2, 5)                    \
  X(9, 1, 5)                    \
  X(8, 1, 5)                    \
  X(0, 2, 5)                    \
  X(0, 2, 7)                    \
  X(0, 3, 9)                    \
  X(3, 3, 5)                    \
  X(7, 2, 7)                    \
  X(6, 2, 7)
#endif

// The listed instances (ids relative to cfg->first_instance) on the shape
// (layout, cfg->n_proposers, cfg->n_acceptors); rec: n_ids records of LW_N +
// n_acceptors words.  -1: not one of the shapes built here.
extern "C" int ev_limits_run(const pxb_config* cfg, int layout, const uint32_t* ids, uint32_t n_ids, uint32_t* rec) {
  if (!cfg || !eligible(cfg) || !layout_serves(layout, cfg)) return -1;
  if (cfg->flags & PXB_CFG_RANDOMIZE) return -1;
#define SHAPE(ID, PMv, Nv)                                                                                    \
  if (layout == ID && cfg->n_proposers == PMv && cfg->n_acceptors == Nv)                                      \
    return run_shape<PMv, Nv, Row<ID>::W, Row<ID>::C, Row<ID>::L, Row<ID>::S, Row<ID>::SP>(cfg, ids, n_ids, rec);
  PXB_EV_LIMITS_SHAPES(SHAPE)
#undef SHAPE
  return -1;
}

extern "C" int ev_limits_words(void) { return LW_N; }
