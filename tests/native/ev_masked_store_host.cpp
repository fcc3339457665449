// ev_masked_store_host.cpp — TEST ONLY, stand-alone: runs the per-lane kernel's
// state machine (cloud-haskell-paxos_amd/csrc/paxos_ev.h) on the host over a
// recording memory accessor that has the lane-masked stores (st_if, st16h_if,
// sth_if), one listed instance at a time (tests/test_ev_masked_store.py).
//
// The accessor checks every access against the shape's words, and
//   * that a masked store with a false predicate leaves memory as it was and
//     one with a true predicate leaves the value (RW_ERR_STORE);
//   * that no acceptor op takes a broadcast payload that was not written
//     since the instance started: the payload halfwords (words in log mode)
//     are the ones whose store-back, and the load that fed it, went
//     (RW_ERR_STALE);
// and counts the masked stores by region and predicate.
//
//   ev_masked_store_host run   <config hex> <layout> <pm> <id>...   one record line per id
//   ev_masked_store_host bails <config hex> <layout> <pm> <n>       the ids of 0 .. n-1 handed on
//
// <config hex>: the bytes of a pxb_config.  Nothing here is linked into
// libpaxos_batch.so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define PXB_EV_PROBES 1
#include "../../cloud-haskell-paxos_amd/csrc/paxos_ev_kernel.h"

namespace pxb { namespace ev { thread_local uint32_t ev_probe_bits = 0; } }

using namespace pxb;
using namespace pxb::ev;

namespace {

#define PXB_MCHK(c)                                                                          \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      fprintf(stderr, "masked-store host: access out of the shape's words: %s\n", #c);     \
      abort();                                                                              \
    }                                                                                       \
  } while (0)

enum { RG_REQ = 0, RG_RSP, RG_POOL, RG_BRING, RG_OTHER, RG_N };

// what the accessor has seen (shared by the copies the lane makes of it)
struct Rec {
  uint32_t n_words;
  uint32_t lo[RG_N], hi[RG_N];       // the regions' words [lo, hi)
  uint32_t st_true[RG_N], st_false[RG_N];
  uint32_t err_store;                // masked stores that left the wrong memory
  bool stale_read;                   // this iteration loaded an unwritten payload
  // (payloads are loaded as words in log mode and as halfwords otherwise; the
  // other kind of load in their region is a pool load at an unused entry's
  // index, whose value no lane uses)
  bool words;
  std::vector<uint8_t> valid;        // per halfword of the payload region: written since init
  int region(uint32_t word) const {
    for (int r = 0; r < RG_OTHER; ++r)
      if (word >= lo[r] && word < hi[r]) return r;
    return RG_OTHER;
  }
  void wrote(uint32_t hw, uint32_t n) {   // halfwords [hw, hw + n)
    for (uint32_t k = hw; k < hw + n; ++k)
      if (k >= 2u * lo[RG_BRING] && k < 2u * hi[RG_BRING]) valid[k - 2u * lo[RG_BRING]] = 1;
  }
  void read(uint32_t hw, uint32_t n) {
    for (uint32_t k = hw; k < hw + n; ++k)
      if (k >= 2u * lo[RG_BRING] && k < 2u * hi[RG_BRING] && !valid[k - 2u * lo[RG_BRING]]) stale_read = true;
  }
};

struct RecMem {
  uint32_t* w;
  Rec* r;
  uint16_t* h() const { return reinterpret_cast<uint16_t*>(w); }
  uint32_t ld(uint32_t i) const {
    PXB_MCHK(i < r->n_words);
    if (r->words) r->read(2u * i, 2u);
    return w[i];
  }
  void st(uint32_t i, uint32_t v) const { PXB_MCHK(i < r->n_words); r->wrote(2u * i, 2u); w[i] = v; }
  uint32_t ld16(uint32_t base, uint32_t i) const {
    PXB_MCHK(2u * base + i < 2u * r->n_words);
    if (!r->words) r->read(2u * base + i, 1u);
    return h()[2u * base + i];
  }
  void st16(uint32_t base, uint32_t i, uint32_t v) const {
    PXB_MCHK(2u * base + i < 2u * r->n_words);
    r->wrote(2u * base + i, 1u);
    h()[2u * base + i] = (uint16_t)v;
  }
  uint32_t ld16h(uint32_t i, uint32_t half) const { PXB_MCHK(half < 2u); return ld16(i, half); }
  void st16h(uint32_t i, uint32_t half, uint32_t v) const { PXB_MCHK(half < 2u); st16(i, half, v); }
  uint32_t ldh(uint32_t base, uint32_t i) const { return ld16(base, i); }
  void sth(uint32_t base, uint32_t i, uint32_t v) const { st16(base, i, v); }
  void orw(uint32_t i, uint32_t v) const { PXB_MCHK(i < r->n_words); w[i] |= v; }
  // ---- the lane-masked stores: checked against the memory before and after ----
  void count(uint32_t word, bool c) const { (c ? r->st_true : r->st_false)[r->region(word)] += 1u; }
  void st_if(uint32_t i, uint32_t v, bool c) const {
    PXB_MCHK(!c || i < r->n_words);              // (a lane that does not store may hold any address)
    const bool in = i < r->n_words;
    const uint32_t old = in ? w[i] : 0u;
    if (c) st(i, v);
    if (in && w[i] != (c ? v : old)) r->err_store += 1u;
    count(i, c);
  }
  void st16h_if(uint32_t i, uint32_t half, uint32_t v, bool c) const { sth_if(i, half, v, c); }
  void sth_if(uint32_t base, uint32_t i, uint32_t v, bool c) const {
    const uint32_t k = 2u * base + i;
    PXB_MCHK(!c || k < 2u * r->n_words);
    const bool in = k < 2u * r->n_words;
    const uint16_t old = in ? h()[k] : (uint16_t)0;
    if (c) st16(base, i, v);
    if (in && h()[k] != (c ? (uint16_t)v : old)) r->err_store += 1u;
    count(k >> 1, c);
  }
};

// one record per instance, RW_N words and then the N log digests
enum {
  RW_ID = 0,
  RW_RES = 1,        // 4 words: pxb_result
  RW_ROUNDS = 5,
  RW_EXECS,
  RW_MSGS,
  RW_CANON,
  RW_BAILED,         // 1: handed on (no outputs)
  RW_PROBES,         // OR of the probe bits of every iteration (handed on: of its last one)
  RW_ITERS,
  RW_FLAGS,
  RW_STEPS,
  RW_BC_NONE,        // iterations whose proposer op made no broadcast, one (p0), two (p0 and p1)
  RW_BC_ONE,
  RW_BC_TWO,
  RW_S1_REPLY,       // iterations whose first send was the acceptor's reply, a second copy, neither
  RW_S1_COPY,
  RW_S1_NONE,
  RW_ST_TRUE,        // RG_N words: masked stores with a true predicate, by region
  RW_ST_FALSE = RW_ST_TRUE + RG_N,
  RW_ERR_STORE = RW_ST_FALSE + RG_N,
  RW_ERR_STALE,      // acceptor ops that took a payload not written since init
  RW_N
};

template <int PM, int N, int W, bool CMP, bool LG, bool SL, int SP>
int run_shape(const pxb_config* cfg, const std::vector<uint32_t>& ids, bool bails_only) {
  constexpr int POOL = EvPool<PM, N, CMP, LG, SL, SP, W>::value;
  using S = Shape<PM, N, POOL, W, CMP, LG, SL, SP>;
  using Lane = EvLane<PM, N, POOL, W, CMP, RecMem, true, LG, SL, SP>;
  static_assert(mem_has_st_if<RecMem>::value, "the lane must use the accessor's masked stores");
  std::vector<uint32_t> buf(S::WORDS, 0xDEADBEEFu);
  Rec rec{};
  rec.n_words = S::WORDS;
  rec.words = LG;
  rec.lo[RG_REQ] = S::REQ, rec.hi[RG_REQ] = S::REQ + S::NLQ;
  rec.lo[RG_RSP] = S::RSP, rec.hi[RG_RSP] = S::RSP + (S::RH ? (S::NLQ + 1) / 2 : S::NLQ);
  rec.lo[RG_POOL] = S::POOLB, rec.hi[RG_POOL] = S::POOLW + POOL;
  rec.lo[RG_BRING] = S::BRING, rec.hi[RG_BRING] = S::CLOG;
  rec.valid.assign(2u * (rec.hi[RG_BRING] - rec.lo[RG_BRING]), 0);
  const EvParams p = make_params(cfg);
  Lane L;
  L.m = RecMem{buf.data(), &rec};
  L.set_keys(p);
  for (uint32_t g : ids) {
    std::vector<uint32_t> r(RW_N + N, 0u);
    r[RW_ID] = g;
    memset(rec.st_true, 0, sizeof rec.st_true);
    memset(rec.st_false, 0, sizeof rec.st_false);
    rec.err_store = 0u;
    std::fill(rec.valid.begin(), rec.valid.end(), 0);
    L.bailed = false;
    L.init(p, g);
    bool ended = L.bailed;                           // (a fuzzed P above the shape's)
    r[RW_BAILED] = L.bailed ? 1u : 0u;
    EvOut o{};
    for (uint64_t guard = 0; !ended;) {
      const uint32_t msgs0 = L.msgs;
      ev_probe_bits = 0;
      rec.stale_read = false;
      const bool done = L.step(p, o);
      r[RW_ITERS] += 1u;
      if (++guard > 100000ull * cfg->step_cap) return 3;
      const uint32_t pb = ev_probe_bits;
      r[RW_ERR_STALE] += ((pb & EVP_ACC) && rec.stale_read) ? 1u : 0u;
      r[(pb & EVP_RESTART) ? RW_BC_TWO : (pb & EVP_BCAST) ? RW_BC_ONE : RW_BC_NONE] += 1u;
      r[!(pb & EVP_SEND1) ? RW_S1_NONE : (L.msgs != msgs0) ? RW_S1_REPLY : RW_S1_COPY] += 1u;
      if (L.bailed) {
        r[RW_BAILED] = 1u;
        r[RW_PROBES] = pb;
        ended = true;
      } else {
        r[RW_PROBES] |= pb;
        if (done) {
          memcpy(&r[RW_RES], o.res, 16);
          r[RW_ROUNDS] = L.rounds;
          r[RW_EXECS] = L.execs;
          r[RW_MSGS] = L.msgs_sent();
          r[RW_CANON] = L.canon;
          r[RW_FLAGS] = o.flags;
          r[RW_STEPS] = o.steps;
          for (int a = 0; a < N; ++a) r[RW_N + a] = L.digest_of(a);
          ended = true;
        }
      }
    }
    for (int k = 0; k < RG_N; ++k) r[RW_ST_TRUE + k] = rec.st_true[k], r[RW_ST_FALSE + k] = rec.st_false[k];
    r[RW_ERR_STORE] = rec.err_store;
    if (bails_only) {
      if (r[RW_ERR_STORE] | r[RW_ERR_STALE]) return 4;
      if (r[RW_BAILED]) printf("%u\n", g);
    } else {
      for (size_t k = 0; k < r.size(); ++k) printf("%u%c", r[k], k + 1 == r.size() ? '\n' : ' ');
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

int run(const pxb_config* cfg, int layout, uint32_t pm, const std::vector<uint32_t>& ids, bool bails_only) {
  if (!eligible(cfg) || !layout_serves(layout, cfg)) return 2;
  if (pm > cfg->n_proposers || (pm < cfg->n_proposers && !(cfg->flags & PXB_CFG_RANDOMIZE))) return 2;
#define SHAPE(ID, PMv, Nv)                                                                                    \
  if (layout == ID && pm == PMv && cfg->n_acceptors == Nv)                                                    \
    return run_shape<PMv, Nv, Row<ID>::W, Row<ID>::C, Row<ID>::L, Row<ID>::S, Row<ID>::SP>(cfg, ids, bails_only);
  SHAPE(7, 2, 7)   // tight
  SHAPE(6, 2, 7)   // its second stage
  SHAPE(5, 2, 9)   // slim, two proposers
  SHAPE(5, 3, 9)   // slim, three proposers
  SHAPE(4, 2, 5)   // log mode
#undef SHAPE
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s run|bails <config hex> <layout> <pm> <id>... | <n>\n", argv[0]);
    return 2;
  }
  pxb_config cfg;
  if (strlen(argv[2]) != 2 * sizeof cfg) {
    fprintf(stderr, "config: %zu hex digits expected\n", 2 * sizeof cfg);
    return 2;
  }
  for (size_t i = 0; i < sizeof cfg; ++i) {
    unsigned b = 0;
    if (sscanf(argv[2] + 2 * i, "%2x", &b) != 1) return 2;
    reinterpret_cast<unsigned char*>(&cfg)[i] = (unsigned char)b;
  }
  const bool bails_only = strcmp(argv[1], "bails") == 0;
  std::vector<uint32_t> ids;
  if (bails_only) {
    const uint32_t n = (uint32_t)strtoul(argv[5], nullptr, 10);
    for (uint32_t g = 0; g < n; ++g) ids.push_back(g);
  } else {
    for (int i = 5; i < argc; ++i) ids.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
  }
  return run(&cfg, atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 10), ids, bails_only);
}
