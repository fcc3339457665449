// shrink_host.cpp — TEST ONLY: the batched shrinker's shared logic
// (cloud-haskell-paxos_amd/csrc/shrink_core.h: ShrinkDraws and shrink_begin over
// the per-lane state machine, the per-entry fault test, the rank tables, select
// and settle, the signature) driven sequentially on the host, one parent and
// one candidate at a time, so tests/test_shrink_host.py can check it against
// pxb.shrink without a GPU.  The product runs the same code on the device
// (paxos_shrink.hip); nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/script_lane.h"
#include "../../cloud-haskell-paxos_amd/csrc/shrink_core.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

namespace {

// candidate `c` of a launch as paxos_shrink_kernel runs it
struct Cand {
  const pxb_config* cfg;
  const ShrParams* k;
  uint64_t c;
};

// ShrParams::begin is the kernel's own; the stores after the run are spelled out
// here as in the kernel (paxos_shrink.hip says why they are not shared)
template <int PM, int N, int W, bool LG>
int run_shape(const Cand& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ShrinkDraws>::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  const ShrParams& k = *a.k;
  HostLane<Lane> H(k.p);
  TraceLane<Lane> T;
  if (!host_run(k, H.L, T, a.c, a.cfg->step_cap)) return -100;
  uint16_t* const snt = k.csent + a.c * NL;
  if (T.status == PXB_TRACE_OK) script_sent(H.L, snt);
  else memset(snt, 0, NL * sizeof(uint16_t));
  k.held[a.c] = shrink_holds(T.status, T.res[3], snt, NL, k.depth, k.flag_mask) ? 1u : 0u;
  memcpy(reinterpret_cast<unsigned char*>(k.cres) + 16u * a.c, T.res, 16);
  return 0;
}

#ifdef PXB_SHRINK_HOST_MAIN
// (the sanitizer build: one shape, config 3's)
int dispatch(const Cand& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 2 || c->n_acceptors != 5 || wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return run_shape<2, 5, 8, false>(a);
}
#else
// (the shapes of lane_shapes.h; -1: none)
struct Run {
  const Cand& a;
  template <int PM, int N, int W, bool LG>
  int run() const { return run_shape<PM, N, W, LG>(a); }
};
int dispatch(const Cand& a) { return host_lane_shape(a.cfg, Run{a}, -1); }
#endif

// One launch of the candidate kernel over one parent: its candidates 0 .. n - 1.
// The launch has three parents, the row between two that have no candidate
// (offsets 0, 0, n, n), so that ShrParams::begin's search over the offsets runs.
struct Launch {
  std::vector<uint8_t> held;        // n
  std::vector<uint16_t> sent;       // n * 2 P N
  std::vector<uint32_t> res;        // n * 4
  int run(const pxb_config* cfg, const uint8_t* row, const uint16_t* table, uint32_t depth, uint32_t flag_mask,
          uint32_t n, bool prefix) {
    const ShrinkDims d{cfg->n_proposers, cfg->n_acceptors, depth, cfg->delay_max};
    const uint32_t NL = 2u * d.P * d.N;
    const uint64_t stride = script_stride(d.P, d.N, depth), tstride = shrink_tstride(d);
    const uint64_t offsets[4] = {0u, 0u, n, n};
    std::vector<uint8_t> rows((size_t)(3u * stride), 0u);
    std::vector<uint16_t> tables((size_t)(3u * tstride), (uint16_t)SHR_NONE);
    memcpy(rows.data() + stride, row, (size_t)stride);
    memcpy(tables.data() + tstride, table, (size_t)tstride * sizeof(uint16_t));
    held.assign(n, 0u);
    sent.assign((size_t)n * NL, 0u);
    res.assign((size_t)n * 4u, 0u);
    ShrParams k{};
    k.p = make_params(cfg);
    k.p.first_instance = 0;
    k.rows = rows.data();
    k.stride = stride;
    k.table = tables.data();
    k.tstride = tstride;
    k.offsets = offsets;
    k.count = 3u;
    k.total = n;
    k.depth = depth;
    k.flag_mask = flag_mask;
    k.prefix = prefix;
    k.held = held.data();
    k.csent = sent.data();
    k.cres = reinterpret_cast<uint4*>(res.data());
    for (uint64_t c = 0; c < n; ++c)
      if (int rc = dispatch(Cand{cfg, &k, c})) return rc;
    return 0;
  }
};

constexpr uint32_t NO_PREFIX = 0xFFFFFFFFu;

// the select kernel's accept step, entry by entry: neutralise ranks <= best,
// settle, re-rank the faults of the new row; returns their count
uint32_t accept_and_enumerate(const ShrinkDims& d, uint8_t* row, uint16_t* tab, const uint16_t* sent, uint32_t best) {
  const uint32_t E = shrink_entries(d), Pi = shrink_row_P(d, row);
  uint32_t base = 0u;
  for (uint32_t t = 0; t < E; ++t) {
    const bool neutral = best != NO_PREFIX && tab[t] <= best;
    const bool f = shrink_accept_entry(d, row, Pi, sent, t, neutral);
    tab[t] = (uint16_t)(f ? base++ : SHR_NONE);
  }
  return base;
}

// one parent through pxb.shrink's rounds
int shrink_one(const pxb_config* cfg, uint8_t* row, uint32_t depth, uint32_t flag_mask, uint32_t max_launches,
               uint32_t* status, uint32_t* n_faults, uint32_t* launches_out, uint16_t* sent_out, uint32_t* res_out,
               uint64_t* sig_out) {
  const ShrinkDims d{cfg->n_proposers, cfg->n_acceptors, depth, cfg->delay_max};
  const uint32_t E = shrink_entries(d), NL = 2u * d.P * d.N;
  std::vector<uint16_t> tab((size_t)shrink_tstride(d), (uint16_t)SHR_NONE), psent(NL, 0), cs(NL, 0);
  uint32_t res[4] = {0u, 0u, 0u, 0u}, launches = 1u, nf = 0u, st;
  Launch l;
  if (int rc = l.run(cfg, row, tab.data(), depth, flag_mask, 1u, false)) return rc;
  memcpy(res, l.res.data(), 16);
  cs = l.sent;
  do {
    if (!l.held[0]) {
      st = PXB_SHRINK_NOT_INPUT;
      break;
    }
    uint64_t total = 0;
    for (uint32_t t = 0; t < E; ++t) total += shrink_is_fault(d, row, shrink_row_P(d, row), cs.data(), t);
    if (total > SHR_MAX_FAULTS) {
      st = PXB_SHRINK_TOO_MANY;
      break;
    }
    nf = accept_and_enumerate(d, row, tab.data(), cs.data(), NO_PREFIX);
    psent = cs;
    for (;;) {
      if (nf == 0u) {
        st = PXB_SHRINK_MINIMAL;
        break;
      }
      if (launches + 2u > max_launches) {
        st = PXB_SHRINK_BUDGET;
        break;
      }
      // singles
      if (int rc = l.run(cfg, row, tab.data(), depth, flag_mask, nf, false)) return rc;
      ++launches;
      uint32_t nrem = 0u;
      for (uint32_t t = 0; t < E; ++t) {
        const uint32_t r = tab[t];
        tab[t] = (uint16_t)((r != SHR_NONE && l.held[r]) ? nrem++ : SHR_NONE);
      }
      if (nrem == 0u) {
        st = PXB_SHRINK_MINIMAL;
        break;
      }
      // prefixes: the longest that holds
      if (int rc = l.run(cfg, row, tab.data(), depth, flag_mask, nrem, true)) return rc;
      ++launches;
      uint32_t best = NO_PREFIX;
      for (uint32_t j = 0; j < nrem; ++j)
        if (l.held[j]) best = j;
      if (best == NO_PREFIX) {
        st = PXB_SHRINK_UNSTABLE;
        break;
      }
      cs.assign(l.sent.begin() + (size_t)best * NL, l.sent.begin() + (size_t)(best + 1u) * NL);
      memcpy(res, l.res.data() + (size_t)best * 4u, 16);
      nf = accept_and_enumerate(d, row, tab.data(), cs.data(), best);
      psent = cs;
    }
  } while (0);
  const bool shrunk = st == PXB_SHRINK_MINIMAL || st == PXB_SHRINK_BUDGET || st == PXB_SHRINK_UNSTABLE;
  uint64_t h = 0ull;
  uint32_t n = 0u;
  if (shrunk) {
    h = shrink_fnv_begin(row);
    for (uint32_t t = 0; t < E; ++t)
      if (shrink_is_fault(d, row, shrink_row_P(d, row), psent.data(), t)) {
        h = shrink_fnv_record(h, shrink_fault_record(d, row, t));
        ++n;
      }
  } else {
    std::fill(psent.begin(), psent.end(), (uint16_t)0);
  }
  if (status) *status = st;
  if (n_faults) *n_faults = n;
  if (launches_out) *launches_out = launches;
  if (sent_out) memcpy(sent_out, psent.data(), NL * sizeof(uint16_t));
  if (res_out) memcpy(res_out, res, 16);
  if (sig_out) *sig_out = h;
  return 0;
}

}  // namespace

// pxb_shrink_batch on the host, its arguments (PXB_E_NODEV aside)
extern "C" int shrink_host_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count,
                                 uint32_t depth, uint32_t flag_mask, uint32_t max_launches, uint32_t* status,
                                 uint32_t* n_faults, uint32_t* launches, uint16_t* sent, pxb_result* results,
                                 uint64_t* signature) {
  if (!cfg || (count && !rows) || count > (1ull << 30) || depth > PXB_SCRIPT_MAX_DEPTH || !(flag_mask & 0xFFu) ||
      max_launches == 0u || !trace_config_ok(cfg))
    return PXB_E_INVAL;
  const uint32_t P = cfg->n_proposers, N = cfg->n_acceptors;
  const uint64_t stride = script_stride(P, N, depth);
  EvParams p = make_params(cfg);
  p.first_instance = 0;
  for (uint64_t i = 0; i < count; ++i) {
    uint8_t* const row = rows + i * stride;
    if (ids)
      for (uint64_t j = 0; j < stride; ++j) row[j] = script_row_byte(p, P, N, depth, ids[i], j);
    if (int rc = shrink_one(cfg, row, depth, flag_mask, max_launches, status ? status + i : nullptr,
                            n_faults ? n_faults + i : nullptr, launches ? launches + i : nullptr,
                            sent ? sent + i * 2u * P * N : nullptr,
                            results ? reinterpret_cast<uint32_t*>(results + i) : nullptr,
                            signature ? signature + i : nullptr))
      return rc;
  }
  return 0;
}

#ifdef PXB_SHRINK_HOST_MAIN
// Sanitizer-build driver (tests/test_shrink_host.py): ids first .. first + n - 1
// of config 3's shape shrunk at `depth`, every buffer holding exactly what the
// call may write.  To a file of raw bytes: the rows, then status, fault counts,
// launches, send counts, results and signatures, one array after the other.
// argv: out seed first n depth loss delay skew cap flag_mask max_launches
int main(int argc, char** argv) {
  if (argc != 12) {
    fprintf(stderr, "usage: %s out seed first n depth loss delay skew cap flag_mask max_launches\n", argv[0]);
    return 2;
  }
  pxb_config c{};
  c.seed = strtoull(argv[2], nullptr, 0);
  const uint64_t first = strtoull(argv[3], nullptr, 0), n = strtoull(argv[4], nullptr, 0);
  const uint32_t depth = (uint32_t)strtoul(argv[5], nullptr, 0);
  c.n_proposers = 2;
  c.n_acceptors = 5;
  c.n_ticks = 1;
  c.tick_period = 1;
  c.crash_len_max = 1;
  uint32_t* f[] = {&c.loss_ppm, &c.delay_max, &c.skew_max, &c.step_cap};
  for (int i = 0; i < 4; ++i) *f[i] = (uint32_t)strtoul(argv[6 + i], nullptr, 0);
  const uint32_t flag_mask = (uint32_t)strtoul(argv[10], nullptr, 0), max_launches = (uint32_t)strtoul(argv[11], nullptr, 0);
  const uint32_t P = 2, N = 5;
  std::vector<uint64_t> ids(n);
  for (uint64_t g = 0; g < n; ++g) ids[g] = first + g;
  std::vector<uint8_t> rows(n * script_stride(P, N, depth));   // exactly the rows
  std::vector<uint32_t> st(n), nf(n), la(n);
  std::vector<uint16_t> sent(n * 2u * P * N);
  std::vector<pxb_result> res(n);
  std::vector<uint64_t> sig(n);
  if (shrink_host_batch(&c, ids.data(), rows.data(), n, depth, flag_mask, max_launches, st.data(), nf.data(), la.data(),
                        sent.data(), res.data(), sig.data()) != 0)
    return 4;
  FILE* o = fopen(argv[1], "wb");
  if (!o) return 3;
  fwrite(rows.data(), 1, rows.size(), o);
  fwrite(st.data(), 4, n, o);
  fwrite(nf.data(), 4, n, o);
  fwrite(la.data(), 4, n, o);
  fwrite(sent.data(), 2, sent.size(), o);
  fwrite(res.data(), sizeof(pxb_result), n, o);
  fwrite(sig.data(), 8, n, o);
  fclose(o);
  return 0;
}
#endif
