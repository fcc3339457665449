// shrink_cover_host.cpp — TEST ONLY: the shared logic of pxb_shrink_cover_batch
// (cloud-haskell-paxos_amd/csrc/shrink_cover_core.h: ShrinkEventDraws under
// CoverLane, ShcParams::begin, shrink_cover_holds; shrink_core.h: the rank
// tables, select and settle, the signature) driven sequentially on the host, one
// parent and one candidate at a time, so tests/test_shrink_cover_host.py can
// check it against pxb.shrink_cover without a GPU.  The product runs the same
// code on the device (paxos_shrink_cover.hip, shrink_driver.h); the rounds here
// are the sequential statement of shrink_driver.h's kernels, as in
// shrink_host.cpp.  Nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/script_lane.h"
#include "../../cloud-haskell-paxos_amd/csrc/shrink_cover_core.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

static_assert(offsetof(pxb_shrink_pred, max_launches) == 4 && offsetof(pxb_shrink_pred, q) == 16, "pred fields");

namespace {

// candidate `c` of a launch as paxos_shrink_cover_kernel runs it
struct Cand {
  const pxb_config* cfg;
  const ShcParams* k;
  uint64_t c;
};

// ShcParams::begin is the kernel's own; the stores after the run are spelled out here as in the kernel
template <int PM, int N, int W, bool LG>
int run_shape(const Cand& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ShrinkEventDraws>::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  const ShcParams& k = *a.k;
  HostLane<Lane> H(k.s.p);
  Lane& L = H.L;
  CoverLane<Lane> E;
  bool run = k.begin(L, E, a.c);
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  for (uint64_t guard = 0; run;) {
    run = E.iter(L, k.s.p);
    if (run && ++guard > guard_max) return -100;
  }
  uint16_t* const snt = k.s.csent + a.c * NL;
  if (E.status == PXB_TRACE_OK) script_sent(L, snt);
  else memset(snt, 0, NL * sizeof(uint16_t));
  k.s.held[a.c] = shrink_cover_holds(E.status, E.res[3], E.mask, snt, NL, k.s.depth, k.s.flag_mask, k.q) ? 1u : 0u;
  memcpy(reinterpret_cast<unsigned char*>(k.s.cres) + 16u * a.c, E.res, 16);
  k.cmask[a.c] = E.mask;
  return 0;
}

#ifdef PXB_SHRINK_COVER_HOST_MAIN
// (the sanitizer build: one shape, P = 2, N = 3 on the 8-step wheel)
int dispatch(const Cand& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 2 || c->n_acceptors != 3 || wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return run_shape<2, 3, 8, false>(a);
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
// (offsets 0, 0, n, n), so that ShrParams::start's search over the offsets runs.
struct Launch {
  std::vector<uint8_t> held;        // n
  std::vector<uint16_t> sent;       // n * 2 P N
  std::vector<uint32_t> res;        // n * 4
  std::vector<uint32_t> mask;       // n
  int run(const pxb_config* cfg, const uint8_t* row, const uint16_t* table, uint32_t depth, const pxb_shrink_pred& pr,
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
    mask.assign(n, 0u);
    ShcParams k{};
    k.s.p = make_params(cfg);
    k.s.p.first_instance = 0;
    k.s.rows = rows.data();
    k.s.stride = stride;
    k.s.table = tables.data();
    k.s.tstride = tstride;
    k.s.offsets = offsets;
    k.s.count = 3u;
    k.s.total = n;
    k.s.depth = depth;
    k.s.flag_mask = pr.flag_mask;
    k.s.prefix = prefix;
    k.s.held = held.data();
    k.s.csent = sent.data();
    k.s.cres = reinterpret_cast<uint4*>(res.data());
    k.q = pr.q;
    k.cmask = mask.data();
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

struct Out {
  uint32_t *status, *n_faults, *launches;
  uint16_t* sent;
  uint32_t* res;
  uint64_t* sig;
  uint32_t* mask;
};

// one parent through pxb.shrink_cover's rounds
int shrink_one(const pxb_config* cfg, uint8_t* row, uint32_t depth, const pxb_shrink_pred& pr, const Out& o) {
  const ShrinkDims d{cfg->n_proposers, cfg->n_acceptors, depth, cfg->delay_max};
  const uint32_t E = shrink_entries(d), NL = 2u * d.P * d.N;
  std::vector<uint16_t> tab((size_t)shrink_tstride(d), (uint16_t)SHR_NONE), psent(NL, 0), cs(NL, 0);
  uint32_t res[4] = {0u, 0u, 0u, 0u}, launches = 1u, nf = 0u, st, mask;
  Launch l;
  if (int rc = l.run(cfg, row, tab.data(), depth, pr, 1u, false)) return rc;
  memcpy(res, l.res.data(), 16);
  mask = l.mask[0];
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
      if (launches + 2u > pr.max_launches) {
        st = PXB_SHRINK_BUDGET;
        break;
      }
      // singles
      if (int rc = l.run(cfg, row, tab.data(), depth, pr, nf, false)) return rc;
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
      if (int rc = l.run(cfg, row, tab.data(), depth, pr, nrem, true)) return rc;
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
      mask = l.mask[best];
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
  if (o.status) *o.status = st;
  if (o.n_faults) *o.n_faults = n;
  if (o.launches) *o.launches = launches;
  if (o.sent) memcpy(o.sent, psent.data(), NL * sizeof(uint16_t));
  if (o.res) memcpy(o.res, res, 16);
  if (o.sig) *o.sig = h;
  if (o.mask) *o.mask = mask;
  return 0;
}

}  // namespace

// pxb_shrink_cover_batch on the host, its arguments (PXB_E_NODEV aside)
extern "C" int shrink_cover_host_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count,
                                       uint32_t depth, const pxb_shrink_pred* pr, uint32_t* status, uint32_t* n_faults,
                                       uint32_t* launches, uint16_t* sent, pxb_result* results, uint64_t* signature,
                                       uint32_t* masks) {
  if (!cfg || !pr || (count && !rows) || count > (1ull << 30) || depth > PXB_SCRIPT_MAX_DEPTH ||
      (pr->flag_mask & ~0xFFu) || pr->max_launches == 0u || pr->reserved[0] || pr->reserved[1] || pr->q.reserved ||
      ((pr->q.all_mask | pr->q.any_mask | pr->q.none_mask) >> PXB_COVER_CLASSES) || !trace_config_ok(cfg) ||
      (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return PXB_E_INVAL;
  const uint32_t P = cfg->n_proposers, N = cfg->n_acceptors;
  const uint64_t stride = script_stride(P, N, depth);
  EvParams p = make_params(cfg);
  p.first_instance = 0;
  for (uint64_t i = 0; i < count; ++i) {
    uint8_t* const row = rows + i * stride;
    if (ids)
      for (uint64_t j = 0; j < stride; ++j) row[j] = script_row_byte(p, P, N, depth, ids[i], j);
    const Out o{status ? status + i : nullptr,
                n_faults ? n_faults + i : nullptr,
                launches ? launches + i : nullptr,
                sent ? sent + i * 2u * P * N : nullptr,
                results ? reinterpret_cast<uint32_t*>(results + i) : nullptr,
                signature ? signature + i : nullptr,
                masks ? masks + i : nullptr};
    if (int rc = shrink_one(cfg, row, depth, *pr, o)) return rc;
  }
  return 0;
}

#ifdef PXB_SHRINK_COVER_HOST_MAIN
// Sanitizer-build driver (tests/test_shrink_cover_host.py).  argv: in out.  The
// input file: a pxb_config, a pxb_shrink_pred, then little-endian uint32 depth,
// uint64 first, uint64 n.  Ids first .. first + n - 1 of the P = 2, N = 3 shape
// shrunk at `depth`, every buffer holding exactly what the call may write.  The
// output file: the rows, then status, fault counts, launches, send counts,
// results, signatures and masks, one array after the other.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  pxb_config c{};
  pxb_shrink_pred pr{};
  uint32_t depth = 0;
  uint64_t first = 0, n = 0;
  if (fread(&c, sizeof c, 1, f) != 1 || fread(&pr, sizeof pr, 1, f) != 1 || fread(&depth, 4, 1, f) != 1 ||
      fread(&first, 8, 1, f) != 1 || fread(&n, 8, 1, f) != 1)
    return 3;
  fclose(f);
  if (n > 4096 || depth > PXB_SCRIPT_MAX_DEPTH || c.n_proposers != 2 || c.n_acceptors != 3) return 3;
  const uint32_t P = 2, N = 3;
  std::vector<uint64_t> ids(n);
  for (uint64_t g = 0; g < n; ++g) ids[g] = first + g;
  std::vector<uint8_t> rows(n * script_stride(P, N, depth));   // exactly the rows
  std::vector<uint32_t> st(n), nf(n), la(n), mk(n);
  std::vector<uint16_t> sent(n * 2u * P * N);
  std::vector<pxb_result> res(n);
  std::vector<uint64_t> sig(n);
  if (shrink_cover_host_batch(&c, ids.data(), rows.data(), n, depth, &pr, st.data(), nf.data(), la.data(), sent.data(),
                              res.data(), sig.data(), mk.data()) != 0)
    return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  fwrite(rows.data(), 1, rows.size(), o);
  fwrite(st.data(), 4, n, o);
  fwrite(nf.data(), 4, n, o);
  fwrite(la.data(), 4, n, o);
  fwrite(sent.data(), 2, sent.size(), o);
  fwrite(res.data(), sizeof(pxb_result), n, o);
  fwrite(sig.data(), 8, n, o);
  fwrite(mk.data(), 4, n, o);
  fclose(o);
  return 0;
}
#endif
