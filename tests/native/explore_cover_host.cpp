// explore_cover_host.cpp — TEST ONLY: the shared logic of pxb_explore_cover
// (cloud-haskell-paxos_amd/csrc/explore_cover_core.h: ExploreEventDraws under
// CoverLane, the flag byte; explore_core.h: the space, the keep-site test, the
// minimality test) driven sequentially on the host, one candidate at a time, so
// tests/test_explore_cover_host.py can check it against brute force without a
// GPU.  The product runs the same code on the device
// (paxos_explore_cover.hip); the reach records here are the plain sequential
// statement of what the kernel's wave reduction and atomics compute.  Nothing
// here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/explore_cover_core.h"
#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/script_lane.h"
#include "explore_host.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

static_assert(offsetof(pxb_explore_reach, first) == 512 && offsetof(pxb_explore_reach, parent_mask) == 640 &&
                  offsetof(pxb_explore_reach, union_mask) == 644 && offsetof(pxb_explore_cover_space, q) == 16,
              "record fields");

namespace {

// one candidate: what one lane of paxos_explore_cover_kernel does before its wave's reduction
struct Cand {
  const pxb_config* cfg;
  const ExploreSpace* e;
  const uint8_t* row;
  uint32_t depth, site_depth, c, flag_mask;
  const pxb_cover_query* q;
  uint8_t* flags;
  uint32_t* mask;
};

template <int PM, int N, int W, bool LG>
int run_shape(const Cand& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ExploreEventDraws>::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  *a.flags = 0u;
  *a.mask = 0u;
  const ExploreByte x = explore_byte(*a.e, explore_unrank(*a.e, a.c), a.row, N, a.site_depth, a.depth);
  if (explore_parent_bad(a.row, PM) || explore_changes_keep(x)) return 0;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  uint64_t guard = 0;
  if (explore_cover_begin(L, p, a.depth, a.row, x) != PXB_TRACE_OK) return 0;
  while (E.iter(L, p))
    if (++guard > guard_max) return -100;
  if (E.status != PXB_TRACE_OK) return 0;
  uint16_t snt[NL];
  script_sent(L, snt);
  const uint32_t f = explore_cover_flags(E.res[3], E.mask, snt, NL, a.depth, a.flag_mask, *a.q);
  *a.flags = (uint8_t)f;
  *a.mask = (f & EXP_RAN) ? E.mask : 0u;
  return 0;
}

#ifdef PXB_EXPLORE_COVER_HOST_MAIN
// (the sanitizer build: one shape, P = 1, N = 3 on the 8-step wheel)
int dispatch(const Cand& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 1 || c->n_acceptors != 3 || wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return run_shape<1, 3, 8, false>(a);
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

}  // namespace

// pxb_explore_cover_device on the host, its arguments; `bytes` (nullable):
// count * T flag bytes, what the kernels keep in scratch; `masks` (nullable):
// count * T masks, which the kernels keep nowhere
extern "C" int explore_cover_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                                      const pxb_explore_cover_space* sp, uint64_t first_parent, uint64_t* ids,
                                      uint64_t capacity, uint64_t* n_matches, uint32_t* counts,
                                      pxb_explore_reach* reach, uint32_t* status, uint8_t* bytes, uint32_t* masks) {
  if (!cfg || !sp || !n_matches || (count && !rows) || depth > PXB_SCRIPT_MAX_DEPTH || sp->site_depth == 0u ||
      sp->site_depth > depth || sp->radius > PXB_EXPLORE_MAX_RADIUS || (sp->flag_mask && !(sp->flag_mask & 0xFFu)) ||
      (sp->flags & ~PXB_EXPLORE_MINIMAL) || sp->q.reserved || (capacity && !ids) || !trace_config_ok(cfg) ||
      (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return PXB_E_INVAL;
  const uint32_t P = cfg->n_proposers, N = cfg->n_acceptors;
  const ExploreSpace e = explore_space(explore_sites(P, N, sp->site_depth), cfg->delay_max, sp->radius);
  if (!e.T || count * e.T > (1ull << 32)) return PXB_E_INVAL;
  const uint64_t stride = script_stride(P, N, depth);
  const uint32_t sel = (sp->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  uint64_t pos = *n_matches;
  const ExploreHostOut out{first_parent, ids, capacity, &pos, counts, status, bytes};
  std::vector<uint8_t> f((size_t)e.T);
  std::vector<uint32_t> m((size_t)e.T);
  for (uint64_t i = 0; i < count; ++i) {
    const uint8_t* const row = rows + i * stride;
    for (uint64_t c = 0; c < e.T; ++c)
      if (int rc = dispatch(Cand{cfg, &e, row, depth, sp->site_depth, (uint32_t)c, sp->flag_mask, &sp->q,
                                 &f[(size_t)c], &m[(size_t)c]}))
        return rc;
    explore_host_parent(e, P, row, i, sel, f.data(), out);
    // the reach record: the masks folded by radius and class
    pxb_explore_reach r;
    memset(&r, 0, sizeof r);
    for (int b = 0; b < 32; ++b) r.first[b] = 0xFFFFFFFFu;
    r.parent_mask = m[0];
    for (uint64_t c = 0; c < e.T; ++c) {
      const uint32_t rad = explore_unrank(e, c).r;
      for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b)
        if ((m[(size_t)c] >> b) & 1u) {
          r.count[rad][b] += 1u;
          if ((uint32_t)c < r.first[b]) r.first[b] = (uint32_t)c;
          r.union_mask |= 1u << b;
        }
    }
    if (reach) memcpy(reinterpret_cast<unsigned char*>(reach) + i * sizeof r, &r, sizeof r);
    if (masks) memcpy(masks + i * e.T, m.data(), (size_t)e.T * 4u);
  }
  *n_matches = pos;
  return 0;
}

#ifdef PXB_EXPLORE_COVER_HOST_MAIN
// Sanitizer-build driver (tests/test_explore_cover_host.py).  argv: in out.
// The input file: a pxb_config, a pxb_explore_cover_space, then little-endian
// uint32 depth, uint64 count, then the rows.  Every buffer holds exactly what
// the call may write.  The output file: the flag bytes, the masks, the counts,
// the reach records, the status words, the match count and the listed ids.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  pxb_config c{};
  pxb_explore_cover_space sp{};
  uint32_t depth = 0;
  uint64_t count = 0;
  if (fread(&c, sizeof c, 1, f) != 1 || fread(&sp, sizeof sp, 1, f) != 1 || fread(&depth, 4, 1, f) != 1 ||
      fread(&count, 8, 1, f) != 1)
    return 3;
  if (count > 64 || depth > PXB_SCRIPT_MAX_DEPTH || c.n_proposers != 1 || c.n_acceptors != 3) return 3;
  const uint64_t T = explore_space(explore_sites(1u, 3u, sp.site_depth), c.delay_max, sp.radius).T;
  if (!T || T > (1u << 16)) return 3;
  const uint64_t stride = script_stride(1u, 3u, depth);
  std::vector<uint8_t> rows((size_t)(count * stride));                  // exactly the rows
  if (count && fread(rows.data(), 1, rows.size(), f) != rows.size()) return 3;
  fclose(f);
  std::vector<uint8_t> bytes((size_t)(count * T));
  std::vector<uint32_t> masks((size_t)(count * T)), counts((size_t)(count * 12u)), status((size_t)count);
  std::vector<pxb_explore_reach> reach((size_t)count);
  uint64_t n = 0;
  if (explore_cover_host_run(&c, rows.data(), count, depth, &sp, 0, nullptr, 0, &n, counts.data(), reach.data(),
                             status.data(), bytes.data(), masks.data()))
    return 4;
  std::vector<uint64_t> ids((size_t)n);                                  // exactly the matches
  uint64_t n2 = 0;
  if (explore_cover_host_run(&c, rows.data(), count, depth, &sp, 0, ids.data(), n, &n2, counts.data(), reach.data(),
                             status.data(), bytes.data(), masks.data()) ||
      n2 != n)
    return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  fwrite(bytes.data(), 1, bytes.size(), o);
  fwrite(masks.data(), 4, masks.size(), o);
  fwrite(counts.data(), 4, counts.size(), o);
  fwrite(reach.data(), sizeof(pxb_explore_reach), reach.size(), o);
  fwrite(status.data(), 4, status.size(), o);
  fwrite(&n, 8, 1, o);
  fwrite(ids.data(), 8, ids.size(), o);
  fclose(o);
  return 0;
}
#endif
