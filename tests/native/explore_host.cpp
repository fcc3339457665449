// explore_host.cpp — TEST ONLY: the explorer's shared logic
// (cloud-haskell-paxos_amd/csrc/explore_core.h: the space, unrank and rank,
// ExploreByte and ExploreDraws over the per-lane state machine, the keep-site
// test, the minimality test) driven sequentially on the host, one candidate at
// a time, so tests/test_explore_host.py can check it against pxb.explore_rows
// and the scripted lane without a GPU.  The product runs the same code on the
// device (paxos_explore.hip); nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/explore_core.h"
#include "explore_host.h"

using namespace pxb;
using namespace pxb::ev;

namespace {

// one candidate: what one lane of paxos_explore_kernel does (spelled out here
// as in the kernel: paxos_explore.hip says why it is not shared)
struct Cand {
  const pxb_config* cfg;
  const ExploreSpace* e;
  const uint8_t* row;
  uint32_t depth, site_depth, c, flag_mask;
  uint8_t* flags;
};

template <int PM, int N, int W, bool LG>
int run_shape(const Cand& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ExploreDraws>::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  *a.flags = 0u;
  const ExploreByte x = explore_byte(*a.e, explore_unrank(*a.e, a.c), a.row, N, a.site_depth, a.depth);
  if (explore_parent_bad(a.row, PM) || explore_changes_keep(x)) return 0;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  TraceLane<Lane> T;
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  uint64_t guard = 0;
  T.begin_count(1u, 0u);
  if (explore_begin(L, p, a.depth, a.row, x) != PXB_TRACE_OK) return 0;
  while (T.iter(L, p))
    if (++guard > guard_max) return -100;
  if (T.status != PXB_TRACE_OK) return 0;
  uint16_t snt[NL];
  script_sent(L, snt);
  *a.flags = (uint8_t)explore_flags(T.status, T.res[3], snt, NL, a.depth, a.flag_mask);
  return 0;
}

#ifdef PXB_EXPLORE_HOST_MAIN
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

extern "C" {

// T of S sites with A alternatives within radius R (0: none)
uint64_t explore_host_total(uint64_t S, uint32_t A, uint32_t R) { return explore_space(S, A, R).T; }

// every candidate of the space: rank(unrank(c)) == c, the radius is that of c's
// interval, the sites ascend below S, the digits are below A.  Returns the
// number of candidates that fail (or ~0 for no space).
uint64_t explore_host_check(uint64_t S, uint32_t A, uint32_t R) {
  const ExploreSpace e = explore_space(S, A, R);
  if (!e.T) return ~0ull;
  uint64_t bad = 0;
  for (uint64_t c = 0; c < e.T; ++c) {
    const ExploreCand k = explore_unrank(e, c);
    bool ok = k.r <= R && c >= e.base[k.r] && c < e.base[k.r + 1u] && explore_rank(e, k) == c;
    for (uint32_t i = 0; i < k.r; ++i)
      ok = ok && k.site[i] < S && (i == 0u || k.site[i - 1u] < k.site[i]) && k.digit[i] < A;
    bad += !ok;
  }
  return bad;
}

// candidates c[0..n): out[7 i ..] = r, site[3], digit[3]
int explore_host_unrank(uint64_t S, uint32_t A, uint32_t R, const uint64_t* c, uint64_t n, uint32_t* out) {
  const ExploreSpace e = explore_space(S, A, R);
  if (!e.T) return PXB_E_INVAL;
  for (uint64_t i = 0; i < n; ++i) {
    if (c[i] >= e.T) return PXB_E_INVAL;
    const ExploreCand k = explore_unrank(e, c[i]);
    out[7 * i] = k.r;
    for (uint32_t j = 0; j < 3u; ++j) out[7 * i + 1 + j] = k.site[j], out[7 * i + 4 + j] = k.digit[j];
  }
  return 0;
}

// pxb_explore_device on the host, its arguments; `bytes` (nullable): count * T
// flag bytes, what the kernels keep in scratch
int explore_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                     const pxb_explore_space* sp, uint64_t first_parent, uint64_t* ids, uint64_t capacity,
                     uint64_t* n_matches, uint32_t* counts, uint32_t* status, uint8_t* bytes) {
  if (!explore_host_link_rules(cfg, depth, sp) || !n_matches || (count && !rows) || !(sp->flag_mask & 0xFFu) ||
      (sp->flags & ~ExploreLinkX::FLAGS) || (capacity && !ids))
    return PXB_E_INVAL;
  const uint32_t P = cfg->n_proposers, N = cfg->n_acceptors;
  const ExploreSpace e = explore_space(explore_sites(P, N, sp->site_depth), cfg->delay_max, sp->radius);
  if (!e.T || count * e.T > (1ull << 32)) return PXB_E_INVAL;
  const uint64_t stride = script_stride(P, N, depth);
  const uint32_t sel = (sp->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  uint64_t pos = *n_matches;
  const ExploreHostOut out{first_parent, ids, capacity, &pos, counts, status, bytes};
  std::vector<uint8_t> f((size_t)e.T);
  for (uint64_t i = 0; i < count; ++i) {
    const uint8_t* const row = rows + i * stride;
    for (uint64_t c = 0; c < e.T; ++c)
      if (int rc = dispatch(Cand{cfg, &e, row, depth, sp->site_depth, (uint32_t)c, sp->flag_mask, &f[(size_t)c]}))
        return rc;
    explore_host_parent<ExploreLinkX>(e, P, row, i, sel, f.data(), out);
  }
  *n_matches = pos;
  return 0;
}

}  // extern "C"

#ifdef PXB_EXPLORE_HOST_MAIN
// Sanitizer-build driver (tests/test_explore_host.py): the benign row of P = 1,
// N = 3, delay_max 2 (every link byte 1, no skews, no windows) explored at
// depth 16, site_depth 2, radius 3, every buffer holding exactly what the call
// may write.  To a file of raw bytes: the flag bytes, the counts, the status,
// the match count and the listed ids.
// argv: out seed step_cap flag_mask flags
int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s out seed step_cap flag_mask flags\n", argv[0]);
    return 2;
  }
  pxb_config c{};
  c.seed = strtoull(argv[2], nullptr, 0);
  c.n_proposers = 1;
  c.n_acceptors = 3;
  c.delay_max = 2;
  c.n_ticks = 1;
  c.tick_period = 1;
  c.crash_len_max = 1;
  c.step_cap = (uint32_t)strtoul(argv[3], nullptr, 0);
  const pxb_explore_space sp{2u, 3u, (uint32_t)strtoul(argv[4], nullptr, 0), (uint32_t)strtoul(argv[5], nullptr, 0)};
  const uint32_t depth = 16u;
  const uint64_t T = explore_host_total(explore_sites(1u, 3u, sp.site_depth), c.delay_max, sp.radius);
  std::vector<uint8_t> row((size_t)script_stride(1u, 3u, depth), 0u);   // exactly the row
  row[8] = 1u;
  memset(row.data() + script_links_off(3u), 1, (size_t)script_links_bytes(1u, 3u, depth));
  std::vector<uint8_t> bytes((size_t)T);
  std::vector<uint32_t> counts(12), status(1);
  uint64_t n = 0;
  if (explore_host_run(&c, row.data(), 1, depth, &sp, 0, nullptr, 0, &n, counts.data(), status.data(), bytes.data()))
    return 4;
  std::vector<uint64_t> ids((size_t)n);                                  // exactly the matches
  uint64_t n2 = 0;
  if (explore_host_run(&c, row.data(), 1, depth, &sp, 0, ids.data(), n, &n2, counts.data(), status.data(), bytes.data()) ||
      n2 != n)
    return 4;
  FILE* o = fopen(argv[1], "wb");
  if (!o) return 3;
  fwrite(bytes.data(), 1, bytes.size(), o);
  fwrite(counts.data(), 4, counts.size(), o);
  fwrite(status.data(), 4, 1, o);
  fwrite(&n, 8, 1, o);
  fwrite(ids.data(), 8, ids.size(), o);
  fclose(o);
  return 0;
}
#endif
