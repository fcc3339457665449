// explore_win_host.cpp — TEST ONLY: the shared logic of pxb_explore_win
// (cloud-haskell-paxos_amd/csrc/explore_win_core.h: the window space, its unrank
// and rank, the overwrite of a started lane's windows, the two-axis minimality
// test; explore_cover_core.h: the lane and the flag byte) driven sequentially on
// the host, one candidate at a time (explore_host.h, over the joint space's
// policy), so tests/test_explore_win_host.py can check
// it against brute force without a GPU.  The product runs the same code on the
// device (paxos_explore_win.hip); the counts and the reach records here are the
// plain sequential statement of what the kernels' wave reductions and atomics
// compute.  Nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/explore_win_core.h"
#include "explore_host.h"

using namespace pxb;
using namespace pxb::ev;

static_assert(offsetof(pxb_explore_win_reach, first) == 1536 && offsetof(pxb_explore_win_reach, parent_mask) == 3072 &&
                  offsetof(pxb_explore_win_reach, union_mask) == 3076 && offsetof(pxb_explore_win_space, q) == 16 &&
                  offsetof(pxb_explore_win_space, win_radius) == 32,
              "record fields");

namespace {

ExploreWin space_of(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp) {
  return explore_win_make(explore_space(explore_sites(P, N, sp->site_depth), delay_max, sp->radius),
                          explore_win_space(N, sp->win_radius, sp->win_first, sp->win_starts, sp->win_lens,
                                            (sp->flags & PXB_EXPLORE_WIN_OPEN) != 0u));
}

}  // namespace

extern "C" {

// T_w of the space (0: none)
uint64_t explore_win_host_total(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp) {
  return space_of(P, N, delay_max, sp).Tw;
}

// every candidate c' of the space: rank(unrank(c')) == c', the radii are those
// of the intervals, the acceptors ascend below N, the digits are below W, the
// window is non-empty and within 4096.  Returns the number of candidates that
// fail (or ~0 for no space).
uint64_t explore_win_host_check(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp) {
  const ExploreWin x = space_of(P, N, delay_max, sp);
  if (!x.Tw) return ~0ull;
  uint64_t bad = 0;
  for (uint64_t cw = 0; cw < x.Tw; ++cw) {
    const uint64_t h = cw / x.e.T, c = cw % x.e.T;
    const WinCand kw = explore_win_unrank(x.w, h);
    const ExploreCand kl = explore_unrank(x.e, c);
    bool ok = kw.r <= sp->win_radius && h >= x.w.base[kw.r] && h < x.w.base[kw.r + 1u] &&
              explore_win_rank(x.w, kw) * x.e.T + explore_rank(x.e, kl) == cw &&
              explore_win_cell(x, (uint32_t)h, (uint32_t)c) == kw.r * 4u + kl.r;
    for (uint32_t i = 0; i < kw.r; ++i) {
      uint32_t c0, c1;
      explore_win_bounds(x.w, kw.digit[i], &c0, &c1);
      ok = ok && kw.acc[i] < N && (i == 0u || kw.acc[i - 1u] < kw.acc[i]) && kw.digit[i] < x.w.W && c0 < c1 &&
           c1 <= 4096u && explore_win_word(x.w, kw.digit[i]) == (c0 | (c1 << 16));
    }
    bad += !ok;
  }
  return bad;
}

// candidates c[0..n): out[12 i ..] = r_w, acc[2], wdigit[2], r_l, site[3], digit[3]
int explore_win_host_unrank(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp,
                            const uint64_t* c, uint64_t n, uint32_t* out) {
  const ExploreWin x = space_of(P, N, delay_max, sp);
  if (!x.Tw) return PXB_E_INVAL;
  for (uint64_t i = 0; i < n; ++i) {
    if (c[i] >= x.Tw) return PXB_E_INVAL;
    const WinCand kw = explore_win_unrank(x.w, c[i] / x.e.T);
    const ExploreCand kl = explore_unrank(x.e, c[i] % x.e.T);
    uint32_t* const o = out + 12 * i;
    o[0] = kw.r, o[5] = kl.r;
    for (uint32_t j = 0; j < 2u; ++j) o[1 + j] = kw.acc[j], o[3 + j] = kw.digit[j];
    for (uint32_t j = 0; j < 3u; ++j) o[6 + j] = kl.site[j], o[9 + j] = kl.digit[j];
  }
  return 0;
}

// pxb_explore_win_device on the host, its arguments; `bytes` (nullable): count *
// T_w flag bytes, what the kernels keep in scratch; `masks` (nullable): count *
// T_w masks, which the kernels keep nowhere
int explore_win_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                         const pxb_explore_win_space* sp, uint64_t first_parent, uint64_t* ids, uint64_t capacity,
                         uint64_t* n_matches, uint32_t* counts, pxb_explore_win_reach* reach, uint32_t* status,
                         uint8_t* bytes, uint32_t* masks) {
  if (!explore_host_link_rules(cfg, depth, sp)) return PXB_E_INVAL;
  return explore_cover_host_run<ExploreWinX>(cfg, space_of(cfg->n_proposers, cfg->n_acceptors, cfg->delay_max, sp), rows,
                                             count, depth, sp,
                                             ExploreHostOut{first_parent, ids, capacity, nullptr, counts, status, bytes},
                                             n_matches, reach, masks);
}

}  // extern "C"

#ifdef PXB_EXPLORE_WIN_HOST_MAIN
// Sanitizer-build driver (tests/test_explore_win_host.py).  argv: in out.  The
// input file: a pxb_config, a pxb_explore_win_space, then little-endian uint32
// depth, uint64 count, then the rows.  Every buffer holds exactly what the call
// may write.  The output file: the bijection check's failures (uint64), the
// flag bytes, the masks, the counts, the reach records, the status words, the
// match count and the listed ids.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  pxb_config c{};
  pxb_explore_win_space sp{};
  uint32_t depth = 0;
  uint64_t count = 0;
  if (fread(&c, sizeof c, 1, f) != 1 || fread(&sp, sizeof sp, 1, f) != 1 || fread(&depth, 4, 1, f) != 1 ||
      fread(&count, 8, 1, f) != 1)
    return 3;
  if (count > 64 || depth > PXB_SCRIPT_MAX_DEPTH || c.n_proposers != 1 || c.n_acceptors != 3) return 3;
  const uint64_t T = explore_win_host_total(1u, 3u, c.delay_max, &sp);
  if (!T || T > (1u << 16)) return 3;
  const uint64_t stride = script_stride(1u, 3u, depth);
  std::vector<uint8_t> rows((size_t)(count * stride));                  // exactly the rows
  if (count && fread(rows.data(), 1, rows.size(), f) != rows.size()) return 3;
  fclose(f);
  const uint64_t bad = explore_win_host_check(1u, 3u, c.delay_max, &sp);
  std::vector<uint8_t> bytes((size_t)(count * T));
  std::vector<uint32_t> masks((size_t)(count * T)), counts((size_t)(count * EXW_CELLS * 3u)), status((size_t)count);
  std::vector<pxb_explore_win_reach> reach((size_t)count);
  uint64_t n = 0;
  if (explore_win_host_run(&c, rows.data(), count, depth, &sp, 0, nullptr, 0, &n, counts.data(), reach.data(),
                           status.data(), bytes.data(), masks.data()))
    return 4;
  std::vector<uint64_t> ids((size_t)n);                                  // exactly the matches
  uint64_t n2 = 0;
  if (explore_win_host_run(&c, rows.data(), count, depth, &sp, 0, ids.data(), n, &n2, counts.data(), reach.data(),
                           status.data(), bytes.data(), masks.data()) ||
      n2 != n)
    return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  fwrite(&bad, 8, 1, o);
  fwrite(bytes.data(), 1, bytes.size(), o);
  fwrite(masks.data(), 4, masks.size(), o);
  fwrite(counts.data(), 4, counts.size(), o);
  fwrite(reach.data(), sizeof(pxb_explore_win_reach), reach.size(), o);
  fwrite(status.data(), 4, status.size(), o);
  fwrite(&n, 8, 1, o);
  fwrite(ids.data(), 8, ids.size(), o);
  fclose(o);
  return 0;
}
#endif
