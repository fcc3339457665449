// explore_cover_host.cpp — TEST ONLY: the shared logic of pxb_explore_cover
// (cloud-haskell-paxos_amd/csrc/explore_cover_core.h: ExploreEventDraws under
// CoverLane, the flag byte; explore_core.h: the space, the keep-site test, the
// minimality test) driven sequentially on the host, one candidate at a time
// (explore_host.h, over the link space's policy), so
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
#include "explore_host.h"

using namespace pxb;
using namespace pxb::ev;

static_assert(offsetof(pxb_explore_reach, first) == 512 && offsetof(pxb_explore_reach, parent_mask) == 640 &&
                  offsetof(pxb_explore_reach, union_mask) == 644 && offsetof(pxb_explore_cover_space, q) == 16,
              "record fields");

// pxb_explore_cover_device on the host, its arguments; `bytes` (nullable):
// count * T flag bytes, what the kernels keep in scratch; `masks` (nullable):
// count * T masks, which the kernels keep nowhere
extern "C" int explore_cover_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                                      const pxb_explore_cover_space* sp, uint64_t first_parent, uint64_t* ids,
                                      uint64_t capacity, uint64_t* n_matches, uint32_t* counts,
                                      pxb_explore_reach* reach, uint32_t* status, uint8_t* bytes, uint32_t* masks) {
  if (!explore_host_link_rules(cfg, depth, sp)) return PXB_E_INVAL;
  const ExploreSpace e =
      explore_space(explore_sites(cfg->n_proposers, cfg->n_acceptors, sp->site_depth), cfg->delay_max, sp->radius);
  return explore_cover_host_run<ExploreLinkX>(cfg, e, rows, count, depth, sp,
                                              ExploreHostOut{first_parent, ids, capacity, nullptr, counts, status, bytes},
                                              n_matches, reach, masks);
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
