// sweep_plan_host.cpp — TEST ONLY: prints the chunk list of a pxb_sweep
// (csrc/sweep_plan.h) so that the chunk arithmetic is checked without a GPU:
//   sweep_plan_host <first_instance> <n_instances> <PXB_SWEEP_CHUNK value>
// prints the clamped chunk size, then one "first count" line per chunk.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../cloud-haskell-paxos_amd/csrc/sweep_plan.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const uint64_t first = strtoull(argv[1], nullptr, 10), n = strtoull(argv[2], nullptr, 10);
  const uint64_t chunk = pxb::sweep_clamp_chunk(atoll(argv[3]));
  printf("%" PRIu64 "\n", chunk);
  for (uint64_t k = 0, nk = pxb::sweep_n_chunks(n, chunk); k < nk; ++k) {
    const pxb::SweepChunk c = pxb::sweep_chunk_at(first, n, chunk, k);
    printf("%" PRIu64 " %" PRIu64 "\n", c.first, c.count);
  }
  return 0;
}
