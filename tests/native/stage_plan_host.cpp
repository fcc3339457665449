// stage_plan_host.cpp — host checks of csrc/stage_plan.h (tests/test_stage_plan.py
// builds it with -Wall -Werror, and again under the address and undefined
// behaviour sanitizers).  "check": the properties, exit 0 or a message and 1.
// "scripted P N count depth stride" / "shrink ...": the offsets and the total of
// the region lists of pxb_run_scripted / pxb_shrink_batch, for the test to
// compare with the sums it computes itself.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cloud-haskell-paxos_amd/csrc/stage_plan.h"

using pxb::StagePlan;
using pxb::StageRegion;

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      printf("line %d: %s\n", __LINE__, #x);                  \
      return 1;                                               \
    }                                                         \
  } while (0)

static int check() {
  // a mixed list: odd sizes, an exact multiple of 256, empty regions in the middle and at both ends
  const uint64_t elem[] = {8, 1, 16, 4, 4, 292, 2, 96, 1, 8}, count[] = {0, 1300, 130, 0, 64, 7, 131, 0, 1, 0};
  StagePlan plan;
  uint64_t end = 0;
  for (int i = 0; i < 10; ++i) {
    const uint64_t before = plan.total;
    const StageRegion r = plan.add(elem[i], count[i]);
    CHECK(plan.valid && !r.late && r.elem == elem[i] && r.count == count[i] && r.bytes() == elem[i] * count[i]);
    CHECK(plan.total % 256 == 0);
    if (r.bytes() == 0) {
      CHECK(plan.total == before);                 // takes nothing
      continue;
    }
    CHECK(r.offset % 256 == 0 && r.offset >= end);  // aligned, ascending, past the one before
    CHECK(r.offset == before);
    end = r.offset + r.bytes();
    CHECK(plan.total == ((end + 255) & ~(uint64_t)255) && plan.total - end < 256);   // the padded end
  }
  CHECK(end == 256 * 26 + 1 && plan.total == 256 * 27);   // blocks: 1300 -> 6, 2080 -> 9, 256 -> 1, 2044 -> 8, 262 -> 2, 1 -> 1
  StagePlan none;
  CHECK(none.valid && none.total == 0);
  // overflow: a product, then a sum that wraps; both invalid, and they stay so
  StagePlan a;
  a.add(4, 10);
  const StageRegion big = a.add(16, 1ull << 62);
  CHECK(!a.valid && big.count == 0 && big.bytes() == 0);
  a.add(1, 1);
  CHECK(!a.valid);
  StagePlan b;
  b.add(1, ~(uint64_t)0 - 100);
  CHECK(!b.valid);                                 // (the padding of the end wraps)
  StagePlan c;
  c.add(1, 1ull << 63);
  CHECK(c.valid && c.total == 1ull << 63);
  c.add(1, 1ull << 63);
  CHECK(!c.valid);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "check")) {
    const int rc = check();
    if (rc == 0) printf("ok\n");
    return rc;
  }
  if (argc != 7) return 2;
  const uint64_t P = strtoull(argv[2], 0, 10), N = strtoull(argv[3], 0, 10), count = strtoull(argv[4], 0, 10);
  const uint64_t stride = strtoull(argv[6], 0, 10);
  StagePlan plan;
  StageRegion r[8];
  int n = 0;
  if (!strcmp(argv[1], "scripted")) {              // rows | results | digests | records | status | sent
    r[n++] = plan.add(stride, count);
    r[n++] = plan.add(16, count);
    r[n++] = plan.add(N * 4, count);
    r[n++] = plan.add(N * 16, count);
    r[n++] = plan.add(4, count);
    r[n++] = plan.add(2 * P * N * 2, count);
  } else if (!strcmp(argv[1], "shrink")) {         // rows | ids | status | faults | launches | sent | results | signature
    r[n++] = plan.add(stride, count);
    r[n++] = plan.add(8, count);
    r[n++] = plan.add(4, count);
    r[n++] = plan.add(4, count);
    r[n++] = plan.add(4, count);
    r[n++] = plan.add(2 * P * N * 2, count);
    r[n++] = plan.add(16, count);
    r[n++] = plan.add(8, count);
  } else {
    return 2;
  }
  for (int i = 0; i < n; ++i) printf("%llu ", (unsigned long long)r[i].offset);
  printf("%llu %d\n", (unsigned long long)plan.total, plan.valid ? 1 : 0);
  return 0;
}
