// cover_host.cpp — TEST ONLY: the coverage lane (cloud-haskell-paxos_amd/csrc/
// cover_core.h: CoverLane over the scripted lane with the tapped draw source) on
// the host, one row at a time, so tests/test_cover_host.py can check it against
// the reference model's events without a GPU.  The product runs the same lane
// on the device (paxos_cover.hip); the summary here is the plain sequential
// statement of what the kernel's wave reduction and atomics compute.  Nothing
// here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/cover_core.h"
#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

static_assert(offsetof(pxb_cover_summary, n_matches) == 24 && offsetof(pxb_cover_summary, count) == 32 &&
                  offsetof(pxb_cover_summary, witness) == 288 && offsetof(pxb_cover_summary, witness_steps) == 544 &&
                  offsetof(pxb_cover_summary, union_mask) == 672 && offsetof(pxb_cover_summary, reserved) == 676,
              "summary fields");

namespace {

struct Args {
  const pxb_config* cfg;
  const uint8_t* row;
  uint32_t depth;
  uint32_t* mask;
  uint32_t* status;
  uint32_t* res;
};

// what one lane of paxos_cover_kernel does for its row
template <int PM, int N, int W, bool LG>
int run_shape(const Args& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, EventDraws>::Lane;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  const uint32_t st = script_begin(L, p, a.depth, a.row);
  if (st != PXB_TRACE_OK) {
    E.status = st;
  } else {
    const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
    uint64_t guard = 0;
    while (E.iter(L, p))
      if (++guard > guard_max) return -100;
  }
  *a.mask = E.status == PXB_TRACE_OK ? E.mask : 0u;
  *a.status = E.status;
  memcpy(a.res, E.res, 16);
  return 0;
}

#ifdef PXB_COVER_HOST_MAIN
// (the sanitizer build: N = 3 on the 8-step wheel, single decree and log mode)
int dispatch(const Args& a) {
  const pxb_config* c = a.cfg;
  if (c->n_acceptors != 3 || wheel_for(c->delay_max) != 8) return -1;
  if (c->n_ticks > 1) return c->n_proposers == 2 ? run_shape<2, 3, 8, true>(a) : -1;
  switch (c->n_proposers) {
    case 1: return run_shape<1, 3, 8, false>(a);
    case 2: return run_shape<2, 3, 8, false>(a);
    case 3: return run_shape<3, 3, 8, false>(a);
  }
  return -1;
}
#else
struct Run {
  const Args& a;
  template <int PM, int N, int W, bool LG>
  int run() const { return run_shape<PM, N, W, LG>(a); }
};
int dispatch(const Args& a) { return host_lane_shape(a.cfg, Run{a}, -1); }
#endif

}  // namespace

// pxb_cover over host buffers, row by row.  Return codes as the library's
// (PXB_E_INVAL for what it refuses), -100 a hang.
extern "C" int cover_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                              uint32_t* masks, uint32_t* status, pxb_result* results, pxb_cover_summary* summary) {
  if (!cfg || (count && !rows) || count > (1ull << 30) || depth > PXB_SCRIPT_MAX_DEPTH || !trace_config_ok(cfg) ||
      (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return PXB_E_INVAL;
  const uint64_t stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  pxb_cover_summary s;
  memset(&s, 0, sizeof s);
  uint64_t key[32];
  for (int b = 0; b < 32; ++b) key[b] = ~0ull;
  for (uint64_t i = 0; i < count; ++i) {
    uint32_t m = 0, st = 0, res[4];
    Args a{cfg, rows + i * stride, depth, &m, &st, res};
    if (int rc = dispatch(a)) return rc < -1 ? rc : PXB_E_INVAL;
    if (masks) masks[i] = m;
    if (status) status[i] = st;
    if (results) memcpy(results + i, res, 16);
    s.rows_ok += st == PXB_TRACE_OK;
    s.rows_bailed += st == PXB_TRACE_BAILED;
    s.rows_bad += st == PXB_SCRIPT_BAD;
    const uint64_t k = ((uint64_t)(res[3] >> 16) << 32) | i;
    for (int b = 0; b < PXB_COVER_CLASSES; ++b)
      if ((m >> b) & 1u) {
        s.count[b] += 1;
        if (k < key[b]) key[b] = k;
      }
  }
  for (int b = 0; b < 32; ++b) {
    const bool has = s.count[b] != 0;
    s.witness[b] = has ? (key[b] & 0xFFFFFFFFull) : ~0ull;
    s.witness_steps[b] = has ? (uint32_t)(key[b] >> 32) : 0xFFFFFFFFu;
    s.union_mask |= has ? 1u << b : 0u;
  }
  if (summary) memcpy(summary, &s, sizeof s);
  return PXB_OK;
}

#ifdef PXB_COVER_HOST_MAIN
// Sanitizer-build driver (tests/test_cover_host.py).  argv: in out.  The input
// file: a pxb_config, then little-endian uint32 depth, uint64 count, then the
// rows.  Every buffer holds exactly what the call may write.  The output file:
// the masks, the status words, the results, the summary.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  pxb_config c{};
  uint32_t depth = 0;
  uint64_t count = 0;
  if (fread(&c, sizeof c, 1, f) != 1 || fread(&depth, 4, 1, f) != 1 || fread(&count, 8, 1, f) != 1) return 3;
  if (count > (1u << 20) || depth > PXB_SCRIPT_MAX_DEPTH || c.n_proposers > 3 || c.n_acceptors > 9) return 3;
  const uint64_t stride = script_stride(c.n_proposers, c.n_acceptors, depth);
  std::vector<uint8_t> rows(count * stride);
  if (count && fread(rows.data(), 1, rows.size(), f) != rows.size()) return 3;
  fclose(f);
  std::vector<uint32_t> masks(count), st(count);
  std::vector<pxb_result> res(count);
  pxb_cover_summary s;
  if (cover_host_run(&c, rows.data(), count, depth, masks.data(), st.data(), res.data(), &s) != 0) return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  fwrite(masks.data(), 4, masks.size(), o);
  fwrite(st.data(), 4, st.size(), o);
  fwrite(res.data(), sizeof(pxb_result), res.size(), o);
  fwrite(&s, sizeof s, 1, o);
  fclose(o);
  return 0;
}
#endif
