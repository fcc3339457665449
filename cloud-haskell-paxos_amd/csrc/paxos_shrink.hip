// paxos_shrink.hip — the batched shrinker (include/paxos_batch.h, docs/SEMANTICS.md
// §11): pxb_shrink_batch and pxb_shrink_batch_device.
//
// pxb.shrink's rounds for many rows in lockstep, everything on the device: the
// parent rows, their rank tables (shrink_core.h), the candidate runs, the
// choice of the next parent row and the final signature.  Here, the candidate
// kernel: paxos_script_kernel's lane over ShrinkDraws.  Lane l of block b is
// candidate 64 b + l of the launch; its parent comes from a binary search over
// hipCUB's exclusive sum of the per-parent candidate counts; it reads the
// parent's row and table (no candidate row exists), runs to its end under
// TraceLane with the empty record window and writes one `held` byte, and in the
// initial and the prefix launches its send counts and result.  The select, the
// finish and the fill kernel and the host loop around them are shrink_driver.h's,
// shared with pxb_shrink_cover_batch (paxos_shrink_cover.hip).  No block waits
// for another; plain vector stores only.
//
// Built as three units by proposer count (-DPXB_SHR_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the driver's kernels and
// the entry points.  What one candidate's lane does before its run is
// ShrParams::begin (shrink_core.h), which tests/native/shrink_host.cpp runs on
// the host; the shapes are lane_shapes.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "lane_shapes.h"
#include "script_lane.h"
#include "shrink_core.h"

#ifndef PXB_SHR_P
#error "PXB_SHR_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_shrink_kernel(ShrParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ShrinkDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t c = (uint64_t)blockIdx.x * 64u + lane;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  TraceLane<Lane> T;
  const bool run = k.begin(L, T, c);
  script_run(L, T, k.p, run);
  // (the stores stay here: in a shared member, as begin is, the same text
  // compiled to 200 more instructions for the shapes of 48 and 54 links)
  if (c < k.total) {
    uint16_t snt[NL];
    if (T.status == PXB_TRACE_OK) {
      script_sent(L, snt);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < NL; ++q) snt[q] = 0u;
    }
    k.held[c] = shrink_holds(T.status, T.res[3], snt, NL, k.depth, k.flag_mask) ? 1u : 0u;
    if (k.csent) {
#pragma unroll
      for (uint32_t q = 0; q < NL; ++q) k.csent[c * NL + q] = snt[q];
    }
    if (k.cres) k.cres[c] = make_uint4(T.res[0], T.res[1], T.res[2], T.res[3]);
  }
}

typedef void (*shr_ptr)(ShrParams);
struct ShrFamily {                  // (lane_shapes.h)
  typedef shr_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_shrink_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ShrFamily, PXB_SHR_P)

}  // namespace ev
}  // namespace pxb

#if PXB_SHR_P == 1
#include "shrink_driver.h"

namespace pxsh {

static int pick(const pxb_config* cfg, shr_ptr* fn) {
  *fn = lane_kernel<ShrFamily>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}
// the argument rules both calls share
static int validate(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth, uint32_t flag_mask,
                    uint32_t max_launches, shr_ptr* fn) {
  if (int rc = shrink_validate(cfg, rows, count, depth, max_launches)) return rc;
  if ((flag_mask & 0xFFu) == 0u) return PXB_E_INVAL;
  return pick(cfg, fn);
}

}  // namespace pxsh

extern "C" {

int pxb_shrink_batch_device(const pxb_config* cfg, uint8_t* d_rows, uint64_t count, uint32_t depth,
                            uint32_t flag_mask, uint32_t max_launches, uint32_t* d_status, uint32_t* d_n_faults,
                            uint32_t* d_launches, uint16_t* d_sent, pxb_result* d_results, uint64_t* d_signature,
                            void* stream) {
  using namespace pxsh;
  shr_ptr fn = nullptr;
  if (int rc = validate(cfg, d_rows, count, depth, flag_mask, max_launches, &fn)) return rc;
  const ShrOut o{d_status, d_n_faults, d_launches, d_sent, reinterpret_cast<uint4*>(d_results), d_signature, nullptr};
  if (!shrink_aligned(d_rows, o)) return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;
  ShrParams c{};
  c.flag_mask = flag_mask;
  return shrink_drive(cfg, d_rows, count, depth, max_launches, fn, c, c, nullptr, o, dev, st);
}

int pxb_shrink_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                     uint32_t flag_mask, uint32_t max_launches, uint32_t* status, uint32_t* n_faults,
                     uint32_t* launches, uint16_t* sent, pxb_result* results, uint64_t* signature) {
  using namespace pxsh;
  shr_ptr fn = nullptr;
  if (int rc = validate(cfg, rows, count, depth, flag_mask, max_launches, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) return PXB_OK;
  const ShrOut h{status, n_faults, launches, sent, reinterpret_cast<uint4*>(results), signature, nullptr};
  return shrink_staged(cfg, ids, rows, count, depth, h, false, [&](uint8_t* d_rows, const ShrOut& d) {
    return pxb_shrink_batch_device(cfg, d_rows, count, depth, flag_mask, max_launches, d.status, d.n_faults, d.launches,
                                   d.sent, reinterpret_cast<pxb_result*>(d.results), d.signature, nullptr);
  });
}

}  // extern "C"
#endif  // PXB_SHR_P == 1
