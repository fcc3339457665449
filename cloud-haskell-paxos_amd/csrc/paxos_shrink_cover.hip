// paxos_shrink_cover.hip — the batched shrinker over a coverage predicate
// (include/paxos_batch.h, docs/SEMANTICS.md §16): pxb_shrink_cover_batch and
// pxb_shrink_cover_batch_device.
//
// pxb_shrink_batch's rounds with pxb_cover's fold in the predicate.  The
// candidate kernel is paxos_shrink_kernel's with CoverLane (cover_core.h) in
// TraceLane's place over ShrinkEventDraws (shrink_cover_core.h): lane l of block
// b is candidate 64 b + l of the launch, which finds its parent, reads the
// parent's row through its rank table, runs to its end folding its events into
// its mask in registers and writes ONE `held` byte (§16's predicate), and in the
// initial and the prefix launches its send counts, its result and its 4-byte
// mask.  No candidate row, no event and no mask of a single is ever stored.
// Everything around the candidate kernel (select, finish, the fill kernel, the
// host loop) is shrink_driver.h's, which carries the accepted candidate's mask
// to its parent as it carries the result.  No block waits for another; plain
// vector stores only.
//
// Built as three units by proposer count (-DPXB_SHC_P=1|2|3); the unit of P = 1
// also holds the driver's kernels and the entry points.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "lane_shapes.h"
#include "script_lane.h"
#include "shrink_cover_core.h"

#ifndef PXB_SHC_P
#error "PXB_SHC_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_shrink_cover_kernel(ShcParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ShrinkEventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t c = (uint64_t)blockIdx.x * 64u + lane;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.s.p);
  CoverLane<Lane> E;
  const bool run = k.begin(L, E, c);
  script_run(L, E, k.s.p, run);
  // (the stores stay here, as in paxos_shrink_kernel)
  if (c < k.s.total) {
    uint16_t snt[NL];
    if (E.status == PXB_TRACE_OK) {
      script_sent(L, snt);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < NL; ++q) snt[q] = 0u;
    }
    k.s.held[c] = shrink_cover_holds(E.status, E.res[3], E.mask, snt, NL, k.s.depth, k.s.flag_mask, k.q) ? 1u : 0u;
    if (k.s.csent) {
#pragma unroll
      for (uint32_t q = 0; q < NL; ++q) k.s.csent[c * NL + q] = snt[q];
    }
    if (k.s.cres) k.s.cres[c] = make_uint4(E.res[0], E.res[1], E.res[2], E.res[3]);
    if (k.cmask) k.cmask[c] = E.mask;   // (0 unless the run ended PXB_TRACE_OK)
  }
}

typedef void (*shc_ptr)(ShcParams);
struct ShcFamily {                  // (lane_shapes.h)
  typedef shc_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_shrink_cover_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ShcFamily, PXB_SHC_P)

}  // namespace ev
}  // namespace pxb

#if PXB_SHC_P == 1
#include "shrink_driver.h"

namespace pxsh {

// the argument rules both calls share
static int validate_cover(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth,
                          const pxb_shrink_pred* pred, shc_ptr* fn) {
  if (!pred) return PXB_E_INVAL;
  if (int rc = shrink_validate(cfg, rows, count, depth, pred->max_launches)) return rc;
  constexpr uint32_t CLASSES = (1u << PXB_COVER_CLASSES) - 1u;
  if ((pred->flag_mask & ~0xFFu) || pred->reserved[0] || pred->reserved[1] || pred->q.reserved) return PXB_E_INVAL;
  if ((pred->q.all_mask | pred->q.any_mask | pred->q.none_mask) & ~CLASSES) return PXB_E_INVAL;
  if (cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<ShcFamily>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxsh

extern "C" {

int pxb_shrink_cover_batch_device(const pxb_config* cfg, uint8_t* d_rows, uint64_t count, uint32_t depth,
                                  const pxb_shrink_pred* pred, uint32_t* d_status, uint32_t* d_n_faults,
                                  uint32_t* d_launches, uint16_t* d_sent, pxb_result* d_results,
                                  uint64_t* d_signature, uint32_t* d_masks, void* stream) {
  using namespace pxsh;
  shc_ptr fn = nullptr;
  if (int rc = validate_cover(cfg, d_rows, count, depth, pred, &fn)) return rc;
  const ShrOut o{d_status, d_n_faults, d_launches, d_sent, reinterpret_cast<uint4*>(d_results), d_signature, d_masks};
  if (!shrink_aligned(d_rows, o)) return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;
  ShcParams c{};
  c.s.flag_mask = pred->flag_mask;
  c.q = pred->q;
  return shrink_drive(cfg, d_rows, count, depth, pred->max_launches, fn, c, c.s, &c.cmask, o, dev, st);
}

int pxb_shrink_cover_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                           const pxb_shrink_pred* pred, uint32_t* status, uint32_t* n_faults, uint32_t* launches,
                           uint16_t* sent, pxb_result* results, uint64_t* signature, uint32_t* masks) {
  using namespace pxsh;
  shc_ptr fn = nullptr;
  if (int rc = validate_cover(cfg, rows, count, depth, pred, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) return PXB_OK;
  const ShrOut h{status, n_faults, launches, sent, reinterpret_cast<uint4*>(results), signature, masks};
  return shrink_staged(cfg, ids, rows, count, depth, h, true, [&](uint8_t* d_rows, const ShrOut& d) {
    return pxb_shrink_cover_batch_device(cfg, d_rows, count, depth, pred, d.status, d.n_faults, d.launches, d.sent,
                                         reinterpret_cast<pxb_result*>(d.results), d.signature, d.masks, nullptr);
  });
}

}  // extern "C"
#endif  // PXB_SHC_P == 1
