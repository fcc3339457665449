// paxos_explore_cover.hip — which handler classes lie within k faults of a row
// (include/paxos_batch.h, docs/SEMANTICS.md §15): pxb_explore_cover,
// pxb_explore_cover_device.
//
// pxb_explore's space and list with pxb_cover's fold.  The candidate kernel is
// paxos_explore_kernel's with CoverLane (cover_core.h) in TraceLane's place over
// ExploreEventDraws (explore_cover_core.h): lane l of block b is candidate
// 64 b + l of the call, which unranks its changes, tests its site bytes for keep
// entries, runs to its end folding its events into its mask in registers and
// writes ONE flag byte (ran OK, held by §15's predicate).  No candidate row, no
// event and no per-candidate mask is ever stored.  The wave then reduces into
// the parents' reach records: a wave of 64 consecutive candidates can straddle
// parents and radii, so it walks its distinct (parent, radius) keys as the
// minimal kernel does, and per key the 29 classes as the cover kernel does: one
// ballot, and where a lane has the class one atomic add to count[r][b] and one
// atomic minimum to first[b] with the c of the lowest such lane (within one
// parent c ascends with the lane).  Integer adds and minima only: the records
// do not depend on the order the waves end in.  An init kernel in front sets
// the records, a finishing kernel behind gives union_mask.  The list is
// pxb_explore's (explore_driver.h, with the host side of both calls) over the
// flag bytes.  No block waits for another; plain vector stores only.
//
// Built as three units by proposer count (-DPXB_EXC_P=1|2|3); the unit of P = 1
// also holds the other kernels and the entry points.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "explore_cover_core.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXC_P
#error "PXB_EXC_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct ExcParams {
  EvParams p;
  ExploreSpace e;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  uint64_t total;                   // candidates of this call (count * T <= 2^32)
  uint32_t depth, site_depth, flag_mask;
  pxb_cover_query q;
  uint8_t* bytes;                   // total flag bytes
  pxb_explore_reach* reach;         // count records, initialised (nullable)
};

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_cover_kernel(ExcParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ExploreEventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 64u + lane;
  const bool in = g < k.total;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  bool run = in;
  if (run) {
    const uint32_t tt = (uint32_t)k.e.T, i = (uint32_t)g / tt, c = (uint32_t)g - i * tt;   // (g < 2^32)
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.e, explore_unrank(k.e, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_cover_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
  }
  const bool started = run;
  script_run(L, E, k.p, run);
  uint32_t f = 0u, m = 0u;
  if (started && E.status == PXB_TRACE_OK) {
    uint16_t snt[NL];
    script_sent(L, snt);
    f = explore_cover_flags(E.res[3], E.mask, snt, NL, k.depth, k.flag_mask, k.q);
    m = (f & EXP_RAN) ? E.mask : 0u;
  }
  if (in) k.bytes[g] = (uint8_t)f;
  if (k.reach == nullptr) return;   // (wave-uniform)
  // ---- the wave's reduction into the reach records ----
  uint32_t key = 0u, c = 0u;
  if (in) {
    const uint32_t tt = (uint32_t)k.e.T, i = (uint32_t)g / tt;
    c = (uint32_t)g - i * tt;
    key = i * 4u + explore_radius(k.e, c);
    if (c == 0u) k.reach[i].parent_mask = m;
  }
  unsigned long long act = __ballot(m != 0u);
  while (act != 0ull) {             // (wave-uniform) one distinct (parent, radius) a turn
    const int lead = __ffsll(act) - 1;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const bool same = (m != 0u) & (key == k0);
    pxb_explore_reach* const o = k.reach + (k0 >> 2);
    uint32_t* const cnt = &o->count[0][0] + (k0 & 3u) * 32u;
#pragma unroll 1
    for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b) {
      const unsigned long long bal = __ballot(same & (((m >> b) & 1u) != 0u));
      if (bal == 0ull) continue;    // (wave-uniform: no candidate of the key has the class)
      const uint32_t cmin = (uint32_t)__builtin_amdgcn_readlane((int)c, __ffsll(bal) - 1);
      if ((int)lane == lead) {
        atomicAdd(cnt + b, (uint32_t)__popcll(bal));
        atomicMin(&o->first[b], cmin);
      }
    }
    act &= ~__ballot(same);
  }
}

typedef void (*exc_ptr)(ExcParams);
struct ExcFamily {                  // (lane_shapes.h)
  typedef exc_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_explore_cover_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ExcFamily, PXB_EXC_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EXC_P == 1
#include "explore_driver.h"

namespace pxx {

constexpr uint32_t REACH_WORDS = (uint32_t)(sizeof(pxb_explore_reach) / 4u);   // 128 counts | 32 firsts | 2 masks

// one thread per word of the records: counts 0, firsts all-ones, masks 0
__global__ __launch_bounds__(256) void reach_init_kernel(uint32_t* words, uint64_t n_words) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_words) return;
  const uint32_t w = (uint32_t)(t % REACH_WORDS);
  words[t] = (w >= 128u && w < 160u) ? 0xFFFFFFFFu : 0u;
}

// behind the candidate kernel, 32 threads a parent, thread b: the union of the
// counted classes (first[b] is all-ones where nothing was counted: only a count
// comes with a minimum)
__global__ __launch_bounds__(32) void reach_finish_kernel(pxb_explore_reach* reach) {
  pxb_explore_reach* const o = reach + blockIdx.x;
  const uint32_t b = threadIdx.x;
  const bool has = (o->count[0][b] | o->count[1][b] | o->count[2][b] | o->count[3][b]) != 0u;
  const unsigned long long bal = __ballot(has);
  if (b == 0u) o->union_mask = (uint32_t)bal;
}

// explore_driver.h's rules and pxb_explore_cover's own: no outcome condition, or
// one over the outcome bits; no reserved word; no production draws (the event
// lanes have none); *fn: the shape's kernel
static int validate(const ExpArgs& a, const pxb_explore_cover_space* sp, ExploreSpace* e, exc_ptr* fn) {
  if (int rc = explore_validate(a, sp, e)) return rc;
  if ((sp->flag_mask != 0u && (sp->flag_mask & 0xFFu) == 0u) || sp->q.reserved != 0u) return PXB_E_INVAL;
  if (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<ExcFamily>(a.cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxx

extern "C" {

int pxb_explore_cover_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                             const pxb_explore_cover_space* space, uint64_t first_parent, uint64_t* d_ids,
                             uint64_t capacity, uint64_t* d_n_matches, uint32_t* d_counts, pxb_explore_reach* d_reach,
                             uint32_t* d_status, void* stream) {
  using namespace pxx;
  const ExpArgs a{cfg, d_rows, count, depth, first_parent, d_ids, capacity, d_n_matches, d_counts, d_status};
  ExploreSpace e;
  exc_ptr fn = nullptr;
  if (int rc = validate(a, space, &e, &fn)) return rc;
  if ((uintptr_t)d_reach & 7u) return PXB_E_INVAL;
  ExcParams c{};
  c.q = space->q;
  c.reach = d_reach;
  // the records set in front of the candidates, union_mask behind them
  const auto init = [&](hipStream_t st) {
    if (!d_reach) return hipSuccess;
    const uint64_t n_words = count * REACH_WORDS;
    hipLaunchKernelGGL(reach_init_kernel, dim3((unsigned)((n_words + 255u) / 256u)), dim3(256), 0, st,
                       reinterpret_cast<uint32_t*>(d_reach), n_words);
    return hipGetLastError();
  };
  const auto finish = [&](hipStream_t st) {
    if (!d_reach) return hipSuccess;
    hipLaunchKernelGGL(reach_finish_kernel, dim3((unsigned)count), dim3(32), 0, st, d_reach);
    return hipGetLastError();
  };
  return explore_device(a, space, e, (hipStream_t)stream, fn, c, init, finish);
}

int pxb_explore_cover(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                      const pxb_explore_cover_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                      uint32_t* counts, pxb_explore_reach* reach, uint32_t* status) {
  using namespace pxx;
  const ExpArgs h{cfg, rows, count, depth, 0, ids, capacity, n_matches, counts, status};
  ExploreSpace e;
  exc_ptr fn = nullptr;
  if (int rc = validate(h, space, &e, &fn)) return rc;
  return explore_staged(h, e, reach, sizeof(pxb_explore_reach), [&](const ExpArgs& d, void* d_reach) {
    return pxb_explore_cover_device(cfg, d.rows, d.count, depth, space, d.first_parent, d.ids, d.capacity,
                                    d.n_matches, d.counts, static_cast<pxb_explore_reach*>(d_reach), d.status,
                                    nullptr);
  });
}

}  // extern "C"
#endif  // PXB_EXC_P == 1
