// paxos_explore.hip — bounded exhaustive exploration (include/paxos_batch.h,
// docs/SEMANTICS.md §12): pxb_explore, pxb_explore_device, pxb_explore_row and
// pxb_explore_total.
//
// Every schedule within `radius` changed link entries of each parent row, run
// on the device.  Candidate g of a call is candidate g % T of parent g / T (T is
// the same for every parent: no search), and no candidate row exists: a
// candidate is its parent's row read through ExploreByte (explore_core.h).
// Four kernels and hipCUB's exclusive sum:
//   the candidate kernel: paxos_shrink_kernel's shape over ExploreDraws.  Lane l
//     of block b is candidate 64 b + l; it unranks its changes, tests its at
//     most three site bytes for keep entries, runs to its end under TraceLane
//     with the empty record window and writes ONE flag byte (ran OK, held);
//   the minimal kernel, one thread per candidate: a held candidate ranks its at
//     most 6 proper non-empty subsets and candidate 0, reads their bytes and
//     sets the minimal bit; the wave adds its per-(parent, radius) counts with
//     integer atomics (one add per distinct key and column); the block writes
//     the number of candidates it lists;
//   the cursor kernel and the scatter kernel of paxos_query.hip's list, over
//     the flag bytes: ascending g from the caller's cursor, below `capacity`.
// Everything is sized from count x T: the device form never synchronises.  No
// block waits for another; plain vector stores only.  All but the candidate
// kernel live in explore_list.h, which pxb_explore_cover
// (paxos_explore_cover.hip) shares.
//
// Built as three units by proposer count (-DPXB_EXP_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the other kernels and
// the entry points.  The shapes are lane_shapes.h's.  (The kernel spells out
// what its lane does before and after the run, and tests/native/explore_host.cpp
// spells it again: moved into shared members the same text compiled to other
// register counts)
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "explore_core.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXP_P
#error "PXB_EXP_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct ExpParams {
  EvParams p;
  ExploreSpace e;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  uint64_t total;                   // candidates of this call (count * T <= 2^32)
  uint32_t depth, site_depth, flag_mask;
  uint8_t* bytes;                   // total flag bytes
};

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_kernel(ExpParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ExploreDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 64u + lane;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  TraceLane<Lane> T;
  T.begin_count(1u, 0u);            // (an empty window: no records are counted)
  bool run = g < k.total;
  if (run) {
    const uint32_t tt = (uint32_t)k.e.T, i = (uint32_t)g / tt, c = (uint32_t)g - i * tt;   // (g < 2^32)
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.e, explore_unrank(k.e, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
  }
  const bool started = run;
  script_run(L, T, k.p, run);
  if (g < k.total) {
    uint32_t f = 0u;
    if (started && T.status == PXB_TRACE_OK) {
      uint16_t snt[NL];
      script_sent(L, snt);
      f = explore_flags(T.status, T.res[3], snt, NL, k.depth, k.flag_mask);
    }
    k.bytes[g] = (uint8_t)f;
  }
}

typedef void (*exp_ptr)(ExpParams);
// the kernel of a config's shape among the unit's of PM proposers (null: none);
// each unit specialises it for its own proposer count
template <int PM>
exp_ptr exp_pick(const pxb_config* cfg);
template <> exp_ptr exp_pick<1>(const pxb_config* cfg);
template <> exp_ptr exp_pick<2>(const pxb_config* cfg);
template <> exp_ptr exp_pick<3>(const pxb_config* cfg);

template <int PM>
struct ExpKernel {
  template <int N, int W, bool LG>
  exp_ptr shape() const { return paxos_explore_kernel<PM, N, W, LG>; }
};
template <>
exp_ptr exp_pick<PXB_EXP_P>(const pxb_config* cfg) { return lane_shape(cfg, ExpKernel<PXB_EXP_P>{}, (exp_ptr) nullptr); }

}  // namespace ev
}  // namespace pxb

#if PXB_EXP_P == 1
#include "explore_list.h"

extern "C" uint64_t explore_chunk_hook(void);   // paxos_batch.hip: PXB_EXPLORE_CHUNK

namespace pxx {
using namespace pxb::ev;
using namespace pxb::host;

struct ExpPick {
  const pxb_config* cfg;
  template <int PM>
  exp_ptr proposers() const { return exp_pick<PM>(cfg); }
};
static int pick(const pxb_config* cfg, exp_ptr* fn) {
  *fn = lane_proposers(cfg, ExpPick{cfg}, (exp_ptr) nullptr);
  return *fn ? PXB_OK : PXB_E_INVAL;
}
static int validate_space(const pxb_config* cfg, uint32_t depth, const pxb_explore_space* sp, ExploreSpace* e) {
  if (!sp) return PXB_E_INVAL;
  return validate_space_of(cfg, depth, sp->site_depth, sp->radius, e);
}
// the argument rules both calls share
static int validate(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth,
                    const pxb_explore_space* sp, const void* ids, uint64_t capacity, const void* n_matches,
                    ExploreSpace* e, exp_ptr* fn) {
  if (int rc = validate_space(cfg, depth, sp, e)) return rc;
  if ((count && !rows) || count > MAX_COUNT || !n_matches || (capacity && !ids)) return PXB_E_INVAL;
  if ((sp->flag_mask & 0xFFu) == 0u || (sp->flags & ~PXB_EXPLORE_MINIMAL) != 0u) return PXB_E_INVAL;
  return pick(cfg, fn);
}

}  // namespace pxx

extern "C" {

uint64_t pxb_explore_total(uint32_t P, uint32_t N, uint32_t delay_max, uint32_t site_depth, uint32_t radius) {
  using namespace pxb::ev;
  return explore_space(explore_sites(P, N, site_depth), delay_max, radius).T;
}

int pxb_explore_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_space* space, const uint8_t* parent,
                    uint64_t c, uint8_t* out_row) {
  using namespace pxx;
  ExploreSpace e;
  if (int rc = validate_space(cfg, depth, space, &e)) return rc;
  if (!parent || !out_row || c >= e.T) return PXB_E_INVAL;
  const uint32_t N = cfg->n_acceptors;
  const ExploreByte x = explore_byte(e, explore_unrank(e, c), parent, N, space->site_depth, depth);
  if (explore_changes_keep(x)) return PXB_E_INVAL;
  if (out_row != parent) memcpy(out_row, parent, (size_t)script_stride(cfg->n_proposers, N, depth));
  uint8_t* const links = out_row + script_links_off(N);
  for (uint32_t i = 0; i < 3u; ++i)
    if (x.idx[i] != EXP_NO_SITE) links[x.idx[i]] = (uint8_t)explore_alt(x.links[x.idx[i]], x.dig[i], x.A);
  return PXB_OK;
}

int pxb_explore_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                       const pxb_explore_space* space, uint64_t first_parent, uint64_t* d_ids, uint64_t capacity,
                       uint64_t* d_n_matches, uint32_t* d_counts, uint32_t* d_status, void* stream) {
  using namespace pxx;
  ExploreSpace e;
  exp_ptr fn = nullptr;
  if (int rc = validate(cfg, d_rows, count, depth, space, d_ids, capacity, d_n_matches, &e, &fn)) return rc;
  if (count * e.T > MAX_CALL) return PXB_E_INVAL;                       // (count <= 2^30, T <= 2^30)
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_ids & 7u) || ((uintptr_t)d_n_matches & 7u) ||
      ((uintptr_t)d_counts & 3u) || ((uintptr_t)d_status & 3u))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;

  const uint64_t total = count * e.T;
  ExpScratch x;
  if (int rc = explore_scratch(dev, total, st, &x)) return rc;
  uint8_t* const bytes = x.bytes;

  ExpParams c{};
  c.p = make_params(cfg);
  c.p.first_instance = 0;
  c.e = e;
  c.rows = d_rows;
  c.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  c.total = total;
  c.depth = depth;
  c.site_depth = space->site_depth;
  c.flag_mask = space->flag_mask;
  c.bytes = bytes;
  ExpList l{};
  l.e = e;
  l.rows = d_rows;
  l.stride = c.stride;
  l.total = total;
  l.P = cfg->n_proposers;
  l.sel = (space->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  l.bytes = bytes;
  l.tcount = x.tcount;
  l.counts = d_counts;
  l.status = d_status;

  hipError_t err = hipSuccess;
  do {
    if (d_counts && (err = hipMemsetAsync(d_counts, 0, (size_t)(count * 12u * 4u), st)) != hipSuccess) break;
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 63u) / 64u)), dim3(64), 0, st, c);
    if ((err = hipGetLastError()) != hipSuccess) break;
    err = explore_list(l, x, first_parent * e.T, d_ids, capacity, d_n_matches, st);
  } while (0);
  const hipError_t f = hipFreeAsync(x.buf, st);   // (stream-ordered: after the launches above)
  if (err == hipSuccess) err = f;
  return (err == hipSuccess) ? PXB_OK : hip_fail(err);
}

int pxb_explore(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                const pxb_explore_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                uint32_t* counts, uint32_t* status) {
  using namespace pxx;
  ExploreSpace e;
  exp_ptr fn = nullptr;
  if (int rc = validate(cfg, rows, count, depth, space, ids, capacity, n_matches, &e, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  *n_matches = 0;
  if (count == 0) return PXB_OK;
  // whole parents, at most PXB_EXPLORE_CHUNK candidates a chunk (and at least one parent)
  const uint64_t chunk = explore_chunk_hook();
  const uint64_t per = chunk / e.T ? chunk / e.T : 1u, m_max = per < count ? per : count;
  const uint64_t stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  const uint64_t cap = capacity < count * e.T ? capacity : count * e.T;
  pxb::StagePlan plan;                            // rows (one chunk) | cursor | ids | counts | status
  const pxb::StageRegion r_rows = plan.add(stride, m_max), r_n = plan.add(sizeof(uint64_t), 1);
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), cap), r_cnt = plan.add(12u * sizeof(uint32_t), count);
  const pxb::StageRegion r_st = plan.add(sizeof(uint32_t), count);
  Staging S(plan);
  S.zero(r_n);
  uint32_t* const d_cnt = S.ptr<uint32_t>(r_cnt, counts);
  uint32_t* const d_st = S.ptr<uint32_t>(r_st, status);
  for (uint64_t a = 0; a < count && S.ok(); a += m_max) {
    const uint64_t m = count - a < m_max ? count - a : m_max;
    S.up(r_rows, rows + a * stride, m);
    if (S.ok())
      S.note(pxb_explore_device(cfg, S.ptr<uint8_t>(r_rows), m, depth, space, a, S.ptr<uint64_t>(r_ids), cap,
                                S.ptr<uint64_t>(r_n), d_cnt ? d_cnt + a * 12u : nullptr, d_st ? d_st + a : nullptr,
                                nullptr));
    // (the next chunk's rows overwrite these: wait for the kernels that read them)
    if (S.ok()) S.note(hipStreamSynchronize(nullptr));
  }
  S.down(r_n, n_matches, 1);
  if (S.ok()) S.down(r_ids, ids, *n_matches < cap ? *n_matches : cap);
  S.down(r_cnt, counts, count);
  S.down(r_st, status, count);
  return S.finish();
}

}  // extern "C"
#endif  // PXB_EXP_P == 1
