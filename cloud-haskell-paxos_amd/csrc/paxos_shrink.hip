// paxos_shrink.hip — the batched shrinker (include/paxos_batch.h, docs/SEMANTICS.md
// §11): pxb_shrink_batch and pxb_shrink_batch_device.
//
// pxb.shrink's rounds for many rows in lockstep, everything on the device: the
// parent rows, their rank tables (shrink_core.h), the candidate runs, the
// choice of the next parent row and the final signature.  Four kernels:
//   the candidate kernel: paxos_script_kernel's lane over ShrinkDraws.  Lane l
//     of block b is candidate 64 b + l of the launch; its parent comes from a
//     binary search over hipCUB's exclusive sum of the per-parent candidate
//     counts; it reads the parent's row and table (no candidate row exists),
//     runs to its end under TraceLane with the empty record window and writes
//     one `held` byte, and in the initial and the prefix launches its send
//     counts and result;
//   the select kernel, one 64-lane wave per parent: after the initial launch it
//     settles and enumerates the row (ballot + mbcnt ranks), after a singles
//     launch it compacts the held singles into the removable ranking, after a
//     prefix launch it takes the longest held prefix (ballot + clz), applies it
//     in place, settles and re-enumerates;
//   the finish kernel, one wave per parent: status, fault count, launches, send
//     counts, result and the FNV-1a-64 signature;
//   a fill kernel for the first launch's counts.
// The host loop reads one 8-byte candidate total per launch to size the next
// grid: the stream is synchronised once per launch.  No block waits for
// another; plain vector stores only.
//
// Built as three units by proposer count (-DPXB_SHR_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the other kernels and
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
// the kernel of a config's shape among the unit's of PM proposers (null: none);
// each unit specialises it for its own proposer count
template <int PM>
shr_ptr shr_pick(const pxb_config* cfg);
template <> shr_ptr shr_pick<1>(const pxb_config* cfg);
template <> shr_ptr shr_pick<2>(const pxb_config* cfg);
template <> shr_ptr shr_pick<3>(const pxb_config* cfg);

template <int PM>
struct ShrKernel {
  template <int N, int W, bool LG>
  shr_ptr shape() const { return paxos_shrink_kernel<PM, N, W, LG>; }
};
template <>
shr_ptr shr_pick<PXB_SHR_P>(const pxb_config* cfg) { return lane_shape(cfg, ShrKernel<PXB_SHR_P>{}, (shr_ptr) nullptr); }

}  // namespace ev
}  // namespace pxb

#if PXB_SHR_P == 1
#include "host_util.h"

namespace pxsh {
using namespace pxb::ev;
using namespace pxb::host;

constexpr uint32_t ACTIVE = 0xFFFFFFFFu;          // state: still shrinking (else the final status)
constexpr uint32_t PH_INIT = 0u, PH_SINGLES = 1u, PH_PREFIXES = 2u;
constexpr uint32_t NO_PREFIX = 0xFFFFFFFFu;

// the parents' state between launches
struct ShrCtl {
  ShrinkDims d;
  uint32_t n_links;                 // 2 P N
  uint32_t max_launches, phase;
  uint64_t count;
  uint8_t* rows;
  uint64_t stride;
  uint16_t* table;
  uint64_t tstride;
  uint16_t* psent;                  // count * n_links: the accepted row's send counts
  uint32_t* cnt;                    // count + 1: candidates in the coming launch (the last: 0)
  const uint64_t* offsets;          // count + 1: of the launch just run
  uint32_t* state;                  // ACTIVE or the final status
  uint32_t* launches;
  uint32_t* nf;                     // faults of the accepted row
  uint4* res;                       // its result
  const uint8_t* held;              // the launch just run
  const uint16_t* csent;
  const uint4* cres;
};

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {   // set bits of lanes before this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// The accepted row of parent i: neutralises the entries of rank <= best (none:
// NO_PREFIX), settles against `sent`, and rewrites the table as the fault
// ranking of the new row.  Returns the fault count (wave-uniform).
__device__ uint32_t accept_and_enumerate(const ShrCtl& k, uint64_t i, const uint16_t* sent, uint32_t best) {
  uint8_t* const row = k.rows + i * k.stride;
  uint16_t* const tab = k.table + i * k.tstride;
  const uint32_t E = shrink_entries(k.d), Pi = shrink_row_P(k.d, row), lane = threadIdx.x;
  uint32_t base = 0u;
  for (uint32_t t0 = 0u; t0 < E; t0 += 64u) {
    const uint32_t t = t0 + lane;
    const bool in = t < E;
    const uint32_t r = in ? tab[t] : SHR_NONE;
    const bool neutral = (best != NO_PREFIX) & (r <= best);         // (best < SHR_NONE)
    const bool f = in && shrink_accept_entry(k.d, row, Pi, sent, t, neutral);
    const uint64_t b = __builtin_amdgcn_ballot_w64(f);
    if (in) tab[t] = (uint16_t)(f ? base + lanes_below(b) : SHR_NONE);
    base += (uint32_t)__builtin_popcountll(b);
  }
  return base;
}

// after an accepted row: done, out of budget, or the next singles launch
__device__ void decide(const ShrCtl& k, uint64_t i, uint32_t nf, uint32_t launches) {
  if (threadIdx.x != 0u) return;
  k.nf[i] = nf;
  k.launches[i] = launches;
  const bool done = nf == 0u, broke = launches + 2u > k.max_launches;
  k.state[i] = done ? PXB_SHRINK_MINIMAL : broke ? PXB_SHRINK_BUDGET : ACTIVE;
  k.cnt[i] = (done | broke) ? 0u : nf;
}

__device__ void stop(const ShrCtl& k, uint64_t i, uint32_t status, uint32_t launches) {
  if (threadIdx.x != 0u) return;
  k.state[i] = status;
  k.launches[i] = launches;
  k.cnt[i] = 0u;
}

__global__ __launch_bounds__(64) void shrink_select_kernel(ShrCtl k) {
  const uint64_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (k.state[i] != ACTIVE) return;               // (wave-uniform)
  const uint64_t off = k.offsets[i];
  const uint32_t n = k.cnt[i], launches = k.launches[i] + 1u, E = shrink_entries(k.d);
  uint16_t* const tab = k.table + i * k.tstride;
  if (k.phase == PH_SINGLES) {
    // the held singles, in fault order, are the removable ranking
    uint32_t base = 0u;
    for (uint32_t t0 = 0u; t0 < E; t0 += 64u) {
      const uint32_t t = t0 + lane;
      const bool in = t < E;
      const uint32_t r = in ? tab[t] : SHR_NONE;
      const bool h = (r != SHR_NONE) && k.held[off + r] != 0u;
      const uint64_t b = __builtin_amdgcn_ballot_w64(h);
      if (in) tab[t] = (uint16_t)(h ? base + lanes_below(b) : SHR_NONE);
      base += (uint32_t)__builtin_popcountll(b);
    }
    if (base == 0u) {                             // 1-minimal: this launch is the proof
      stop(k, i, PXB_SHRINK_MINIMAL, launches);
    } else if (lane == 0u) {
      k.launches[i] = launches;
      k.cnt[i] = base;
    }
    return;
  }
  uint32_t best = 0u;
  if (k.phase == PH_INIT) {
    if (lane == 0u) k.res[i] = k.cres[off];
    if (k.held[off] == 0u) {
      stop(k, i, PXB_SHRINK_NOT_INPUT, launches);
      return;
    }
    // (the count first: a row with too many faults is left as it is.  Settling
    // changes no entry's fault test: it clamps, and rewrites entries at k >= sent)
    const uint8_t* const row = k.rows + i * k.stride;
    const uint32_t Pi = shrink_row_P(k.d, row);
    uint64_t total = 0u;
    for (uint32_t t0 = 0u; t0 < E; t0 += 64u) {
      const uint32_t t = t0 + lane;
      const bool f = t < E && shrink_is_fault(k.d, row, Pi, k.csent + off * k.n_links, t);
      total += (uint64_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(f));
    }
    if (total > SHR_MAX_FAULTS) {
      stop(k, i, PXB_SHRINK_TOO_MANY, launches);
      return;
    }
    best = NO_PREFIX;
  } else {
    // the longest prefix that held, 64 candidates at a time from the top
    best = NO_PREFIX;
    for (uint32_t s = ((n - 1u) >> 6) << 6;; s -= 64u) {
      const uint32_t j = s + lane;
      const bool h = j < n && k.held[off + j] != 0u;
      const uint64_t b = __builtin_amdgcn_ballot_w64(h);
      if (b != 0ull) {
        best = s + 63u - (uint32_t)__builtin_clzll(b);
        break;
      }
      if (s == 0u) break;
    }
    if (best == NO_PREFIX) {                      // (prefix 0 is a single that held: deterministic runs keep it)
      stop(k, i, PXB_SHRINK_UNSTABLE, launches);
      return;
    }
    if (lane == 0u) k.res[i] = k.cres[off + best];
  }
  const uint64_t cand = off + (best == NO_PREFIX ? 0u : best);
  const uint16_t* const sent = k.csent + cand * k.n_links;
  const uint32_t nf = accept_and_enumerate(k, i, sent, best);
  if (lane < k.n_links) k.psent[i * k.n_links + lane] = sent[lane];
  decide(k, i, nf, launches);
}

struct ShrOut {
  uint32_t* status;
  uint32_t* n_faults;
  uint32_t* launches;
  uint16_t* sent;
  uint4* results;
  uint64_t* signature;
};

__global__ __launch_bounds__(64) void shrink_finish_kernel(ShrCtl k, ShrOut o) {
  const uint64_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint32_t st = k.state[i];
  const bool shrunk = (st == PXB_SHRINK_MINIMAL) | (st == PXB_SHRINK_BUDGET) | (st == PXB_SHRINK_UNSTABLE);
  const uint8_t* const row = k.rows + i * k.stride;
  const uint16_t* const sent = k.psent + i * k.n_links;
  uint64_t h = 0ull;
  uint32_t nf = 0u;
  if (shrunk) {                                   // (wave-uniform)
    const uint32_t E = shrink_entries(k.d), Pi = shrink_row_P(k.d, row);
    h = shrink_fnv_begin(row);
    for (uint32_t t0 = 0u; t0 < E; t0 += 64u) {
      const uint32_t t = t0 + lane;
      const bool f = t < E && shrink_is_fault(k.d, row, Pi, sent, t);
      const uint64_t rec = f ? shrink_fault_record(k.d, row, t) : 0ull;
      uint64_t b = __builtin_amdgcn_ballot_w64(f);
      nf += (uint32_t)__builtin_popcountll(b);
      while (b != 0ull) {                         // the strip's faults in order, every lane folding the same hash
        const int src = __builtin_ctzll(b);
        const uint32_t rl = (uint32_t)__shfl((int)(uint32_t)rec, src, 64);
        const uint32_t rh = (uint32_t)__shfl((int)(uint32_t)(rec >> 32), src, 64);
        h = shrink_fnv_record(h, (uint64_t)rl | ((uint64_t)rh << 32));
        b &= b - 1ull;
      }
    }
  }
  if (o.sent && lane < k.n_links) o.sent[i * k.n_links + lane] = shrunk ? sent[lane] : (uint16_t)0u;
  if (lane != 0u) return;
  if (o.status) o.status[i] = st;
  if (o.n_faults) o.n_faults[i] = nf;
  if (o.launches) o.launches[i] = k.launches[i];
  if (o.results) o.results[i] = k.res[i];
  if (o.signature) o.signature[i] = h;
}

// the first launch: one candidate per parent (the row itself: no rank selects anything)
__global__ __launch_bounds__(256) void shrink_first_counts_kernel(uint32_t* cnt, uint64_t count) {
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= count; i += step) cnt[i] = i < count ? 1u : 0u;
}

struct ShrPick {
  const pxb_config* cfg;
  template <int PM>
  shr_ptr proposers() const { return shr_pick<PM>(cfg); }
};
static int pick(const pxb_config* cfg, shr_ptr* fn) {
  *fn = lane_proposers(cfg, ShrPick{cfg}, (shr_ptr) nullptr);
  return *fn ? PXB_OK : PXB_E_INVAL;
}
// the argument rules both calls share
static int validate(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth, uint32_t flag_mask,
                    uint32_t max_launches, shr_ptr* fn) {
  if (!cfg || (count && !rows) || count > MAX_COUNT || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  if ((flag_mask & 0xFFu) == 0u || max_launches == 0u) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
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
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_n_faults & 3u) ||
      ((uintptr_t)d_launches & 3u) || ((uintptr_t)d_sent & 1u) || ((uintptr_t)d_results & 15u) ||
      ((uintptr_t)d_signature & 7u))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;

  ShrCtl k{};
  k.d = ShrinkDims{cfg->n_proposers, cfg->n_acceptors, depth, cfg->delay_max};
  k.n_links = 2u * cfg->n_proposers * cfg->n_acceptors;
  k.max_launches = max_launches;
  k.count = count;
  k.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  k.tstride = shrink_tstride(k.d);

  size_t scan_b = 0;
  if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, widen_iter(nullptr, Widen{}), (uint64_t*)nullptr,
                                                      (int64_t)(count + 1), st))
    return hip_fail(e);
  // the call's scratch: work rows | tables | sent | counts | offsets | state | launches | faults | results | scan
  // (the rows are shrunk in a copy and written back at the end: a failed call writes nothing)
  const size_t rows_b = pad256((size_t)(count * k.stride)), tab_b = pad256((size_t)(count * k.tstride * 2u));
  const size_t sent_b = pad256((size_t)(count * k.n_links * 2u)), cnt_b = pad256((size_t)((count + 1) * 4u));
  const size_t off_b = pad256((size_t)((count + 1) * 8u)), w_b = pad256((size_t)(count * 4u));
  const size_t res_b = pad256((size_t)(count * 16u));
  char* buf = nullptr;
  if (int rc = pxw::scratch(dev, rows_b + tab_b + sent_b + cnt_b + off_b + 3u * w_b + res_b + scan_b, st,
                            reinterpret_cast<void**>(&buf)))
    return rc;
  char* q = buf;
  k.rows = reinterpret_cast<uint8_t*>(q), q += rows_b;
  k.table = reinterpret_cast<uint16_t*>(q), q += tab_b;
  k.psent = reinterpret_cast<uint16_t*>(q), q += sent_b;
  k.cnt = reinterpret_cast<uint32_t*>(q), q += cnt_b;
  uint64_t* const offsets = reinterpret_cast<uint64_t*>(q);
  k.offsets = offsets, q += off_b;
  k.state = reinterpret_cast<uint32_t*>(q), q += w_b;
  k.launches = reinterpret_cast<uint32_t*>(q), q += w_b;
  k.nf = reinterpret_cast<uint32_t*>(q), q += w_b;
  k.res = reinterpret_cast<uint4*>(q), q += res_b;
  void* const scan_tmp = q;

  ShrParams c{};
  c.p = make_params(cfg);
  c.p.first_instance = 0;
  c.rows = k.rows;
  c.stride = k.stride;
  c.table = k.table;
  c.tstride = k.tstride;
  c.offsets = offsets;
  c.count = count;
  c.depth = depth;
  c.flag_mask = flag_mask;

  const dim3 parents((unsigned)count);
  hipError_t e = hipSuccess;
  int rc = PXB_OK;
  do {
    if ((e = hipMemcpyAsync(k.rows, d_rows, (size_t)(count * k.stride), hipMemcpyDeviceToDevice, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.table, 0xFF, (size_t)(count * k.tstride * 2u), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.psent, 0, sent_b, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.state, 0xFF, w_b, st)) != hipSuccess) break;        // ACTIVE
    if ((e = hipMemsetAsync(k.launches, 0, 2u * w_b + res_b, st)) != hipSuccess) break;
    {
      const uint64_t blocks = (count + 256u) / 256u;
      hipLaunchKernelGGL(shrink_first_counts_kernel, dim3((unsigned)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0,
                         st, k.cnt, count);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    // initial | singles | prefixes | singles | ...: ends when no parent has a candidate
    for (uint32_t phase = PH_INIT;; phase = phase == PH_SINGLES ? PH_PREFIXES : PH_SINGLES) {
      e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_b, widen_iter(k.cnt, Widen{}), offsets, (int64_t)(count + 1), st);
      if (e != hipSuccess) break;
      uint64_t total = 0;
      if ((e = hipMemcpyAsync(&total, offsets + count, sizeof(total), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;
      if (total == 0) break;
      const uint64_t blocks = (total + 63u) / 64u;
      if (blocks > 0x7FFFFFFFull) {               // (beyond one grid, and beyond any device's memory)
        rc = PXB_E_OOM;
        break;
      }
      const bool keep = phase != PH_SINGLES;      // the accepted candidate's send counts and result are needed
      const size_t held_b = pad256((size_t)total);
      const size_t cs_b = keep ? pad256((size_t)(total * k.n_links * 2u)) : 0, cr_b = keep ? (size_t)(total * 16u) : 0;
      char* lb = nullptr;
      if ((rc = pxw::scratch(dev, held_b + cs_b + cr_b, st, reinterpret_cast<void**>(&lb)))) break;
      c.total = total;
      c.prefix = phase == PH_PREFIXES;
      c.held = reinterpret_cast<uint8_t*>(lb);
      c.csent = keep ? reinterpret_cast<uint16_t*>(lb + held_b) : nullptr;
      c.cres = keep ? reinterpret_cast<uint4*>(lb + held_b + cs_b) : nullptr;
      hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64), 0, st, c);
      if ((e = hipGetLastError()) == hipSuccess) {
        k.phase = phase;
        k.held = c.held;
        k.csent = c.csent;
        k.cres = c.cres;
        hipLaunchKernelGGL(shrink_select_kernel, parents, dim3(64), 0, st, k);
        e = hipGetLastError();
      }
      const hipError_t f = hipFreeAsync(lb, st);  // (stream-ordered: after the launches above)
      if (e == hipSuccess) e = f;
      if (e != hipSuccess) break;
    }
    if (e != hipSuccess || rc) break;
    const ShrOut o{d_status, d_n_faults, d_launches, d_sent, reinterpret_cast<uint4*>(d_results), d_signature};
    hipLaunchKernelGGL(shrink_finish_kernel, parents, dim3(64), 0, st, k, o);
    if ((e = hipGetLastError()) != hipSuccess) break;
    e = hipMemcpyAsync(d_rows, k.rows, (size_t)(count * k.stride), hipMemcpyDeviceToDevice, st);
  } while (0);
  const hipError_t f = hipFreeAsync(buf, st);
  if (e == hipSuccess) e = f;
  return rc ? rc : (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

int pxb_shrink_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                     uint32_t flag_mask, uint32_t max_launches, uint32_t* status, uint32_t* n_faults,
                     uint32_t* launches, uint16_t* sent, pxb_result* results, uint64_t* signature) {
  using namespace pxsh;
  shr_ptr fn = nullptr;
  if (int rc = validate(cfg, rows, count, depth, flag_mask, max_launches, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) return PXB_OK;
  const uint64_t NL = 2u * cfg->n_proposers * cfg->n_acceptors;
  pxb::StagePlan plan;                            // rows | ids | status | faults | launches | sent | results | signature
  const pxb::StageRegion r_rows = plan.add(script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count);
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), count);
  const pxb::StageRegion r_st = plan.add(sizeof(uint32_t), count), r_nf = plan.add(sizeof(uint32_t), count);
  const pxb::StageRegion r_la = plan.add(sizeof(uint32_t), count), r_sent = plan.add(NL * sizeof(uint16_t), count);
  const pxb::StageRegion r_res = plan.add(sizeof(pxb_result), count), r_sig = plan.add(sizeof(uint64_t), count);
  Staging S(plan);
  uint8_t* const d_rows = S.ptr<uint8_t>(r_rows);
  if (ids) {
    S.up(r_ids, ids, count);
    if (S.ok()) S.note(pxb_schedule_extract_device(cfg, S.ptr<uint64_t>(r_ids), count, depth, d_rows, nullptr));
  } else {
    S.up(r_rows, rows, count);
  }
  // (an output that was not asked for: null, and the finish kernel does not store it)
  if (S.ok())
    S.note(pxb_shrink_batch_device(cfg, d_rows, count, depth, flag_mask, max_launches, S.ptr<uint32_t>(r_st, status),
                                   S.ptr<uint32_t>(r_nf, n_faults), S.ptr<uint32_t>(r_la, launches),
                                   S.ptr<uint16_t>(r_sent, sent), S.ptr<pxb_result>(r_res, results),
                                   S.ptr<uint64_t>(r_sig, signature), nullptr));
  S.down(r_rows, rows, count);
  S.down(r_st, status, count);
  S.down(r_nf, n_faults, count);
  S.down(r_la, launches, count);
  S.down(r_sent, sent, count);
  S.down(r_res, results, count);
  S.down(r_sig, signature, count);
  return S.finish();
}

}  // extern "C"
#endif  // PXB_SHR_P == 1
