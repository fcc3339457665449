// shrink_driver.h — the batched shrinker's driver (include/paxos_batch.h,
// docs/SEMANTICS.md §11, §16): what pxb_shrink_batch_device (paxos_shrink.hip)
// and pxb_shrink_cover_batch_device (paxos_shrink_cover.hip) share behind their
// candidate kernels.  The parents' state between launches, three kernels and the
// host loop:
//   the select kernel, one 64-lane wave per parent: after the initial launch it
//     settles and enumerates the row (ballot + mbcnt ranks), after a singles
//     launch it compacts the held singles into the removable ranking, after a
//     prefix launch it takes the longest held prefix (ballot + clz), applies it
//     in place, settles and re-enumerates; the accepted candidate's result, and
//     its coverage mask where the launch has that column, go to the parent;
//   the finish kernel, one wave per parent: status, fault count, launches, send
//     counts, result, mask and the FNV-1a-64 signature;
//   a fill kernel for the first launch's counts.
// shrink_drive is parameterised by the candidate launch: the kernel, its
// parameters, the ShrParams among them that the loop fills in per launch, and
// (nullable) the parameter that takes the launch's per-candidate mask column.
// It reads one 8-byte candidate total per launch to size the next grid: the
// stream is synchronised once per launch.  No block waits for another; plain
// vector stores only.  Internal to the units that hold the entry points (the
// kernels have internal linkage: each such unit carries its own).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "host_util.h"
#include "paxos_trace_core.h"
#include "shrink_core.h"

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
  uint32_t* mask;                   // its coverage mask (null: the call has no masks)
  const uint8_t* held;              // the launch just run
  const uint16_t* csent;
  const uint4* cres;
  const uint32_t* cmask;            // (null with `mask`)
};

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {   // set bits of lanes before this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// The accepted row of parent i: neutralises the entries of rank <= best (none:
// NO_PREFIX), settles against `sent`, and rewrites the table as the fault
// ranking of the new row.  Returns the fault count (wave-uniform).
__device__ inline uint32_t accept_and_enumerate(const ShrCtl& k, uint64_t i, const uint16_t* sent, uint32_t best) {
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
__device__ inline void decide(const ShrCtl& k, uint64_t i, uint32_t nf, uint32_t launches) {
  if (threadIdx.x != 0u) return;
  k.nf[i] = nf;
  k.launches[i] = launches;
  const bool done = nf == 0u, broke = launches + 2u > k.max_launches;
  k.state[i] = done ? PXB_SHRINK_MINIMAL : broke ? PXB_SHRINK_BUDGET : ACTIVE;
  k.cnt[i] = (done | broke) ? 0u : nf;
}

__device__ inline void stop(const ShrCtl& k, uint64_t i, uint32_t status, uint32_t launches) {
  if (threadIdx.x != 0u) return;
  k.state[i] = status;
  k.launches[i] = launches;
  k.cnt[i] = 0u;
}

// candidate c of the launch just run becomes parent i's accepted run: its result and mask
__device__ __forceinline__ void take(const ShrCtl& k, uint64_t i, uint64_t c) {
  if (threadIdx.x != 0u) return;
  k.res[i] = k.cres[c];
  if (k.cmask) k.mask[i] = k.cmask[c];
}

static __global__ __launch_bounds__(64) void shrink_select_kernel(ShrCtl k) {
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
    take(k, i, off);                              // (NOT_INPUT and TOO_MANY report the given row's)
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
    take(k, i, off + best);
  }
  const uint64_t cand = off + (best == NO_PREFIX ? 0u : best);
  const uint16_t* const sent = k.csent + cand * k.n_links;
  const uint32_t nf = accept_and_enumerate(k, i, sent, best);
  if (lane < k.n_links) k.psent[i * k.n_links + lane] = sent[lane];
  decide(k, i, nf, launches);
}

// the call's per-row outputs (every one nullable)
struct ShrOut {
  uint32_t* status;
  uint32_t* n_faults;
  uint32_t* launches;
  uint16_t* sent;
  uint4* results;
  uint64_t* signature;
  uint32_t* masks;                  // (only with ShrCtl::mask)
};
inline bool shrink_aligned(const void* d_rows, const ShrOut& o) {
  return !(((uintptr_t)d_rows & 7u) || ((uintptr_t)o.status & 3u) || ((uintptr_t)o.n_faults & 3u) ||
           ((uintptr_t)o.launches & 3u) || ((uintptr_t)o.sent & 1u) || ((uintptr_t)o.results & 15u) ||
           ((uintptr_t)o.signature & 7u) || ((uintptr_t)o.masks & 3u));
}

static __global__ __launch_bounds__(64) void shrink_finish_kernel(ShrCtl k, ShrOut o) {
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
  if (o.masks) o.masks[i] = k.mask[i];
}

// the first launch: one candidate per parent (the row itself: no rank selects anything)
static __global__ __launch_bounds__(256) void shrink_first_counts_kernel(uint32_t* cnt, uint64_t count) {
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= count; i += step) cnt[i] = i < count ? 1u : 0u;
}

// the argument rules every shrinking call shares (the outcome flags and the kernel of the shape are the caller's)
inline int shrink_validate(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth,
                           uint32_t max_launches) {
  if (!cfg || (count && !rows) || count > MAX_COUNT || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  if (max_launches == 0u || !trace_config_ok(cfg)) return PXB_E_INVAL;
  return PXB_OK;
}

// The rounds over d_rows (validated, aligned, count > 0) on the device `dev`.
// fn(c) is the candidate launch; `core` is the ShrParams inside c, of which the
// caller has set flag_mask and the loop sets the rest; `cmask`, where not null,
// is the pointer inside c that takes the launch's per-candidate mask column
// (total words, allocated in the initial and the prefix launches, null in the
// singles'), which the select kernel then carries to the parent as it carries
// cres, and o.masks is written.
template <class Params>
int shrink_drive(const pxb_config* cfg, uint8_t* d_rows, uint64_t count, uint32_t depth, uint32_t max_launches,
                 void (*fn)(Params), Params& c, ShrParams& core, uint32_t** cmask, const ShrOut& o, int dev,
                 hipStream_t st) {
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
  // the call's scratch: work rows | tables | sent | counts | offsets | state | launches | faults | results | masks | scan
  // (the rows are shrunk in a copy and written back at the end: a failed call writes nothing)
  const size_t rows_b = pad256((size_t)(count * k.stride)), tab_b = pad256((size_t)(count * k.tstride * 2u));
  const size_t sent_b = pad256((size_t)(count * k.n_links * 2u)), cnt_b = pad256((size_t)((count + 1) * 4u));
  const size_t off_b = pad256((size_t)((count + 1) * 8u)), w_b = pad256((size_t)(count * 4u));
  const size_t res_b = pad256((size_t)(count * 16u)), mask_b = cmask ? w_b : 0;
  char* buf = nullptr;
  if (int rc = pxw::scratch(dev, rows_b + tab_b + sent_b + cnt_b + off_b + 3u * w_b + res_b + mask_b + scan_b, st,
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
  k.mask = cmask ? reinterpret_cast<uint32_t*>(q) : nullptr, q += mask_b;
  void* const scan_tmp = q;

  core.p = make_params(cfg);
  core.p.first_instance = 0;
  core.rows = k.rows;
  core.stride = k.stride;
  core.table = k.table;
  core.tstride = k.tstride;
  core.offsets = offsets;
  core.count = count;
  core.depth = depth;

  const dim3 parents((unsigned)count);
  hipError_t e = hipSuccess;
  int rc = PXB_OK;
  do {
    if ((e = hipMemcpyAsync(k.rows, d_rows, (size_t)(count * k.stride), hipMemcpyDeviceToDevice, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.table, 0xFF, (size_t)(count * k.tstride * 2u), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.psent, 0, sent_b, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(k.state, 0xFF, w_b, st)) != hipSuccess) break;        // ACTIVE
    if ((e = hipMemsetAsync(k.launches, 0, 2u * w_b + res_b + mask_b, st)) != hipSuccess) break;
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
      // the accepted candidate's send counts, result and mask are needed
      const bool keep = phase != PH_SINGLES;
      const size_t held_b = pad256((size_t)total);
      const size_t cs_b = keep ? pad256((size_t)(total * k.n_links * 2u)) : 0, cr_b = keep ? (size_t)(total * 16u) : 0;
      const size_t cm_b = (keep && cmask) ? (size_t)(total * 4u) : 0;
      char* lb = nullptr;
      if ((rc = pxw::scratch(dev, held_b + cs_b + cr_b + cm_b, st, reinterpret_cast<void**>(&lb)))) break;
      core.total = total;
      core.prefix = phase == PH_PREFIXES;
      core.held = reinterpret_cast<uint8_t*>(lb);
      core.csent = keep ? reinterpret_cast<uint16_t*>(lb + held_b) : nullptr;
      core.cres = keep ? reinterpret_cast<uint4*>(lb + held_b + cs_b) : nullptr;
      k.cmask = cm_b ? reinterpret_cast<uint32_t*>(lb + held_b + cs_b + cr_b) : nullptr;
      if (cmask) *cmask = const_cast<uint32_t*>(k.cmask);
      hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64), 0, st, c);
      if ((e = hipGetLastError()) == hipSuccess) {
        k.phase = phase;
        k.held = core.held;
        k.csent = core.csent;
        k.cres = core.cres;
        hipLaunchKernelGGL(shrink_select_kernel, parents, dim3(64), 0, st, k);
        e = hipGetLastError();
      }
      const hipError_t f = hipFreeAsync(lb, st);  // (stream-ordered: after the launches above)
      if (e == hipSuccess) e = f;
      if (e != hipSuccess) break;
    }
    if (e != hipSuccess || rc) break;
    hipLaunchKernelGGL(shrink_finish_kernel, parents, dim3(64), 0, st, k, o);
    if ((e = hipGetLastError()) != hipSuccess) break;
    e = hipMemcpyAsync(d_rows, k.rows, (size_t)(count * k.stride), hipMemcpyDeviceToDevice, st);
  } while (0);
  const hipError_t f = hipFreeAsync(buf, st);
  if (e == hipSuccess) e = f;
  return rc ? rc : (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

// The host-buffer form around a device form (validated, a device present, count
// > 0): the rows up, or the schedules of `ids` extracted on the device, then
// call(d_rows, d) over the device copies `d` of the outputs `h` that were asked
// for (the others null: the finish kernel does not store them), and those down.
// `masks`: the form has that column.
template <class Call>
int shrink_staged(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                  const ShrOut& h, bool masks, const Call& call) {
  const uint64_t NL = 2u * cfg->n_proposers * cfg->n_acceptors;
  pxb::StagePlan plan;                            // rows | ids | status | faults | launches | sent | results | signature | masks
  const pxb::StageRegion r_rows = plan.add(script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count);
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), count);
  const pxb::StageRegion r_st = plan.add(sizeof(uint32_t), count), r_nf = plan.add(sizeof(uint32_t), count);
  const pxb::StageRegion r_la = plan.add(sizeof(uint32_t), count), r_sent = plan.add(NL * sizeof(uint16_t), count);
  const pxb::StageRegion r_res = plan.add(sizeof(pxb_result), count), r_sig = plan.add(sizeof(uint64_t), count);
  const pxb::StageRegion r_m = plan.add(sizeof(uint32_t), masks ? count : 0u);
  Staging S(plan);
  uint8_t* const d_rows = S.ptr<uint8_t>(r_rows);
  if (ids) {
    S.up(r_ids, ids, count);
    if (S.ok()) S.note(pxb_schedule_extract_device(cfg, S.ptr<uint64_t>(r_ids), count, depth, d_rows, nullptr));
  } else {
    S.up(r_rows, rows, count);
  }
  const ShrOut d{S.ptr<uint32_t>(r_st, h.status),   S.ptr<uint32_t>(r_nf, h.n_faults), S.ptr<uint32_t>(r_la, h.launches),
                 S.ptr<uint16_t>(r_sent, h.sent),   S.ptr<uint4>(r_res, h.results),    S.ptr<uint64_t>(r_sig, h.signature),
                 S.ptr<uint32_t>(r_m, h.masks)};
  if (S.ok()) S.note(call(d_rows, d));
  S.down(r_rows, rows, count);
  S.down(r_st, h.status, count);
  S.down(r_nf, h.n_faults, count);
  S.down(r_la, h.launches, count);
  S.down(r_sent, h.sent, count);
  S.down(r_res, h.results, count);
  S.down(r_sig, h.signature, count);
  S.down(r_m, h.masks, count);
  return S.finish();
}

}  // namespace pxsh
