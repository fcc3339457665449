// paxos_cover.hip — handler-path coverage of scripted rows and id ranges
// (include/paxos_batch.h, docs/SEMANTICS.md §14): pxb_cover, pxb_cover_range.
//
// The lane kernel is paxos_events.hip's with CoverLane (cover_core.h) in
// EventLane's place: lane l of block b runs row 64 b + l to its end and folds
// its events into the row's mask in registers.  The wave then reduces into the
// call's pxb_cover_summary: per class one ballot and popcount, and, where the
// wave has the class at all, a wave minimum of (steps, lane) and one atomic add
// and one atomic minimum of the key (steps << 32) | row index.  Integer adds
// and minima only, so the summary is the same whatever order the waves end in.
// While a call accumulates, witness[b] holds that key; a 32-thread kernel
// behind the lanes splits it into witness[b] and witness_steps[b].
//
// The range form runs the plain instances first + i as all-keep rows at depth 0
// a chunk at a time: a dense kernel writes the chunk's rows, the lane kernel
// gives the chunk's masks, status and summary, a 32-thread kernel merges that
// summary into the call's (a later chunk replaces a witness only with strictly
// fewer steps, so ties stay with the lowest i), and, with a query, hipCUB's
// select over the chunk's indices compacts the matches in ascending i behind
// those of the earlier chunks.  Nothing is read back between chunks.
//
// Built as three units by proposer count (-DPXB_COV_P=1|2|3), as the events
// kernels are; the unit of P = 1 also holds the dense kernels and the entry
// points.  The shapes are lane_shapes.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "cover_core.h"
#include "lane_shapes.h"

#ifndef PXB_COV_P
#error "PXB_COV_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct CovParams {
  EvParams p;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t count;
  uint32_t depth;
  uint32_t* masks;                  // nullable
  uint32_t* status;                 // nullable
  uint4* res;                       // nullable
  pxb_cover_summary* sum;           // nullable; witness[b]: the key while the call accumulates
};

// the smallest v of the wave's lanes, in every lane
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_cover_kernel(CovParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, EventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * 64u, i = i0 + lane;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  const bool in = i < k.count;
  bool run = in;
  if (run) {
    const uint32_t st = script_begin(L, k.p, k.depth, k.rows + i * k.stride);
    if (st != PXB_TRACE_OK) {       // a malformed row: not run
      E.status = st;
      run = false;
    }
  }
  script_run(L, E, k.p, run);
  const bool ok = in & (E.status == PXB_TRACE_OK);
  const uint32_t m = ok ? E.mask : 0u;
  if (in) {
    if (k.masks) k.masks[i] = m;
    if (k.status) k.status[i] = E.status;
    if (k.res) k.res[i] = make_uint4(E.res[0], E.res[1], E.res[2], E.res[3]);
  }
  if (k.sum == nullptr) return;     // (wave-uniform)
  // ---- the wave's reduction: one lane issues the atomics ----
  const bool lead = lane == 0u;
  const uint32_t n_ok = (uint32_t)__popcll(__ballot(ok));
  const uint32_t n_bail = (uint32_t)__popcll(__ballot(in & (E.status == PXB_TRACE_BAILED)));
  const uint32_t n_bad = (uint32_t)__popcll(__ballot(in & (E.status == PXB_SCRIPT_BAD)));
  if (lead) {
    if (n_ok) atomicAdd((unsigned long long*)&k.sum->rows_ok, (unsigned long long)n_ok);
    if (n_bail) atomicAdd((unsigned long long*)&k.sum->rows_bailed, (unsigned long long)n_bail);
    if (n_bad) atomicAdd((unsigned long long*)&k.sum->rows_bad, (unsigned long long)n_bad);
  }
  // (steps <= 4095: steps and the lane in one word order as (steps, row index) does within the wave)
  const uint32_t key = ((E.res[3] >> 16) << 6) | lane;
#pragma unroll 1
  for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b) {
    const bool has = ((m >> b) & 1u) != 0u;
    const unsigned long long bal = __ballot(has);
    if (bal == 0ull) continue;      // (wave-uniform: no row of the wave has the class)
    const uint32_t kmin = wave_min(has ? key : 0xFFFFFFFFu);
    if (lead) {
      atomicAdd((unsigned long long*)&k.sum->count[b], (unsigned long long)__popcll(bal));
      atomicMin((unsigned long long*)&k.sum->witness[b], ((unsigned long long)(kmin >> 6) << 32) | (i0 + (kmin & 63u)));
    }
  }
}

typedef void (*cov_ptr)(CovParams);
struct CovFamily {                  // (lane_shapes.h)
  typedef cov_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_cover_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(CovFamily, PXB_COV_P)

}  // namespace ev
}  // namespace pxb

#if PXB_COV_P == 1
#include "host_util.h"

namespace pxcv {
using namespace pxb::ev;
using namespace pxb::host;

constexpr uint64_t DEFAULT_CHUNK = 1ull << 20;

// 32 threads, thread b: the empty summary, in its final form (accumulate = false)
// or with the keys' identity in witness[] for the lane kernel's minima
__global__ __launch_bounds__(32) void cover_init_kernel(pxb_cover_summary* s) {
  const uint32_t b = threadIdx.x;
  s->count[b] = 0ull;
  s->witness[b] = ~0ull;
  s->witness_steps[b] = 0xFFFFFFFFu;
  if (b == 0u) {
    s->rows_ok = s->rows_bailed = s->rows_bad = s->n_matches = 0ull;
    s->union_mask = s->reserved = 0u;
  }
}

// 32 threads behind the lane kernel: key -> (witness, witness_steps), the union
__global__ __launch_bounds__(32) void cover_finish_kernel(pxb_cover_summary* s) {
  const uint32_t b = threadIdx.x;
  const bool has = s->count[b] != 0ull;
  const uint64_t key = s->witness[b];
  s->witness[b] = has ? (key & 0xFFFFFFFFull) : ~0ull;
  s->witness_steps[b] = has ? (uint32_t)(key >> 32) : 0xFFFFFFFFu;
  const unsigned long long bal = __ballot(has);
  if (b == 0u) s->union_mask = (uint32_t)bal;
}

// 32 threads: the finished summary c of the chunk that starts at id `id0` into the call's
__global__ __launch_bounds__(32) void cover_merge_kernel(pxb_cover_summary* s, const pxb_cover_summary* c, uint64_t id0) {
  const uint32_t b = threadIdx.x;
  s->count[b] += c->count[b];
  if (c->count[b] != 0ull && c->witness_steps[b] < s->witness_steps[b]) {   // (strictly: ties stay with the lower i)
    s->witness_steps[b] = c->witness_steps[b];
    s->witness[b] = id0 + c->witness[b];
  }
  if (b == 0u) {
    s->rows_ok += c->rows_ok;
    s->rows_bailed += c->rows_bailed;
    s->rows_bad += c->rows_bad;
    s->union_mask |= c->union_mask;
  }
}

// the all-keep depth-0 rows of ids id0 + i, i < n, one thread per 8-byte word:
// base, n_proposers = 0 and reserved = 0, then keep bytes up to 16 + 4 N, zeros to the stride
__global__ __launch_bounds__(256) void cover_fill_kernel(uint64_t* rows, uint32_t wpr, uint32_t keep_end, uint64_t id0,
                                                         uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n * wpr) return;
  const uint64_t i = t / wpr;
  const uint32_t w = (uint32_t)(t - i * wpr);
  uint64_t v = id0 + i;
  if (w != 0u) {
    v = 0ull;
    for (uint32_t j = 0; j < 8u; ++j) {
      const uint32_t off = 8u * w + j;
      v |= (uint64_t)((off >= 10u && off < keep_end) ? SCR_KEEP8 : 0u) << (8u * j);
    }
  }
  rows[t] = v;
}

struct MatchOp {
  const uint32_t* masks;
  const uint32_t* status;
  uint32_t all, any, none;
  __host__ __device__ __forceinline__ bool operator()(const uint32_t& i) const {
    return status[i] == PXB_TRACE_OK && cover_match(masks[i], all, any, none);
  }
};

// the chunk's selected indices (ascending) behind the call's matches so far
__global__ __launch_bounds__(256) void cover_append_kernel(const uint32_t* sel, const uint32_t* n_sel,
                                                           const uint32_t* masks, uint64_t id0,
                                                           const pxb_cover_summary* s, uint64_t* ids, uint32_t* mm,
                                                           uint64_t max_matches) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= *n_sel) return;
  const uint64_t pos = s->n_matches + j;
  if (pos >= max_matches) return;
  const uint32_t i = sel[j];
  ids[pos] = id0 + i;
  if (mm) mm[pos] = masks[i];
}
__global__ void cover_count_kernel(pxb_cover_summary* s, const uint32_t* n_sel) { s->n_matches += *n_sel; }

// the config rules every form shares
static int validate_cfg(const pxb_config* cfg, cov_ptr* fn) {
  if (!cfg || !trace_config_ok(cfg) || (cfg->flags & PXB_CFG_TRACE_PRODUCTION)) return PXB_E_INVAL;
  *fn = lane_kernel<CovFamily>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}
static int validate_rows(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth, cov_ptr* fn) {
  if (!cfg || (count && !rows) || count > MAX_COUNT || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  return validate_cfg(cfg, fn);
}

// the launches of one rows call on st: the summary's start, the lanes, the summary's end
static hipError_t launch(cov_ptr fn, const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                         uint32_t* d_masks, uint32_t* d_status, pxb_result* d_results, pxb_cover_summary* d_summary,
                         hipStream_t st) {
  hipError_t e = hipSuccess;
  if (d_summary) {
    hipLaunchKernelGGL(cover_init_kernel, dim3(1), dim3(32), 0, st, d_summary);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (count) {
    CovParams k{};
    k.p = make_params(cfg);
    k.p.first_instance = 0;
    k.rows = d_rows;
    k.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
    k.count = count;
    k.depth = depth;
    k.masks = d_masks;
    k.status = d_status;
    k.res = reinterpret_cast<uint4*>(d_results);
    k.sum = d_summary;
    hipLaunchKernelGGL(fn, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (d_summary) {
    hipLaunchKernelGGL(cover_finish_kernel, dim3(1), dim3(32), 0, st, d_summary);
    e = hipGetLastError();
  }
  return e;
}

static void empty_summary(pxb_cover_summary* s) {
  memset(s, 0, sizeof *s);
  for (int b = 0; b < 32; ++b) {
    s->witness[b] = ~0ull;
    s->witness_steps[b] = 0xFFFFFFFFu;
  }
}

}  // namespace pxcv

extern "C" {

int pxb_cover_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth, uint32_t* d_masks,
                     uint32_t* d_status, pxb_result* d_results, pxb_cover_summary* d_summary, void* stream) {
  using namespace pxcv;
  cov_ptr fn = nullptr;
  if (int rc = validate_rows(cfg, d_rows, count, depth, &fn)) return rc;
  // (the results move as 16-byte words, the summary's counts and keys as 8-byte ones)
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_masks & 3u) || ((uintptr_t)d_status & 3u) ||
      ((uintptr_t)d_results & 15u) || ((uintptr_t)d_summary & 7u))
    return PXB_E_INVAL;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  return hip_rc(launch(fn, cfg, d_rows, count, depth, d_masks, d_status, d_results, d_summary, (hipStream_t)stream));
}

// the HOST-buffer form: device copies of the buffers (host_stage.h) around the device form
int pxb_cover(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth, uint32_t* masks,
              uint32_t* status, pxb_result* results, pxb_cover_summary* summary) {
  using namespace pxcv;
  cov_ptr fn = nullptr;
  if (int rc = validate_rows(cfg, rows, count, depth, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) {
    if (summary) empty_summary(summary);
    return PXB_OK;
  }
  pxb::StagePlan plan;                            // rows | masks | status | results | summary
  const pxb::StageRegion r_rows = plan.add(script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count);
  const pxb::StageRegion r_m = plan.add(sizeof(uint32_t), count), r_st = plan.add(sizeof(uint32_t), count);
  const pxb::StageRegion r_res = plan.add(sizeof(pxb_result), count), r_sum = plan.add(sizeof(pxb_cover_summary), 1);
  Staging S(plan);
  S.up(r_rows, rows, count);
  if (S.ok())
    S.note(pxb_cover_device(cfg, S.ptr<uint8_t>(r_rows), count, depth, S.ptr<uint32_t>(r_m, masks),
                            S.ptr<uint32_t>(r_st, status), S.ptr<pxb_result>(r_res, results),
                            S.ptr<pxb_cover_summary>(r_sum, summary), nullptr));
  S.down(r_m, masks, count);
  S.down(r_st, status, count);
  S.down(r_res, results, count);
  S.down(r_sum, summary, 1);
  return S.finish();
}

int pxb_cover_range(const pxb_config* cfg, uint64_t first, uint64_t count, uint64_t chunk, const pxb_cover_query* q,
                    uint64_t* match_ids, uint32_t* match_masks, uint64_t max_matches, pxb_cover_summary* summary) {
  using namespace pxcv;
  cov_ptr fn = nullptr;
  if (int rc = validate_cfg(cfg, &fn)) return rc;
  if (chunk > MAX_COUNT || (q && q->reserved != 0u) || (q && max_matches && !match_ids)) return PXB_E_INVAL;
  if (device_count() == 0) return PXB_E_NODEV;
  pxb_cover_summary total;
  empty_summary(&total);
  if (count == 0) {
    if (summary) *summary = total;
    return PXB_OK;
  }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (chunk == 0) chunk = DEFAULT_CHUNK;
  if (chunk > count) chunk = count;
  const uint64_t list = q ? max_matches : 0;
  const uint32_t N = cfg->n_acceptors;
  const uint64_t stride = script_stride(cfg->n_proposers, N, 0);
  const uint32_t wpr = (uint32_t)(stride / 8u);
  // the select's scratch, for the largest chunk
  size_t need = 0;
  if (q) {
    const hipError_t e = hipcub::DeviceSelect::If(nullptr, need, hipcub::CountingInputIterator<uint32_t>(0u),
                                                  (uint32_t*)nullptr, (uint32_t*)nullptr, (int)chunk,
                                                  MatchOp{nullptr, nullptr, 0u, 0u, 0u}, (hipStream_t) nullptr);
    if (e != hipSuccess) return hip_fail(e);
  }
  pxb::StagePlan plan;                            // match ids | match masks | the call's summary | the chunk's
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), list), r_mm = plan.add(sizeof(uint32_t), list);
  const pxb::StageRegion r_sum = plan.add(sizeof(pxb_cover_summary), 1), r_csum = plan.add(sizeof(pxb_cover_summary), 1);
  Staging S(plan);
  if (!S.ok()) return S.finish();
  // one chunk from the stream-ordered pool: rows | masks | status | selected indices | their count | the select's scratch
  const size_t rows_b = pad256((size_t)(chunk * stride)), word_b = pad256((size_t)(chunk * sizeof(uint32_t)));
  const size_t sel_b = q ? word_b : 0, nsel_b = q ? 256 : 0;
  void* buf = nullptr;
  if (int rc = pxw::scratch(dev, rows_b + 2 * word_b + sel_b + nsel_b + pad256(need), nullptr, &buf)) {
    S.note(rc);
    return S.finish();
  }
  char* const b = reinterpret_cast<char*>(buf);
  uint64_t* const d_rows = reinterpret_cast<uint64_t*>(b);
  uint32_t* const d_masks = reinterpret_cast<uint32_t*>(b + rows_b);
  uint32_t* const d_status = reinterpret_cast<uint32_t*>(b + rows_b + word_b);
  uint32_t* const d_sel = reinterpret_cast<uint32_t*>(b + rows_b + 2 * word_b);
  uint32_t* const d_nsel = reinterpret_cast<uint32_t*>(b + rows_b + 2 * word_b + sel_b);
  void* const d_tmp = b + rows_b + 2 * word_b + sel_b + nsel_b;
  pxb_cover_summary* const d_sum = S.ptr<pxb_cover_summary>(r_sum);
  pxb_cover_summary* const d_csum = S.ptr<pxb_cover_summary>(r_csum);
  uint64_t* const d_ids = S.ptr<uint64_t>(r_ids);
  uint32_t* const d_mm = S.ptr<uint32_t>(r_mm, match_masks);
  const hipStream_t st = nullptr;
  hipError_t e = hipSuccess;
  hipLaunchKernelGGL(cover_init_kernel, dim3(1), dim3(32), 0, st, d_sum);
  e = hipGetLastError();
  for (uint64_t base = 0; e == hipSuccess && base < count; base += chunk) {
    const uint64_t n = count - base < chunk ? count - base : chunk, id0 = first + base;
    hipLaunchKernelGGL(cover_fill_kernel, dim3((unsigned)((n * wpr + 255u) / 256u)), dim3(256), 0, st, d_rows, wpr,
                       SCR_HDR + 4u * N, id0, n);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = launch(fn, cfg, reinterpret_cast<const uint8_t*>(d_rows), n, 0u, d_masks, d_status, nullptr, d_csum, st)) !=
        hipSuccess)
      break;
    hipLaunchKernelGGL(cover_merge_kernel, dim3(1), dim3(32), 0, st, d_sum, d_csum, id0);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if (q) {
      size_t tb = need;
      e = hipcub::DeviceSelect::If(d_tmp, tb, hipcub::CountingInputIterator<uint32_t>(0u), d_sel, d_nsel, (int)n,
                                   MatchOp{d_masks, d_status, q->all_mask, q->any_mask, q->none_mask}, st);
      if (e != hipSuccess) break;
      if (list) {
        hipLaunchKernelGGL(cover_append_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, d_sel, d_nsel,
                           d_masks, id0, d_sum, d_ids, d_mm, list);
        if ((e = hipGetLastError()) != hipSuccess) break;
      }
      hipLaunchKernelGGL(cover_count_kernel, dim3(1), dim3(1), 0, st, d_sum, d_nsel);
      e = hipGetLastError();
    }
  }
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  S.note(e);
  S.down(r_sum, &total, 1);
  if (S.ok()) {
    const uint64_t m = total.n_matches < list ? total.n_matches : list;
    S.down(r_ids, match_ids, m);
    S.down(r_mm, match_masks, m);
    if (summary) *summary = total;
  }
  return S.finish();
}

}  // extern "C"
#endif  // PXB_COV_P == 1
