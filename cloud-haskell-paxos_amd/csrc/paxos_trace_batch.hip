// paxos_trace_batch.hip — pxb_trace_batch: many instances through the per-lane
// state machine (paxos_ev.h) in one launch, 64 per wave, with the records a
// selection keeps written contiguously in the order of the id list.
//
// Ordered compaction in the library's usual shape (wire codec, query): two
// passes of one kernel with hipCUB's exclusive sum between them, and no block
// that waits for another:
//   1. count   lane l of block b runs ids[64 b + l] to its end and counts the
//              visited steps inside the window; writes the count (scratch), the
//              status and the result;
//   2. scan    exclusive sum of min(count, tail) (count + 1 entries: the last
//              is the total) into d_offsets;
//   3. write   the same kernel with records on: the state machine is
//              deterministic, so the re-run visits the same steps; in-window
//              record j of instance i goes to d_offsets[i] + j - skip_i.  A
//              block whose first offset is at or past `capacity` exits at once,
//              a lane stops once none of its later records can be kept.
// The wave stays together: lanes that have finished idle, and the loop's back
// edge is one ballot (EvLane::step's any_lane ballots then see the live lanes).
//
// Built as three units by proposer count (-DPXB_TRB_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the entry points.  What
// one lane does around its run is TrbParams::begin / finish (paxos_trace_core.h),
// which tests/native/trace_host.cpp runs on the host; the shapes are
// lane_shapes.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "lane_shapes.h"
#include "paxos_ev_kernel.h"
#include "paxos_trace_core.h"

#ifndef PXB_TRB_P
#error "PXB_TRB_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

// the shapes and pools of paxos_trace_kernel
template <int PM, int N, int W, bool EARLY, bool LG = false>
__global__ __launch_bounds__(64) void paxos_trace_batch_kernel(TrbParams k) {
  constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using S = Shape<PM, N, POOL, W, false, LG>;
  using Lane = EvLane<PM, N, POOL, W, false, LdsMem, EARLY, LG>;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * 64u, i = i0 + lane;
  if (k.out != nullptr && k.offsets[i0] >= k.capacity) return;   // (wave-uniform; offsets ascend: nothing of this block fits)
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  TraceLane<Lane> T;
  bool run = k.begin(L, T, i);
  while (any_lane(run)) {
    if (run) run = T.iter(L, k.p);
  }
  k.finish(L, T, i);
}

typedef void (*trb_ptr)(TrbParams);
// two families (lane_shapes.h): the production draws' kernels and the others
template <bool EARLY>
struct TrbFamily {
  typedef trb_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_trace_batch_kernel<PM, N, W, EARLY, LG>; }
};
PXB_LANE_UNIT(TrbFamily<true>, PXB_TRB_P)
PXB_LANE_UNIT(TrbFamily<false>, PXB_TRB_P)

}  // namespace ev
}  // namespace pxb

#if PXB_TRB_P == 1
#include "host_util.h"

namespace pxtb {
using namespace pxb::ev;
using namespace pxb::host;

// the scan's input: what the selection keeps of an instance's in-window records
struct Kept {
  uint32_t tail;
  __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& c) const { return trace_kept(c, tail); }
};
typedef hipcub::TransformInputIterator<uint64_t, Kept, const uint32_t*> kept_iter;

// the argument rules of both forms; *fn: the shape's kernel
int validate(const pxb_config* cfg, const void* ids, uint64_t count, const pxb_trace_sel* sel, const void* records,
             uint64_t capacity, const void* offsets, trb_ptr* fn) {
  if (!cfg || !offsets || (count && !ids) || count > MAX_COUNT) return PXB_E_INVAL;
  if (sel && sel->reserved != 0u) return PXB_E_INVAL;
  if (!records && capacity) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  *fn = (cfg->flags & PXB_CFG_TRACE_PRODUCTION) ? lane_kernel<TrbFamily<true>>(cfg) : lane_kernel<TrbFamily<false>>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

hipError_t scan_bytes(uint64_t count, hipStream_t st, size_t* need) {
  *need = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *need, kept_iter(nullptr, Kept{0u}), (uint64_t*)nullptr,
                                          (int64_t)(count + 1), st);
}

// count pass + scan (phase 1), write pass (phase 2) over cnt (count + 1 words) and the scan's tmp
hipError_t launch(trb_ptr fn, const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, const pxb_trace_sel* sel,
                  pxb_trace_step* d_records, uint64_t capacity, uint64_t* d_offsets, uint32_t* d_status,
                  pxb_result* d_results, hipStream_t st, uint32_t* cnt, void* tmp, size_t need, int phases) {
  TrbParams k{};
  k.p = make_params(cfg);
  k.p.first_instance = 0;
  k.ids = d_ids;
  k.count = count;
  k.smin = sel ? sel->step_min : 0u;
  k.smax = sel ? sel->step_max : 0xFFFFFFFFu;
  k.tail = sel ? sel->tail : 0u;
  k.cnt = cnt;
  k.offsets = d_offsets;
  k.capacity = capacity;
  const dim3 grid((unsigned)((count + 63) / 64));
  hipError_t e = hipSuccess;
  if (phases & 1) {
    if ((e = hipMemsetAsync(cnt + count, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
    k.out = nullptr;
    k.status = d_status;
    k.res = reinterpret_cast<uint4*>(d_results);
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, need, kept_iter(cnt, Kept{k.tail}), d_offsets, (int64_t)(count + 1), st);
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && capacity && d_records) {
    k.out = d_records;
    k.status = nullptr;
    k.res = nullptr;
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace pxtb

extern "C" {

int pxb_trace_batch_device(const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, const pxb_trace_sel* sel,
                           pxb_trace_step* d_records, uint64_t capacity, uint64_t* d_offsets, uint32_t* d_status,
                           pxb_result* d_results, void* stream) {
  using namespace pxtb;
  trb_ptr fn = nullptr;
  if (int rc = validate(cfg, d_ids, count, sel, d_records, capacity, d_offsets, &fn)) return rc;
  // (the records move as 4-byte words, the results as 16-byte ones)
  if (((uintptr_t)d_ids & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_records & 3u) ||
      ((uintptr_t)d_status & 3u) || ((uintptr_t)d_results & 15u))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) {
    const hipError_t e = hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), st);
    return (e == hipSuccess) ? PXB_OK : hip_fail(e);
  }
  size_t need = 0;
  if (hipError_t e = scan_bytes(count, st, &need)) return hip_fail(e);
  const size_t cnt_b = pad256((count + 1) * sizeof(uint32_t));
  void* buf = nullptr;
  if (int rc = pxw::scratch(dev, cnt_b + need, st, &buf)) return rc;
  hipError_t e = launch(fn, cfg, d_ids, count, sel, d_records, capacity, d_offsets, d_status, d_results, st,
                        reinterpret_cast<uint32_t*>(buf), reinterpret_cast<char*>(buf) + cnt_b, need, 3);
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

int pxb_trace_batch(const pxb_config* cfg, const uint64_t* ids, uint64_t count, const pxb_trace_sel* sel,
                    pxb_trace_step* records, uint64_t capacity, uint64_t* offsets, uint32_t* status,
                    pxb_result* results, uint64_t* n_records) {
  using namespace pxtb;
  trb_ptr fn = nullptr;
  if (int rc = validate(cfg, ids, count, sel, records, capacity, offsets, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  size_t need = 0;
  if (count)
    if (hipError_t e = scan_bytes(count, 0, &need)) return hip_fail(e);
  pxb::StagePlan plan;                            // counts | the scan's | ids | offsets | status | results
  const pxb::StageRegion r_cnt = plan.add(sizeof(uint32_t), count + 1), r_tmp = plan.add(1, need);
  // the count pass and the scan once, then the write pass alone over their counts and offsets: not the
  // device form twice (the count pass stores no status or results that were not asked for)
  const auto pass = [&](Staging& S, const TraceBufs& d, pxb_trace_step* d_rec, uint64_t m, bool first) {
    return launch(fn, cfg, static_cast<uint64_t*>(d.in), count, sel, d_rec, m, d.off, first && status ? d.st : nullptr,
                  first && results ? d.res : nullptr, 0, S.ptr<uint32_t>(r_cnt), S.ptr<char>(r_tmp), need, first ? 1 : 2);
  };
  return trace_two_call(
      plan, ids, sizeof(uint64_t), count, records, capacity, offsets, status, results, n_records,
      [&](Staging& S, const TraceBufs& d) { return pass(S, d, nullptr, 0, true); },
      [&](Staging& S, const TraceBufs& d, pxb_trace_step* d_rec, uint64_t m) { return pass(S, d, d_rec, m, false); });
}

}  // extern "C"
#endif  // PXB_TRB_P == 1
