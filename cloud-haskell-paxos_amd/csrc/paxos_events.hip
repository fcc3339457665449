// paxos_events.hip — per-message handler events of scripted rows
// (include/paxos_batch.h, docs/SEMANTICS.md §13): pxb_trace_events.
//
// The lane kernel is paxos_script.hip's with the tapped draw source
// (events_core.h: EventDraws) and EventLane in TraceLane's place: lane l of
// block b runs row 64 b + l to its end.  The count pass writes the status, the
// result and the row's event count; hipCUB's exclusive sum gives d_offsets; the
// write pass runs the deterministic lanes again and stages each row's events,
// in the lane's own order, at its offset in a staging buffer of capacity + 256
// events; a dense kernel, one thread per staged event, then copies each event
// to its canonical place in d_events (event_place).  A row's step segment holds
// at most 246 events, so every segment that starts below `capacity` is whole in
// the staging buffer, and nothing at or past `capacity` is written.  Counts,
// the scan's scratch and the staging buffer come from the per-device
// stream-ordered pool on the caller's stream.  No block waits for another.
//
// Built as three units by proposer count (-DPXB_EVT_P=1|2|3), as the script
// kernels are; the unit of P = 1 also holds the reorder kernel and the entry
// points.  The shapes are lane_shapes.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "events_core.h"
#include "lane_shapes.h"

#ifndef PXB_EVT_P
#error "PXB_EVT_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct EvtParams {
  EvParams p;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t count;
  uint32_t depth;
  uint32_t smin, smax;
  uint32_t* cnt;                    // in-window events per row (count pass: out; write pass: in)
  const uint64_t* offsets;          // write pass: d_offsets
  pxb_trace_event* out;             // write pass: the staging buffer (count pass: null)
  uint64_t room;                    // write pass: the staging buffer's events
  uint32_t* status;                 // count pass, nullable
  uint4* res;                       // count pass, nullable
};

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_events_kernel(EvtParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, EventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * 64u, i = i0 + lane;
  const bool write = k.out != nullptr;
  if (write && k.offsets[i0] >= k.room) return;         // (wave-uniform; offsets ascend: nothing of this block fits)
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  L.e_acc = L.e_pin = false;
  EventLane<Lane> E;
  E.begin_count(k.smin, k.smax);
  bool run = i < k.count;
  if (run && write) {
    const uint32_t c = k.cnt[i];
    const uint64_t base = k.offsets[i];
    run = (c != 0u) & (base < k.room);
    if (run) E.begin_write(k.smin, k.smax, c, k.out + base, k.room - base);
  }
  if (run) {
    const uint32_t st = script_begin(L, k.p, k.depth, k.rows + i * k.stride);
    if (st != PXB_TRACE_OK) {       // a malformed row: not run
      E.status = st;
      run = false;
    }
  }
  script_run(L, E, k.p, run);
  if (!write && i < k.count) {
    k.cnt[i] = E.n;
    if (k.status) k.status[i] = E.status;
    if (k.res) k.res[i] = make_uint4(E.res[0], E.res[1], E.res[2], E.res[3]);
  }
}

typedef void (*evt_ptr)(EvtParams);
struct EvtFamily {                  // (lane_shapes.h)
  typedef evt_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_events_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(EvtFamily, PXB_EVT_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EVT_P == 1
#include "host_util.h"

namespace pxev {
using namespace pxb::ev;
using namespace pxb::host;

// the reorder: staged event t to its canonical place, a grid-stride loop over
// the staged events (offsets[count]: the call's total, on the device)
__global__ __launch_bounds__(256) void paxos_events_place_kernel(const pxb_trace_event* staging, uint64_t room,
                                                                 const uint64_t* offsets, uint64_t count,
                                                                 pxb_trace_event* out, uint64_t capacity) {
  const uint64_t total = offsets[count], staged = total < room ? total : room;
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < staged; t += step)
    event_place(staging, staged, offsets, count, t, out, capacity);
}

// the argument rules both forms share
static int validate(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth, const pxb_trace_sel* sel,
                    const void* events, uint64_t capacity, const void* offsets, evt_ptr* fn) {
  if (!cfg || (count && !rows) || count > MAX_COUNT || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  if (!offsets || (sel && (sel->reserved != 0u || sel->tail != 0u)) || (!events && capacity)) return PXB_E_INVAL;
  if (cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<EvtFamily>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

static hipError_t scan_bytes(uint64_t count, hipStream_t st, size_t* need) {
  *need = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *need, widen_iter(nullptr, Widen{}), (uint64_t*)nullptr,
                                          (int64_t)(count + 1), st);
}

}  // namespace pxev

extern "C" {

int pxb_trace_events_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                            const pxb_trace_sel* sel, pxb_trace_event* d_events, uint64_t capacity,
                            uint64_t* d_offsets, uint32_t* d_status, pxb_result* d_results, void* stream) {
  using namespace pxev;
  evt_ptr fn = nullptr;
  if (int rc = validate(cfg, d_rows, count, depth, sel, d_events, capacity, d_offsets, &fn)) return rc;
  // (the events and the results move as 16-byte words)
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_events & 15u) ||
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
  const bool write = capacity && d_events;
  if (write && capacity > (~(uint64_t)0 >> 8) / sizeof(pxb_trace_event)) return PXB_E_INVAL;
  const uint64_t room = capacity + EVT_SEG_MAX;
  const size_t cnt_b = pad256((count + 1) * sizeof(uint32_t)), scan_b = pad256(need);
  const size_t stage_b = write ? (size_t)(room * sizeof(pxb_trace_event)) : 0;
  void* buf = nullptr;              // counts | the scan's scratch | staging
  if (int rc = pxw::scratch(dev, cnt_b + scan_b + stage_b, st, &buf)) return rc;
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(buf);
  EvtParams k{};
  k.p = make_params(cfg);
  k.p.first_instance = 0;
  k.rows = d_rows;
  k.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  k.count = count;
  k.depth = depth;
  k.smin = sel ? sel->step_min : 0u;
  k.smax = sel ? sel->step_max : 0xFFFFFFFFu;
  k.cnt = cnt;
  k.offsets = d_offsets;
  const dim3 grid((unsigned)((count + 63) / 64));
  hipError_t e = hipSuccess;
  do {
    if ((e = hipMemsetAsync(cnt + count, 0, sizeof(uint32_t), st)) != hipSuccess) break;
    k.status = d_status;
    k.res = reinterpret_cast<uint4*>(d_results);
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess) break;
    e = hipcub::DeviceScan::ExclusiveSum(reinterpret_cast<char*>(buf) + cnt_b, need, widen_iter(cnt, Widen{}),
                                         d_offsets, (int64_t)(count + 1), st);
    if (e != hipSuccess) break;
    if (write) {
      pxb_trace_event* const staging = reinterpret_cast<pxb_trace_event*>(reinterpret_cast<char*>(buf) + cnt_b + scan_b);
      k.out = staging;
      k.room = room;
      k.status = nullptr;
      k.res = nullptr;
      hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
      if ((e = hipGetLastError()) != hipSuccess) break;
      const uint64_t blocks = (room + 255u) / 256u;
      const dim3 pgrid((unsigned)(blocks < (1ull << 20) ? blocks : (1ull << 20)));
      hipLaunchKernelGGL(paxos_events_place_kernel, pgrid, dim3(256), 0, st, staging, room, d_offsets, count,
                         d_events, capacity);
      e = hipGetLastError();
    }
  } while (0);
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

// the HOST-buffer form: device copies of the buffers (host_stage.h) around the device form
int pxb_trace_events(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                     const pxb_trace_sel* sel, pxb_trace_event* events, uint64_t capacity, uint64_t* offsets,
                     uint32_t* status, pxb_result* results, uint64_t* n_events) {
  using namespace pxev;
  evt_ptr fn = nullptr;
  if (int rc = validate(cfg, rows, count, depth, sel, events, capacity, offsets, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  // (both calls get the status and results buffers, whatever the caller asked for)
  const auto call = [&](Staging&, const TraceBufs& d, pxb_trace_event* d_ev = nullptr, uint64_t m = 0) {
    return pxb_trace_events_device(cfg, static_cast<uint8_t*>(d.in), count, depth, sel, d_ev, m, d.off, d.st, d.res,
                                   nullptr);
  };
  pxb::StagePlan plan;                            // rows | offsets | status | results
  return trace_two_call(plan, rows, script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count, events, capacity,
                        offsets, status, results, n_events, call, call);
}

}  // extern "C"
#endif  // PXB_EVT_P == 1
