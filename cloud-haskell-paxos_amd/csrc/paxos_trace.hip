// paxos_trace.hip — pxb_trace_instance: one instance through the per-lane state
// machine (paxos_ev.h) on one GPU lane, with its state recorded at the end of
// every visited step: the device counterpart of the reference's per-message
// `say` dumps (Server.hs:85, Client.hs:108), used to localise a parity break.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "host_stage.h"
#include "lane_shapes.h"
#include "paxos_ev_kernel.h"
#include "paxos_trace_core.h"   // trace_record, trace_config_ok

namespace pxb {
namespace ev {

// one wave, lane 0 runs the instance; status[0] = records written,
// status[1] = 1 bailed / 2 out of records.  EARLY = false (the default trace):
// every step drains its copies, so each record is the oracle's end-of-step
// state exactly; EARLY = true (PXB_CFG_TRACE_PRODUCTION): the carry-over
// variant the batch kernels run (paxos_ev.h, end_op), recorded on entering the
// next step.
// LG: log mode (several Ticks per proposer, logs of commands c<id>.<t>): the
// batch kernels' log-mode shape (layout 4, EvLane<..., LG = true>, 8-step wheel)
template <int PM, int N, int W, bool EARLY, bool LG = false>
__global__ __launch_bounds__(64) void paxos_trace_kernel(EvParams p, uint32_t gid, pxb_trace_step* out, uint32_t max,
                                                         uint32_t* status, uint4* res) {
  constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using S = Shape<PM, N, POOL, W, false, LG>;
  __shared__ uint32_t lds[S::WORDS * 64];
  if (threadIdx.x != 0) return;
  EvLane<PM, N, POOL, W, false, LdsMem, EARLY, LG> L;
  L.m = LdsMem{lds, 0u};
  L.set_keys(p);
  L.init(p, gid);
  uint32_t n = 0;
  for (;;) {
    const int32_t s0 = L.s;
    EvOut o;
    const bool done = L.step(p, o);
    if (L.bailed) {
      status[1] = 1u;
      break;
    }
    if (done || L.s != s0) {
      // an instance that ends at the step cap ends from its last visited step,
      // s0, and its final step is step_cap - 1: both are recorded (the same state)
      if (trace_cap_jump(done, o, L.s, s0)) {
        if (n >= max) {
          status[1] = 2u;
          break;
        }
        trace_record(L, (uint32_t)s0, out + n++);
      }
      const uint32_t step = (uint32_t)(done ? L.s : s0);
      // (production variant: an instance whose carried step held only lost
      // copies ends at the step before it, already recorded: rewrite that record)
      const bool again = EARLY && done && n > 0 && out[n - 1].step == step;
      if (!again && n >= max) {
        status[1] = 2u;
        break;
      }
      trace_record(L, step, out + (again ? n - 1 : n));
      n += again ? 0u : 1u;
    }
    if (done) {
      *res = make_uint4(o.res[0], o.res[1], o.res[2], o.res[3]);
      break;
    }
  }
  status[0] = n;
}

typedef void (*trace_ptr)(EvParams, uint32_t, pxb_trace_step*, uint32_t, uint32_t*, uint4*);

// the kernel of a config's shape (lane_shapes.h)
template <int PM, bool E>
struct TraceKernel {
  template <int N, int W, bool LG>
  trace_ptr shape() const { return paxos_trace_kernel<PM, N, W, E, LG>; }
};
template <bool E>
struct TracePick {
  const pxb_config* cfg;
  template <int PM>
  trace_ptr proposers() const { return lane_shape(cfg, TraceKernel<PM, E>{}, (trace_ptr) nullptr); }
};

}  // namespace ev
}  // namespace pxb

extern "C" int pxb_trace_instance(const pxb_config* cfg, uint64_t instance, pxb_trace_step* out, uint32_t max_records,
                                  uint32_t* n_records, pxb_result* result) {
  using namespace pxb::ev;
  if (!cfg || !out || !n_records || max_records == 0) return PXB_E_INVAL;
  // log mode (n_ticks > 1, ABI 5): the batch kernels' log-mode shape (its
  // ticker, 14-bit commands, Execute-driven logs); eligible() holds its delays
  // to the 8-step wheel
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PXB_E_NODEV;
  const bool prod = (cfg->flags & PXB_CFG_TRACE_PRODUCTION) != 0u;
  const trace_ptr fn = prod ? lane_proposers(cfg, TracePick<true>{cfg}, (trace_ptr) nullptr)
                            : lane_proposers(cfg, TracePick<false>{cfg}, (trace_ptr) nullptr);
  if (!fn) return PXB_E_INVAL;
  EvParams p = make_params(cfg);
  p.first_instance = instance;
  pxb::StagePlan plan;                            // records | status words | result: one block
  const pxb::StageRegion r_out = plan.add(sizeof(pxb_trace_step), max_records);
  const pxb::StageRegion r_st = plan.add(sizeof(uint32_t), 2), r_res = plan.add(sizeof(uint4), 1);
  pxb::host::Staging S(plan);
  uint32_t st[2] = {0, 0};
  S.zero(r_st);
  if (S.ok()) {
    hipLaunchKernelGGL(fn, dim3(1), dim3(64), 0, 0, p, 0u, S.ptr<pxb_trace_step>(r_out), max_records,
                       S.ptr<uint32_t>(r_st), S.ptr<uint4>(r_res));
    S.note(hipGetLastError());
  }
  S.sync();
  S.down(r_st, st, 2);
  if (S.ok() && st[1]) S.note(PXB_E_INVAL);
  S.down(r_out, out, st[0]);
  S.down(r_res, result, 1);
  if (S.ok()) *n_records = st[0];
  return S.finish();
}
