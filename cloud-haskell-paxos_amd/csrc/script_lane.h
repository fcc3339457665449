// script_lane.h — the lane of a scripted kernel over a draw source, shared by
// the script kernels (paxos_script.hip: ScriptDraws) and the shrinker's
// candidate kernel (paxos_shrink.hip: ShrinkDraws), and by the host build of the
// latter (tests/native/shrink_host.cpp, Mem = its checked words): the shapes and
// pools of paxos_trace_batch_kernel's default variant, and the loop that runs a
// wave's started lanes to their ends under TraceLane.
#pragma once
#include "paxos_ev_kernel.h"
#include "paxos_trace_core.h"
#include "script_core.h"

namespace pxb {
namespace ev {

template <int PM, int N, int W, bool LG, class Mem, class Src>
struct ScriptLane {
  static constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using S = Shape<PM, N, POOL, W, false, LG>;
  using Lane = EvLane<PM, N, POOL, W, false, Mem, false, LG, false, 0, Src>;
  using Trace = TraceLane<Lane>;
};

// every lane of the wave to its end (host: the one lane); `run`: this lane started
// (T: what turns an iteration into output, TraceLane<Lane> or events_core.h's EventLane<Lane>)
template <class Lane, class Wrap>
__host__ __device__ __forceinline__ void script_run(Lane& L, Wrap& T, const EvParams& kp, bool run) {
  while (any_lane(run)) {
    if (run) run = T.iter(L, kp);
  }
}

}  // namespace ev
}  // namespace pxb
