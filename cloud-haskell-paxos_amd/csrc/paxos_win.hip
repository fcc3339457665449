// paxos_win.hip — the window pre-pass of the per-lane kernels (paxos_ev.h).
//
// EvLane::init draws one Philox block per acceptor for its isolation window
// (SEMANTICS §4).  In the per-lane kernel that is a refill, which runs under a
// divergent branch for about two lanes of the wave: ~300 wave-instructions draw
// 14 windows where a dense pass of the same instructions draws 448.  The
// windows depend only on (seed, global instance id, acceptor), so this kernel
// draws them for a whole launch, one lane per (instance, acceptor), into the
// launch's digest rows -- N words per instance, written only when that
// instance finishes -- and the refill loads its row instead (EvKParams::win).
// A handed-on instance's row is never written, so the stages behind the first
// (route_plan.h: the split, tight and log-mode second stages over the
// hand-off lists) find its windows still there and need no pre-pass of their
// own; the general kernel draws its own as before.
#include <hip/hip_runtime.h>

#include "paxos_ev_kernel.h"

namespace pxb {
namespace ev {

// rows[i * N + a] = the window word of acceptor a of instance first_instance + i, i < n
template <int N>
__global__ __launch_bounds__(256) void paxos_win_kernel(EvParams p, uint32_t n, uint32_t* rows) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= (uint64_t)n * N) return;
  const uint32_t i = (uint32_t)(t / (uint32_t)N), a = (uint32_t)t - i * (uint32_t)N;
  const uint64_t inst = p.first_instance + i;
  uint32_t crash_m1;
  const bool crashy = crash_of(p, inst, crash_m1);
  rows[t] = window_word(p, inst, a, crashy, crash_m1);
}

hipError_t launch_windows(const EvParams& p, uint32_t n_acc, uint32_t n, uint32_t* rows, hipStream_t st) {
  void (*fn)(EvParams, uint32_t, uint32_t*) = nullptr;
  switch (n_acc) {
    case 2: fn = paxos_win_kernel<2>; break;
    case 3: fn = paxos_win_kernel<3>; break;
    case 4: fn = paxos_win_kernel<4>; break;
    case 5: fn = paxos_win_kernel<5>; break;
    case 6: fn = paxos_win_kernel<6>; break;
    case 7: fn = paxos_win_kernel<7>; break;
    case 8: fn = paxos_win_kernel<8>; break;
    case 9: fn = paxos_win_kernel<9>; break;
  }
  if (!fn) return hipErrorInvalidValue;
  const uint64_t words = (uint64_t)n * n_acc;          // (a chunk: <= 2^26 x 9)
  hipLaunchKernelGGL(fn, dim3((unsigned)((words + 255u) / 256u)), dim3(256), 0, st, p, n, rows);
  return hipGetLastError();
}

}  // namespace ev
}  // namespace pxb
