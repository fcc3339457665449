// paxos_batch.hip — host side of the gfx950 batched ticket-Paxos engine: the
// C ABI (include/paxos_batch.h), launch configuration, dispatch over the
// kernel instantiations, and the single-handler hook kernels.
//
// The batch kernel itself is paxos_kernel.h (design notes there and in
// DESIGN.md); its instantiations are compiled by paxos_inst.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "host_stage.h"
#include "paxos_ev_kernel.h"
#include "paxos_ff1.h"
#include "paxos_ffp.h"
#include "paxos_kernel.h"
#include "route_plan.h"
#include "sweep_plan.h"

namespace pxb {

// The kernel instantiations live in paxos_inst.hip (compiled once per
// proposer count, in parallel); declared here for the dispatch table.
#define PXB_FOR_N(M, PM, LOGM, FF) M(PM, 2, LOGM, FF) M(PM, 3, LOGM, FF) M(PM, 4, LOGM, FF) M(PM, 5, LOGM, FF) \
  M(PM, 6, LOGM, FF) M(PM, 7, LOGM, FF) M(PM, 8, LOGM, FF) M(PM, 9, LOGM, FF)
#define PXB_FOR_MODES(M, PM) PXB_FOR_N(M, PM, false, false) PXB_FOR_N(M, PM, false, true) \
  PXB_FOR_N(M, PM, true, false) PXB_FOR_N(M, PM, true, true)
#define PXB_EXTERN(PM, N, LOGM, FF) extern template __global__ void paxos_batch_kernel<PM, N, LOGM, FF>(KParams);
PXB_FOR_MODES(PXB_EXTERN, 1)
PXB_FOR_MODES(PXB_EXTERN, 2)
PXB_FOR_MODES(PXB_EXTERN, 3)
// per-lane kernels (paxos_ev.hip): every row of ev_layouts.h x its proposer counts x N
#define PXB_EV_EXTERN(PM, N, W, C, L, S, SP) \
  extern template __global__ void ev::paxos_ev_kernel<PM, N, W, C, L, S, SP>(ev::EvKParams);
#define PXB_EV_EXTERN_N(PM, W, C, L, S, SP) PXB_EV_EXTERN(PM, 2, W, C, L, S, SP) PXB_EV_EXTERN(PM, 3, W, C, L, S, SP) \
  PXB_EV_EXTERN(PM, 4, W, C, L, S, SP) PXB_EV_EXTERN(PM, 5, W, C, L, S, SP) PXB_EV_EXTERN(PM, 6, W, C, L, S, SP)     \
  PXB_EV_EXTERN(PM, 7, W, C, L, S, SP) PXB_EV_EXTERN(PM, 8, W, C, L, S, SP) PXB_EV_EXTERN(PM, 9, W, C, L, S, SP)
#define PXB_EV_ROW(ID, W, C, L, S, SP, PART, BUILT) PXB_EV_BUILT_##BUILT(PXB_EV_EXTERN_N, W, C, L, S, SP)
PXB_EV_LAYOUTS(PXB_EV_ROW)
#undef PXB_EV_ROW
#define PXB_FF1_EXTERN(N) extern template __global__ void ff1::paxos_ff1_kernel<N>(ff1::Ff1Params);
PXB_FF1_EXTERN(2) PXB_FF1_EXTERN(3) PXB_FF1_EXTERN(4) PXB_FF1_EXTERN(5)
PXB_FF1_EXTERN(6) PXB_FF1_EXTERN(7) PXB_FF1_EXTERN(8) PXB_FF1_EXTERN(9)
#define PXB_FFP_EXTERN(P, N) extern template __global__ void ffp::paxos_ffp_kernel<P, N>(ffp::FfpParams);
#define PXB_FFP_EXTERN_N(P) PXB_FFP_EXTERN(P, 2) PXB_FFP_EXTERN(P, 3) PXB_FFP_EXTERN(P, 4) PXB_FFP_EXTERN(P, 5) \
  PXB_FFP_EXTERN(P, 6) PXB_FFP_EXTERN(P, 7) PXB_FFP_EXTERN(P, 8) PXB_FFP_EXTERN(P, 9)
PXB_FFP_EXTERN_N(1) PXB_FFP_EXTERN_N(2) PXB_FFP_EXTERN_N(3)

// ---- single-handler hook kernels ------------------------------------------
__global__ void acceptor_hook_kernel(pxb_acceptor_rec* st, const pxb_msg* in, pxb_msg* out, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  AccState A{st[i].t_max, st[i].t_store, st[i].val, (st[i].meta >> 31) != 0u};
  uint32_t log_len = st[i].meta & 0x7FFFFFFFu;
  pxb_msg r{NONE, 0, 0, 0};
  if (!A.dead) {
    int32_t rx, ry;
    uint32_t rz, ev;
    const uint32_t rk = acceptor_step(A, true, in[i].kind, in[i].x, in[i].z, rx, ry, rz, ev);
    if (ev) log_len++;
    if (rk != NONE) r = pxb_msg{rk, rx, ry, rz};
  }
  st[i] = pxb_acceptor_rec{A.t_max, A.t_store, A.val, log_len | ((A.dead ? 1u : 0u) << 31)};
  out[i] = r;
}

__global__ void proposer_hook_kernel(pxb_proposer_rec* st, uint32_t n_acc, const pxb_msg* in,
                                     pxb_msg* bc, uint32_t* nb, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  pxb_proposer_rec R = st[i];
  PropState S{R.ticket, R.cmd, R.acks, R.state, R.mr_t, R.mr_v, R.r2_t, R.r2_v, R.pending != 0u ? 1u : 0u};
  Req o0{NONE, 0, 0}, o1{NONE, 0, 0};
  uint32_t no;
  if (in[i].kind == 3u)
    no = proposer_tick(S, (R.client_id << 24) | ((uint32_t)(S.ticket + 1) & 0xFFFFFFu), o0);
  else
    no = proposer_step(S, n_acc, in[i].kind, in[i].x, in[i].y, in[i].z, o0, o1);
  st[i] = pxb_proposer_rec{S.ticket, S.cmd, S.acks, S.rs, S.mr_t, S.mr_v, S.r2_t, S.r2_v,
                           S.pending ? 1u : 0u, R.client_id};
  bc[2 * i] = (no > 0) ? pxb_msg{o0.kind, o0.x, 0, o0.z} : pxb_msg{NONE, 0, 0, 0};
  bc[2 * i + 1] = (no > 1) ? pxb_msg{o1.kind, o1.x, 0, o1.z} : pxb_msg{NONE, 0, 0, 0};
  nb[i] = no;
}

// per-slot queue / counter words (finalize_kernel resets them; route_plan.h names the ones in use)
constexpr uint32_t QWORDS = 8;

// Sums the TCOPIES partial rows of the general kernel, and those of the
// per-lane kernels unless the bailed-id list the general kernel ran
// (queue[bail_word]) overflowed (then it re-ran every instance of the chunk),
// into the caller's totals; zeroes them and resets the queue words, so the
// launch slot is clean for its next use.  One block of TCOPIES threads;
// thread t reads column t % 16 of rows t/16, t/16+16, ...
__global__ __launch_bounds__(TCOPIES) void finalize_kernel(unsigned long long* part, unsigned long long* part_ev,
                                                            uint32_t* queue, uint32_t bail_word, uint32_t bail_cap,
                                                            unsigned long long* totals, unsigned long long* hand) {
  __shared__ unsigned long long acc[16];
  const uint32_t t = threadIdx.x;
  if (t < 16) acc[t] = 0ull;
  // the device's hand-off counts (pxb_handoff_counts): instances the first
  // per-lane kernel handed on, and those a second one handed on
  if (t < 2 && queue[t ? Q_BAIL2 : Q_BAIL]) atomicAdd(&hand[t], (unsigned long long)queue[t ? Q_BAIL2 : Q_BAIL]);
  __syncthreads();
  const bool ev_ok = queue[bail_word] <= bail_cap;
  unsigned long long v = 0ull;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    v += part[t + j * TCOPIES] + (ev_ok ? part_ev[t + j * TCOPIES] : 0ull);
    part[t + j * TCOPIES] = 0ull;
    part_ev[t + j * TCOPIES] = 0ull;
  }
  if (v) atomicAdd(&acc[t % 16u], v);
  __syncthreads();
  if (t < 16 && acc[t]) atomicAdd(&totals[t], acc[t]);
  if (t >= 16 && t < 16 + QWORDS) queue[t - 16] = 0u;
}

// The read of the device's hand-off counts (pxb_handoff_counts): out[t] = count
// t, zeroed in the same atomic when reset, so a finalize_kernel of another
// thread's chunk never adds between the read and the zeroing
__global__ void hand_xchg_kernel(unsigned long long* h, unsigned long long* out, int reset) {
  const uint32_t t = threadIdx.x;
  if (t < 2) out[t] = reset ? atomicExch(&h[t], 0ull) : atomicAdd(&h[t], 0ull);
}

// ---- host side ----------------------------------------------------------------
typedef void (*kernel_ptr)(KParams);
typedef void (*ev_kernel_ptr)(ev::EvKParams);

template <int PM, int W, bool C, bool L, bool S, int SP>
static ev_kernel_ptr ev_pick_n(uint32_t n) {
  switch (n) {
    case 2: return ev::paxos_ev_kernel<PM, 2, W, C, L, S, SP>;
    case 3: return ev::paxos_ev_kernel<PM, 3, W, C, L, S, SP>;
    case 4: return ev::paxos_ev_kernel<PM, 4, W, C, L, S, SP>;
    case 5: return ev::paxos_ev_kernel<PM, 5, W, C, L, S, SP>;
    case 6: return ev::paxos_ev_kernel<PM, 6, W, C, L, S, SP>;
    case 7: return ev::paxos_ev_kernel<PM, 7, W, C, L, S, SP>;
    case 8: return ev::paxos_ev_kernel<PM, 8, W, C, L, S, SP>;
    case 9: return ev::paxos_ev_kernel<PM, 9, W, C, L, S, SP>;
  }
  return nullptr;
}

typedef void (*ff1_kernel_ptr)(ff1::Ff1Params);
static ff1_kernel_ptr ff1_pick(uint32_t n) {
  switch (n) {
    case 2: return ff1::paxos_ff1_kernel<2>;
    case 3: return ff1::paxos_ff1_kernel<3>;
    case 4: return ff1::paxos_ff1_kernel<4>;
    case 5: return ff1::paxos_ff1_kernel<5>;
    case 6: return ff1::paxos_ff1_kernel<6>;
    case 7: return ff1::paxos_ff1_kernel<7>;
    case 8: return ff1::paxos_ff1_kernel<8>;
    case 9: return ff1::paxos_ff1_kernel<9>;
  }
  return nullptr;
}

typedef void (*ffp_kernel_ptr)(ffp::FfpParams);
template <int P>
static ffp_kernel_ptr ffp_pick_n(uint32_t n) {
  switch (n) {
    case 2: return ffp::paxos_ffp_kernel<P, 2>;
    case 3: return ffp::paxos_ffp_kernel<P, 3>;
    case 4: return ffp::paxos_ffp_kernel<P, 4>;
    case 5: return ffp::paxos_ffp_kernel<P, 5>;
    case 6: return ffp::paxos_ffp_kernel<P, 6>;
    case 7: return ffp::paxos_ffp_kernel<P, 7>;
    case 8: return ffp::paxos_ffp_kernel<P, 8>;
    case 9: return ffp::paxos_ffp_kernel<P, 9>;
  }
  return nullptr;
}
static ffp_kernel_ptr ffp_pick(uint32_t p, uint32_t n) {
  return p == 1 ? ffp_pick_n<1>(n) : p == 2 ? ffp_pick_n<2>(n) : p == 3 ? ffp_pick_n<3>(n) : nullptr;
}

// the kernel of a per-lane stage (a row of ev_layouts.h at one of its proposer counts)
static ev_kernel_ptr ev_pick(RouteStage s, uint32_t n) {
  switch (s.pm * 10 + (uint32_t)s.layout) {
#define PXB_EV_CASE(PM, ID, W, C, L, S, SP) \
  case PM * 10 + ID: return ev_pick_n<PM, W, C, L, S, SP>(n);
#define PXB_EV_ROW(ID, W, C, L, S, SP, PART, BUILT) PXB_EV_BUILT_##BUILT(PXB_EV_CASE, ID, W, C, L, S, SP)
    PXB_EV_LAYOUTS(PXB_EV_ROW)
#undef PXB_EV_ROW
#undef PXB_EV_CASE
  }
  return nullptr;
}
struct kernel_fn {
  kernel_ptr fn;
  int wpb;                       // waves per block (Shape<>::wpb)
  int occ;                       // waves per SIMD target (Shape<>::occ)
  explicit operator bool() const { return fn != nullptr; }
};

template <int PM, int N, bool LOGM, bool FF>
static kernel_fn kfn() { return kernel_fn{paxos_batch_kernel<PM, N, LOGM, FF>, Shape<PM, N, LOGM, FF>::wpb, Shape<PM, N, LOGM, FF>::occ}; }

template <int PM, bool LOGM, bool FF>
static kernel_fn pick_n(uint32_t n) {
  switch (n) {
    case 2: return kfn<PM, 2, LOGM, FF>();
    case 3: return kfn<PM, 3, LOGM, FF>();
    case 4: return kfn<PM, 4, LOGM, FF>();
    case 5: return kfn<PM, 5, LOGM, FF>();
    case 6: return kfn<PM, 6, LOGM, FF>();
    case 7: return kfn<PM, 7, LOGM, FF>();
    case 8: return kfn<PM, 8, LOGM, FF>();
    case 9: return kfn<PM, 9, LOGM, FF>();
  }
  return kernel_fn{nullptr, 0, 0};
}

template <int PM>
static kernel_fn pick_mode(uint32_t n, bool logm, bool ff) {
  if (logm) return ff ? pick_n<PM, true, true>(n) : pick_n<PM, true, false>(n);
  return ff ? pick_n<PM, false, true>(n) : pick_n<PM, false, false>(n);
}

// single decree (one Tick per proposer) or log mode (several); fault-free or not
static kernel_fn pick(uint32_t pm, uint32_t n, bool logm, bool ff) {
  switch (pm) {
    case 1: return pick_mode<1>(n, logm, ff);
    case 2: return pick_mode<2>(n, logm, ff);
    case 3: return pick_mode<3>(n, logm, ff);
  }
  return kernel_fn{nullptr, 0, 0};
}

// Test and A/B hooks (environment variables), read once -- on the first
// launch, or by pxb_reload_hooks() -- and never by getenv in the launch path,
// which is not safe against a concurrent setenv (tests/conftest.py's
// `hooks` helper sets them and reloads)
struct Hooks {
  RouteHooks route;               // PXB_NO_* and PXB_EV_BAIL_CAP (route_plan.h)
  // tests only: PXB_FAIL_AFTER_FIRST=1 fails every chunk right after its first
  // per-lane launch (the list and slot bookkeeping of the failure path);
  // PXB_FF1_BAIL=1 hands every fault-free instance to the general kernel
  bool fail_after_first, ff1_bail;
  // A/B and tests: PXB_NO_WIN_PREPASS=1 keeps the per-lane kernels' window
  // draws in their refill (no paxos_win.hip pre-pass)
  bool no_win_prepass;
  int blocks_per_cu;            // PXB_BLOCKS_PER_CU (0: none)
  int ff1_oversub, ffp_oversub;   // PXB_FF1_OVERSUB / PXB_FFP_OVERSUB (0: FF1_OVERSUB)
  char multi_fail_phase[16];      // PXB_MULTI_FAIL_PHASE / _DEVICE (paxos_multi.cpp)
  int multi_fail_device;
  uint64_t sweep_chunk;           // PXB_SWEEP_CHUNK (instances per pxb_sweep chunk)
  uint64_t explore_chunk;         // PXB_EXPLORE_CHUNK (candidates per pxb_explore chunk)
};
static Hooks g_hooks;
static bool g_hooks_read = false;

static thread_local int g_last_hip = 0;
#ifdef PXB_STAMPS
static unsigned long long* g_dbg = nullptr;
#endif
static std::mutex g_mu;
// blocks per CU that fit of (kernel, block size), per device (occ_blocks; absent or 0 = unknown)
static std::map<std::pair<const void*, int>, int> g_occ[64];
static int g_cus[64];
// Per-launch scratch: QSLOTS slots per device, each two sets of TCOPIES
// partial-total rows (16 x u64; the general kernel's and the per-lane
// kernel's) + the queue words on their own 128-B line.  Each launch takes the
// next slot round-robin; its finalize_kernel leaves the slot zeroed, so
// consecutive launches need no memset.  Up to QSLOTS launches of one device
// may be in flight at once (on any streams).
constexpr int QSLOTS = 64;
constexpr size_t ROWS_U64 = (size_t)TCOPIES * 16;
constexpr size_t SLOT_U64 = 2 * ROWS_U64 + 16;
// (+ 16 words after the last slot: the device's hand-off counts)
constexpr size_t HAND_U64 = (size_t)QSLOTS * SLOT_U64;
static unsigned long long* g_slots[64];
static uint32_t g_qseq[64];
// Each slot's event is recorded behind the last chunk that used it (its
// finalize_kernel, or the zeroing of a failed chunk), and a chunk that takes
// the slot makes its stream wait for it (hipStreamWaitEvent, on the device),
// so a 65th chunk in flight across streams waits for the first one's slot
// instead of sharing its queue words and partial rows
static hipEvent_t g_slot_ev[64][QSLOTS];
static bool g_slot_ev_set[64][QSLOTS];
// (slot creation: a device's own lock, so that its allocation and wait never
// hold up launches on other devices under g_mu)
static std::mutex g_dev_mu[64];
// fault-free per-lane kernels: blocks per launch, in multiples of the resident
// ones (the dispatcher then hands a freed CU the next block, which balances
// waves that run slower; one 2^28 config-2 launch: x1 5.26 ms, x2 4.76, x4 4.42,
// x8 4.30, x16 4.25)
constexpr uint64_t FF1_OVERSUB = 16;
// At most EV_LIST_STREAMS streams per device hold the bailed-id lists of
// route_plan.h (created lazily, 16 MB each + 64 MB for the two-stage routings).  An entry records an event behind
// the last launches that use its lists (on every exit of a chunk once one of
// them is queued, failures included); they are enqueued with g_mu held, so
// whoever takes the entry over later (a stream beyond EV_LIST_STREAMS evicting
// the oldest, or any stream taking one that pxb_stream_release freed) first
// makes its own stream wait for that event (hipStreamWaitEvent: no host wait,
// so no thread blocks under g_mu): two streams never share a list while
// either may still run on it.  Ownership is a flag, not the stream handle:
// the null (default) stream is a stream like any other.
constexpr int EV_LIST_STREAMS = 8;
struct EvLists {
  hipStream_t s;                // owner, when owned
  bool owned;                   // (false: free, buffers kept for the next owner)
  uint32_t* bail;
  uint32_t* split;
  hipEvent_t ev;                // behind the owner's last launches on these lists
  bool ev_set;
};
static EvLists g_lists[64][EV_LIST_STREAMS];
static int g_nlists[64], g_lnext[64];

// (host_stage.h: every unit's hip_fail records here)
void host::set_last_hip_error(int e) { g_last_hip = e; }
using host::hip_fail;
#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t _e = (x);                            \
    if (_e != hipSuccess) return hip_fail(_e);      \
  } while (0)

static int validate(const pxb_config* c) {
  if (!c) return PXB_E_INVAL;
  if (c->n_proposers < 1 || c->n_proposers > PXB_MAX_PROPOSERS) return PXB_E_INVAL;
  if (c->n_acceptors < PXB_MIN_ACCEPTORS || c->n_acceptors > PXB_MAX_ACCEPTORS) return PXB_E_INVAL;
  if (c->loss_ppm > 1000000u || c->crash_ppm > 1000000u) return PXB_E_INVAL;
  if (c->delay_max < 1 || c->delay_max > PXB_MAX_DELAY) return PXB_E_INVAL;
  if (c->crash_len_max < 1 || c->crash_len_max > 4096 || c->crash_start_max > 65535) return PXB_E_INVAL;
  if (c->skew_max > 4096) return PXB_E_INVAL;
  if (c->step_cap < 1 || c->step_cap > PXB_MAX_STEP_CAP) return PXB_E_INVAL;
  if (c->n_instances > (1ull << 40)) return PXB_E_INVAL;
  if (c->n_ticks > PXB_MAX_TICKS) return PXB_E_INVAL;
  if (c->n_ticks > 1 && (c->tick_period < 1 || c->tick_period > PXB_MAX_STEP_CAP)) return PXB_E_INVAL;
  return PXB_OK;
}

}  // namespace pxb

using namespace pxb;

extern "C" {

int pxb_abi_version(void) { return PXB_ABI_VERSION; }

#ifdef PXB_STAMPS
// diagnostic build only: cycles per kernel section and event counts, summed over waves (and reset)
int pxb_debug_stamps(unsigned long long* out16) {
  if (!g_dbg) return PXB_E_INVAL;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out16, g_dbg, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(g_dbg, 0, 16 * sizeof(unsigned long long)));
  return PXB_OK;
}
#endif
#ifdef PXB_WAVE_TIMES
// diagnostic build only: (start, end, HW_ID, XCC_ID, shader-clock start, end) of every wave of the last launch
static unsigned long long* g_wt = nullptr;
static unsigned g_wt_waves = 0;
int pxb_debug_wave_times(unsigned long long* out, unsigned max_waves) {
  if (!g_wt) return PXB_E_INVAL;
  HIPCHK(hipDeviceSynchronize());
  const unsigned nw = std::min(g_wt_waves, max_waves);
  HIPCHK(hipMemcpy(out, g_wt, 6ull * nw * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return (int)nw;
}
#endif
int pxb_last_hip_error(void) { return g_last_hip; }

// the bailed-id lists of (dev, stream) (callers hold g_mu until their launches
// on the lists are enqueued and a RecordOnExit holds the entry's event)
static int stream_lists(int dev, hipStream_t st, bool need_split, uint32_t** bail, uint32_t** split,
                        EvLists** ent) {
  EvLists* e = nullptr;
  for (int k = 0; k < g_nlists[dev] && !e; ++k)
    if (g_lists[dev][k].owned && g_lists[dev][k].s == st) e = &g_lists[dev][k];
  bool handover = e == nullptr;
  for (int k = 0; k < g_nlists[dev] && !e; ++k)      // a freed entry (its owner released it)
    if (!g_lists[dev][k].owned) e = &g_lists[dev][k];
  if (!e) {
    if (g_nlists[dev] < EV_LIST_STREAMS) e = &g_lists[dev][g_nlists[dev]++];
    else e = &g_lists[dev][g_lnext[dev]++ % EV_LIST_STREAMS];   // every entry owned: take the oldest over
  }
  if (handover) {                                    // new owner: after the old owner's launches
    if (e->ev_set) HIPCHK(hipStreamWaitEvent(st, e->ev, 0));
    e->s = st;
    e->owned = true;
  }
  if (!e->ev) HIPCHK(hipEventCreateWithFlags(&e->ev, hipEventDisableTiming));
  if (!e->bail) HIPCHK(hipMalloc(&e->bail, (size_t)EV_BAIL_CAP * sizeof(uint32_t)));
  if (need_split && !e->split) HIPCHK(hipMalloc(&e->split, (size_t)EV_SPLIT_CAP * sizeof(uint32_t)));
  *bail = e->bail;
  *split = need_split ? e->split : nullptr;
  *ent = e;
  return PXB_OK;
}

// Records an event behind whatever a chunk queued on its stream, on every exit
// of the chunk (success or failure): the chunk's scratch slot (g_slot_ev) and,
// where it uses them, its lists (EvLists::ev).  `ev` null: nothing to record.
// (g_mu held: declared after the chunk's lock, so destroyed before it)
struct RecordOnExit {
  hipEvent_t ev;
  bool* set;                    // the event's "recorded" flag
  hipStream_t st;
  ~RecordOnExit() {
    if (!ev) return;
    *set = hipEventRecord(ev, st) == hipSuccess;
    // (no event behind these launches: wait for them here, so that a later
    // user of the slot, or a later owner of the lists, cannot share them)
    if (!*set) (void)hipStreamSynchronize(st);
  }
};

// A stream that is about to be destroyed gives up its lists (paxos_multi.cpp
// creates a stream per device and call): the entry is freed for the next stream
// (which waits for the event first), so lists never outlive their stream's use.
extern "C" void pxb_stream_release(int dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (dev < 0 || dev >= 64) return;
  std::lock_guard<std::mutex> lk(g_mu);
  for (int k = 0; k < g_nlists[dev]; ++k)
    if (g_lists[dev][k].owned && g_lists[dev][k].s == st) g_lists[dev][k].owned = false;
}

// per-device scratch of pxb_run_device, created on the current device `dev`
// (callers do NOT hold g_mu: the allocation and the wait for its zeroing take
// only this device's lock, so a device's first launch holds up no launch on
// another device); published under g_mu
static int ensure_slots(int dev) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_slots[dev]) return PXB_OK;
  }
  std::lock_guard<std::mutex> dl(g_dev_mu[dev]);
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_slots[dev]) return PXB_OK;            // (another thread made them meanwhile)
  }
  unsigned long long* q = nullptr;
  hipStream_t zs = nullptr;
  hipError_t e = hipMalloc(&q, (HAND_U64 + 16) * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&zs, hipStreamNonBlocking);
  // (the zeroing completes before any launch can use the slots: a private
  // stream, so this waits for nothing else on the device)
  if (e == hipSuccess) e = hipMemsetAsync(q, 0, (HAND_U64 + 16) * sizeof(unsigned long long), zs);
  if (e == hipSuccess) e = hipStreamSynchronize(zs);
  for (int k = 0; k < QSLOTS && e == hipSuccess; ++k)
    if (!g_slot_ev[dev][k]) e = hipEventCreateWithFlags(&g_slot_ev[dev][k], hipEventDisableTiming);
  if (zs) (void)hipStreamDestroy(zs);
  if (e != hipSuccess) {
    if (q) (void)hipFree(q);
    return hip_fail(e);
  }
  std::lock_guard<std::mutex> lk(g_mu);
  for (int k = 0; k < QSLOTS; ++k) g_slot_ev_set[dev][k] = false;
  g_slots[dev] = q;
  return PXB_OK;
}

static void read_hooks_locked() {
  Hooks h;
  memset(&h, 0, sizeof(h));
  auto flag = [](const char* name) {
    const char* v = getenv(name);
    return v && atoi(v) > 0;
  };
  auto num = [](const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
  };
  h.route.no_ev = flag("PXB_NO_EV");
  h.route.no_ff1 = flag("PXB_NO_FF1");
  h.route.no_ffp = flag("PXB_NO_FFP");
  h.route.no_split = flag("PXB_NO_SPLIT");
  h.route.no_tight = flag("PXB_NO_TIGHT");
  h.route.no_lg2 = flag("PXB_NO_LG2");
  h.route.no_lgs = flag("PXB_NO_LGS");
  h.fail_after_first = flag("PXB_FAIL_AFTER_FIRST");
  h.ff1_bail = flag("PXB_FF1_BAIL");
  h.no_win_prepass = flag("PXB_NO_WIN_PREPASS");
  h.route.bail_cap = num("PXB_EV_BAIL_CAP", -1);
  h.blocks_per_cu = std::max(0, num("PXB_BLOCKS_PER_CU", 0));
  const int fo = num("PXB_FF1_OVERSUB", 0), po = num("PXB_FFP_OVERSUB", 0);
  h.ff1_oversub = (fo > 0 && fo <= 64) ? fo : 0;
  h.ffp_oversub = (po > 0 && po <= 64) ? po : 0;
  const char* ph = getenv("PXB_MULTI_FAIL_PHASE");
  if (ph) snprintf(h.multi_fail_phase, sizeof(h.multi_fail_phase), "%s", ph);
  h.multi_fail_device = num("PXB_MULTI_FAIL_DEVICE", -1);
  const char* sc = getenv("PXB_SWEEP_CHUNK");
  h.sweep_chunk = sc ? sweep_clamp_chunk(atoll(sc)) : SWEEP_CHUNK_DEFAULT;
  const char* xc = getenv("PXB_EXPLORE_CHUNK");
  const long long xv = xc ? atoll(xc) : 0;
  h.explore_chunk = xv < 1 ? (1ull << 26) : xv > (1ll << 32) ? (1ull << 32) : (uint64_t)xv;   // (unset: 2^26)
  g_hooks = h;
  g_hooks_read = true;
}

// the hooks in force (a copy: callers read it without the lock)
static Hooks hooks() {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_hooks_read) read_hooks_locked();
  return g_hooks;
}

// (paxos_multi.cpp's failure injection: device g fails in `phase`)
bool multi_fail_injected(const char* phase, int g) {
  const Hooks h = hooks();
  return h.multi_fail_phase[0] && strcmp(h.multi_fail_phase, phase) == 0 && h.multi_fail_device == g;
}
// (paxos_explore.hip's chunk size: candidates per pxb_explore chunk)
uint64_t explore_chunk_hook(void) { return hooks().explore_chunk; }


extern "C" void pxb_multi_release(void);   // paxos_multi.cpp
extern "C" void pxb_wire_release(void);    // paxos_wire.hip

int pxb_init(int n_devices) {
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess || visible == 0) return PXB_E_NODEV;
  const int G = (n_devices <= 0) ? visible : n_devices;
  if (G > visible || G > 64) return PXB_E_INVAL;
  int cur = 0;
  HIPCHK(hipGetDevice(&cur));
  (void)hooks();                       // (the test hooks: read now, not in a launch)
  for (int d = 0; d < G; ++d) {
    HIPCHK(hipSetDevice(d));
    if (int rc = ensure_slots(d)) {
      (void)hipSetDevice(cur);
      return rc;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, d));
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_cus[d]) g_cus[d] = prop.multiProcessorCount;
  }
  HIPCHK(hipSetDevice(cur));
  return PXB_OK;
}

void pxb_reload_hooks(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  read_hooks_locked();
}

int pxb_shutdown(void) {
  int cur = 0;
  const bool have_dev = hipGetDevice(&cur) == hipSuccess;
  int rc = PXB_OK;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (int d = 0; d < 64; ++d) {
      const bool any = g_slots[d] != nullptr || g_nlists[d] > 0;
      if (!any) continue;
      if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = PXB_E_HIP;
      if (g_slots[d]) (void)hipFree(g_slots[d]);
      g_slots[d] = nullptr;
      for (int k = 0; k < QSLOTS; ++k) {
        if (g_slot_ev[d][k]) (void)hipEventDestroy(g_slot_ev[d][k]);
        g_slot_ev[d][k] = nullptr;
        g_slot_ev_set[d][k] = false;
      }
      for (int k = 0; k < g_nlists[d]; ++k) {
        if (g_lists[d][k].bail) (void)hipFree(g_lists[d][k].bail);
        if (g_lists[d][k].split) (void)hipFree(g_lists[d][k].split);
        if (g_lists[d][k].ev) (void)hipEventDestroy(g_lists[d][k].ev);
        g_lists[d][k] = EvLists{};
      }
      g_nlists[d] = g_lnext[d] = 0;
      g_qseq[d] = 0;
    }
  }
  pxb_multi_release();
  pxb_wire_release();
  if (have_dev) (void)hipSetDevice(cur);
  return rc;
}

const char* pxb_strerror(int code) {
  switch (code) {
    case PXB_OK: return "ok";
    case PXB_E_INVAL: return "invalid argument";
    case PXB_E_HIP: return "HIP runtime error";
    case PXB_E_OOM: return "device out of memory";
    case PXB_E_NODEV: return "no GPU device";
    case PXB_E_RCCL: return "collective failure";
  }
  return "unknown error";
}

uint64_t pxb_canonical_bytes_nofault(uint32_t n_acceptors) { return 196ull * n_acceptors + 160ull; }

int pxb_handoff_counts(int dev, uint64_t* out2, int reset) {
  if (!out2 || dev < 0 || dev >= 64) return PXB_E_INVAL;
  unsigned long long* h = nullptr;
  {
    // (the device wait below runs without g_mu: launches on other devices go on)
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_slots[dev]) h = g_slots[dev] + HAND_U64;
  }
  if (!h) {
    out2[0] = out2[1] = 0;
    return PXB_OK;
  }
  // (one reader at a time: the exchange's two output words are shared)
  static std::mutex hand_mu;
  std::lock_guard<std::mutex> hl(hand_mu);
  int cur = 0;
  HIPCHK(hipGetDevice(&cur));
  HIPCHK(hipSetDevice(dev));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    // read and (reset) zero in one atomic per count, on the device
    hipLaunchKernelGGL(hand_xchg_kernel, dim3(1), dim3(64), 0, nullptr, h, h + 2, reset ? 1 : 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out2, h + 2, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost);
  (void)hipSetDevice(cur);
  return e == hipSuccess ? PXB_OK : hip_fail(e);
}

// ---- pxb_run_device's pieces: occupancy, parameters, launches ----

// Blocks per CU that fit of `fn` at `block` threads, queried once per device
// and kernel (g_mu held).  Keyed by the kernel itself, so no routing can file
// one kernel's figure under another's.
static int occ_blocks(int dev, const void* fn, int block, int* out) {
  int& o = g_occ[dev][std::make_pair(fn, block)];
  if (!o) {
    int nb = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, 0));
    o = std::max(1, nb);
  }
  *out = o;
  return PXB_OK;
}

// the general kernel's launch parameters of a config (first_instance,
// n_instances, the outputs and the slot: per chunk)
static KParams make_kparams(const pxb_config* cfg) {
  KParams kp;
  memset(&kp, 0, sizeof(kp));
  const bool logm = cfg->n_ticks > 1;
  kp.k0 = (uint32_t)cfg->seed;
  kp.k1 = (uint32_t)(cfg->seed >> 32);
  kp.n_prop = cfg->n_proposers;
  kp.delay_max = cfg->delay_max;
  kp.loss_ppm = cfg->loss_ppm;
  kp.crash_ppm = cfg->crash_ppm;
  kp.crash_len_max = cfg->crash_len_max;
  kp.crash_start_max = cfg->crash_start_max;
  kp.skew_max = cfg->skew_max;
  kp.step_cap = cfg->step_cap;
  kp.n_ticks = logm ? cfg->n_ticks : 1u;
  kp.tick_period = logm ? cfg->tick_period : 1u;
  const uint64_t lt = prob_threshold(cfg->loss_ppm), ct = prob_threshold(cfg->crash_ppm);
  kp.cfg = ((cfg->flags & PXB_CFG_RANDOMIZE) ? CFG_RANDOMIZE : 0u) | (lt ? CFG_LOSSY : 0u) | (ct ? CFG_CRASHY : 0u);
  kp.loss_m1 = (uint32_t)(lt - 1ull);
  kp.crash_m1 = (uint32_t)(ct - 1ull);
  return kp;
}

#ifdef PXB_WAVE_TIMES
// diagnostic build only: the timeline buffer, for a launch of `waves` waves
static int wave_times_buf(unsigned waves, unsigned long long** out) {
  if (!g_wt) HIPCHK(hipMalloc(&g_wt, 6ull * 65536 * sizeof(unsigned long long)));
  g_wt_waves = waves;
  *out = g_wt;
  return PXB_OK;
}
#endif

// the general kernel, `grid` blocks; with `ids`: over the instances a per-lane
// kernel listed there (their count in queue word `word`, the list's capacity `cap`)
static hipError_t launch_general(const kernel_fn& fn, unsigned grid, hipStream_t st, KParams kp,
                                 const uint32_t* ids = nullptr, uint32_t word = 0, uint32_t cap = 0) {
  if (ids) {
    kp.ids = ids;
    kp.n_ids = kp.queue + word;
    kp.ids_cap = cap;
  }
  hipLaunchKernelGGL(fn.fn, dim3(grid), dim3(64 * fn.wpb), 0, st, kp);
  return hipGetLastError();
}

// A fault-free per-lane kernel (paxos_ff1.h / paxos_ffp.h) over the chunk of
// `kp`, `grid` blocks, then the general kernel (`resident` blocks) over its
// bailed ids.  `fp` arrives zeroed but for the fields only its kernel has.
extern "C++" template <class Kernel, class Params>
static hipError_t launch_fault_free(Kernel kernel, Params fp, unsigned grid, const kernel_fn& fn, unsigned resident,
                                    hipStream_t st, const KParams& kp, uint32_t* bail, uint32_t cap, bool bail_all) {
  fp.first_instance = kp.first_instance;
  fp.k0 = kp.k0;
  fp.k1 = kp.k1;
  fp.skew_max = kp.skew_max;
  fp.step_cap = kp.step_cap;
  fp.n_instances = kp.n_instances;
  fp.out = kp.out;
  fp.dig = kp.dig;
  fp.acc = kp.acc;
  fp.part = kp.part + ROWS_U64;
  fp.bail_ids = bail;
  fp.bail_n = kp.queue + Q_BAIL;
  fp.bail_cap = cap;
  fp.bail_all = bail_all ? 1u : 0u;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, fp);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_general(fn, resident, st, kp, bail, Q_BAIL, cap);
}

// Validate, plan (route_plan.h), query the occupancy of the plan's kernels,
// resolve, then chunk by chunk launch what the plan says and finalize_kernel.
int pxb_run_device(const pxb_config* cfg, pxb_result* d_out, uint32_t* d_log_digest,
                   pxb_acceptor_rec* d_acc, int64_t* d_totals, void* stream) {
  int rc = validate(cfg);
  if (rc) return rc;
  if (!d_totals) return PXB_E_INVAL;
  if (cfg->n_instances == 0) return PXB_OK;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return PXB_E_NODEV;
  const Hooks hk = hooks();
  RoutePlan plan = route_plan(cfg, hk.route);
  const uint32_t N = cfg->n_acceptors;
  const kernel_fn fn = pick(cfg->n_proposers, N, plan.logm, plan.ff);
  const ff1_kernel_ptr ffn = plan.kind == ROUTE_FF1 ? ff1_pick(N) : nullptr;
  const ffp_kernel_ptr pfn = plan.kind == ROUTE_FFP ? ffp_pick(cfg->n_proposers, N) : nullptr;
  // (efn: the per-lane stage that hands on to the general kernel; sfn: the one over the chunk before it)
  const ev_kernel_ptr efn = plan.kind == ROUTE_EV ? ev_pick(plan.second, N) : nullptr;
  const ev_kernel_ptr sfn = plan.two_stage != TWO_NONE ? ev_pick(plan.first, N) : nullptr;
  if (!fn || (plan.kind == ROUTE_FF1 && !ffn) || (plan.kind == ROUTE_FFP && !pfn) || (plan.kind == ROUTE_EV && !efn) ||
      (plan.two_stage != TWO_NONE && !sfn))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int occ, cus, eocc = 0, socc = 0;              // blocks per CU: general, last per-lane stage, first one
  if (int rc2 = ensure_slots(dev)) return rc2;   // (not under g_mu: see ensure_slots)
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_cus[dev]) {
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, dev));
      g_cus[dev] = prop.multiProcessorCount;
    }
    cus = g_cus[dev];
    if (int rc2 = occ_blocks(dev, (const void*)fn.fn, 64 * fn.wpb, &occ)) return rc2;
    // Residency: the launch-bounds target (waves per SIMD x 4 SIMDs), even when
    // a small kernel would fit more (measured: 4 -> 6 waves/SIMD costs 5 % on
    // config 2: more, more often partially filled slot generations per wave).
    occ = std::min(occ, std::max(1, 4 * fn.occ / fn.wpb));
    if (ffn || pfn)
      if (int rc2 = occ_blocks(dev, ffn ? (const void*)ffn : (const void*)pfn, 256, &eocc)) return rc2;
    if (efn)
      if (int rc2 = occ_blocks(dev, (const void*)efn, 64, &eocc)) return rc2;
    if (sfn)
      if (int rc2 = occ_blocks(dev, (const void*)sfn, 64, &socc)) return rc2;
    plan = route_resolve(plan, socc, eocc);
    if (hk.blocks_per_cu > 0) {                 // tests / experiments: cap residency
      occ = std::min(occ, hk.blocks_per_cu);
      if (eocc) eocc = std::min(eocc, hk.blocks_per_cu);
      if (socc) socc = std::min(socc, hk.blocks_per_cu);
    }
  }
  const bool two_stage = plan.two_stage != TWO_NONE;
  KParams kp = make_kparams(cfg);
  unsigned long long* const totals = reinterpret_cast<unsigned long long*>(d_totals);
#ifdef PXB_STAMPS
  if (!g_dbg) {
    HIPCHK(hipMalloc(&g_dbg, 16 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(g_dbg, 0, 16 * sizeof(unsigned long long)));
  }
  kp.dbg = g_dbg;
#endif
  const uint64_t G = 64 / N, wpb = (uint64_t)fn.wpb;
  const uint64_t resident = (uint64_t)occ * (uint64_t)cus;
  const uint64_t chunk_max = route_chunk_max(plan, resident, wpb, G);
  for (uint64_t done = 0; done < cfg->n_instances; done += chunk_max) {
    const uint64_t nc = std::min<uint64_t>(chunk_max, cfg->n_instances - done);
    kp.first_instance = cfg->first_instance + done;
    kp.n_instances = (uint32_t)nc;
    kp.out = d_out ? reinterpret_cast<uint4*>(d_out + done) : nullptr;
    kp.dig = d_log_digest ? d_log_digest + done * N : nullptr;
    kp.acc = d_acc ? reinterpret_cast<uint4*>(d_acc + done * N) : nullptr;
    uint32_t *bail = nullptr, *slist = nullptr;
    EvLists* lent = nullptr;
    // (held until this chunk's launches are enqueued: see EvLists)
    std::unique_lock<std::mutex> lk(g_mu);
    const int sidx = (int)(g_qseq[dev]++ % QSLOTS);
    unsigned long long* const slot = g_slots[dev] + (size_t)sidx * SLOT_U64;
    kp.part = slot;
    kp.queue = reinterpret_cast<uint32_t*>(slot + 2 * ROWS_U64);
    // after the slot's last user (another stream's chunk may still run on it)
    if (g_slot_ev_set[dev][sidx]) HIPCHK(hipStreamWaitEvent(st, g_slot_ev[dev][sidx], 0));
    // the slot's event goes behind whatever this chunk queues, on every exit
    RecordOnExit slot_use{g_slot_ev[dev][sidx], &g_slot_ev_set[dev][sidx], st};
    if (plan.kind != ROUTE_GENERAL)
      if (int rc2 = stream_lists(dev, st, two_stage, &bail, &slist, &lent)) return rc2;
    // the lists' event likewise
    RecordOnExit list_use{lent ? lent->ev : nullptr, lent ? &lent->ev_set : nullptr, st};
    // a launch that fails after an earlier one of this chunk has queued leaves
    // the slot half used: zero it behind the queued work before reporting
    // (and wait for that work: the queued per-lane kernel reads its windows
    // from the caller's digest rows and writes its outputs there, and a caller
    // that gets an error may free or reuse its buffers at once -- a next call
    // into the same memory would find its rows overwritten under it.  The
    // failure path only, so the wait under g_mu holds up nothing that matters.)
    auto fail = [&](hipError_t e) {
      (void)hipMemsetAsync(slot, 0, SLOT_U64 * sizeof(unsigned long long), st);
      (void)hipStreamSynchronize(st);
      return hip_fail(e);
    };
    if (plan.kind == ROUTE_FF1 || plan.kind == ROUTE_FFP) {
      // FF1_OVERSUB x the resident blocks (PXB_FF1_OVERSUB / PXB_FFP_OVERSUB=k: k, A/B)
      const int over = plan.kind == ROUTE_FF1 ? hk.ff1_oversub : hk.ffp_oversub;
      const uint64_t fres = (uint64_t)eocc * (uint64_t)cus * (over ? (uint64_t)over : FF1_OVERSUB);
      const unsigned fgrid = (unsigned)std::min<uint64_t>((nc + 255) / 256, fres);
      hipError_t e;
      if (plan.kind == ROUTE_FF1) {
        ff1::Ff1Params fp;
        memset(&fp, 0, sizeof(fp));
        e = launch_fault_free(ffn, fp, fgrid, fn, (unsigned)resident, st, kp, bail, plan.cap, hk.ff1_bail);
      } else {
        ffp::FfpParams fp;
        memset(&fp, 0, sizeof(fp));
        fp.n_prop = cfg->n_proposers;
        fp.n_ticks = kp.n_ticks;
        fp.tick_period = kp.tick_period;
        e = launch_fault_free(pfn, fp, fgrid, fn, (unsigned)resident, st, kp, bail, plan.cap, hk.ff1_bail);
      }
      if (e) return fail(e);
    } else if (plan.kind == ROUTE_EV) {
      // the last per-lane stage over the chunk, or (two-stage) the first one
      // over the chunk and the last over its list; then the general kernel
      // over the last stage's bailed ids
      ev::EvKParams ek;
      memset(&ek, 0, sizeof(ek));
      ek.p = ev::make_params(cfg);
      ek.p.first_instance = kp.first_instance;
      ek.n_instances = (uint32_t)nc;
      ek.out = kp.out;
      ek.dig = kp.dig;
      ek.acc = kp.acc;
      ek.part = kp.part + ROWS_U64;
      ek.queue = kp.queue + Q_EV;
      ek.bail_ids = bail;
      ek.bail_n = kp.queue + Q_BAIL;
      ek.bail_cap = plan.cap;
      // The window pre-pass (paxos_win.hip): with a digest buffer, the chunk's
      // isolation windows are drawn densely into its digest rows and every
      // per-lane stage loads them in its refill.  A row keeps its windows until
      // its instance finishes (a handed-on instance's is never written), so the
      // second stage reads what this one pass left.  Without a digest buffer
      // (totals-only runs), or when no instance can draw a window, the refill
      // draws as before.  PXB_NO_WIN_PREPASS=1 turns it off.
      if (kp.dig && !hk.no_win_prepass && (ek.p.cfg & (ev::EV_CFG_CRASHY | ev::EV_CFG_RANDOMIZE))) {
        if (hipError_t e = ev::launch_windows(ek.p, N, (uint32_t)nc, kp.dig, st)) return fail(e);
        ek.win = kp.dig;
      }
      if (two_stage) {
        ev::EvKParams sk = ek;
        sk.bail_ids = slist;
        sk.bail_cap = plan.first_cap;
        const unsigned sgrid = (unsigned)std::min<uint64_t>((nc + 63) / 64, (uint64_t)socc * (uint64_t)cus);
#ifdef PXB_WAVE_TIMES   // (two-stage: the first per-lane launch's timeline)
        if (int rc2 = wave_times_buf(sgrid, &sk.dbg)) return rc2;
#endif
        hipLaunchKernelGGL(sfn, dim3(sgrid), dim3(64), 0, st, sk);
        if (hipError_t e = hipGetLastError()) return fail(e);
        // (tests: a launch failure right after the first per-lane launch)
        if (hk.fail_after_first) return fail(hipErrorLaunchFailure);
        ek.ids = slist;
        ek.n_ids = kp.queue + Q_BAIL;
        ek.ids_cap = plan.first_cap;
        ek.queue = kp.queue + Q_EV2;
        ek.bail_n = kp.queue + Q_BAIL2;
      }
      const unsigned egrid = (unsigned)std::min<uint64_t>((nc + 63) / 64, (uint64_t)eocc * (uint64_t)cus);
#ifdef PXB_WAVE_TIMES
      if (!two_stage)
        if (int rc2 = wave_times_buf(egrid, &ek.dbg)) return rc2;
#endif
      hipLaunchKernelGGL(efn, dim3(egrid), dim3(64), 0, st, ek);
      if (hipError_t e = hipGetLastError()) return fail(e);
      if (hk.fail_after_first) return fail(hipErrorLaunchFailure);
      if (hipError_t e = launch_general(fn, (unsigned)resident, st, kp, bail, plan.bail_word, plan.cap)) return fail(e);
    } else {
      const uint64_t blocks_needed = ((nc + G - 1) / G + wpb - 1) / wpb;
      const unsigned grid = (unsigned)std::min<uint64_t>(blocks_needed, resident);
#ifdef PXB_WAVE_TIMES
      if (grid * fn.wpb > 65536) return PXB_E_INVAL;
      if (int rc2 = wave_times_buf(grid * fn.wpb, &kp.dbg)) return rc2;
#endif
      HIPCHK(launch_general(fn, grid, st, kp));
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(TCOPIES), 0, st, kp.part, kp.part + ROWS_U64, kp.queue,
                       plan.bail_word, plan.cap, totals, g_slots[dev] + HAND_U64);
    if (hipError_t e = hipGetLastError()) return fail(e);
  }
  return PXB_OK;
}

int pxb_run(const pxb_config* cfg, pxb_result* out, uint32_t* log_digest, pxb_acceptor_rec* acc,
            pxb_counters* totals) {
  int rc = validate(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PXB_E_NODEV;
  const uint64_t n = cfg->n_instances, N = cfg->n_acceptors;
  StagePlan plan;                                 // results | digests | acceptor records | totals: one block
  const StageRegion r_out = plan.add(sizeof(pxb_result), out ? n : 0);
  const StageRegion r_dig = plan.add(N * sizeof(uint32_t), log_digest ? n : 0);
  const StageRegion r_acc = plan.add(N * sizeof(pxb_acceptor_rec), acc ? n : 0), r_tot = plan.add(sizeof(int64_t), PXB_NCOUNTERS);
  host::Staging S(plan);
  S.zero(r_tot);
  if (S.ok())
    S.note(pxb_run_device(cfg, S.ptr<pxb_result>(r_out), S.ptr<uint32_t>(r_dig), S.ptr<pxb_acceptor_rec>(r_acc),
                          S.ptr<int64_t>(r_tot), nullptr));
  S.sync();
  S.down(r_out, out, n);
  S.down(r_dig, log_digest, n);
  S.down(r_acc, acc, n);
  S.down(r_tot, totals ? totals->c : nullptr, PXB_NCOUNTERS);
  return S.finish();
}

extern "C" int pxb_query_validate(const pxb_query* q, const void* ids, uint64_t capacity, const void* n_matches,
                                  const void* hist_steps, const void* hist_rounds);   // paxos_query.hip

// Chunk by chunk (sweep_plan.h): run into the one result buffer, then query it
// on the same stream with the running cursor.  The query is a vanishing part
// of a chunk's time, so nothing overlaps; the device holds one chunk of
// results, the match list and the bins, whatever n_instances is.
int pxb_sweep(const pxb_config* cfg, const pxb_query* q, uint64_t* ids, pxb_result* matched, uint64_t capacity,
              uint64_t* n_matches, int64_t* hist_steps, int64_t* hist_rounds, pxb_counters* totals) {
  int rc = validate(cfg);
  if (rc) return rc;
  if ((rc = pxb_query_validate(q, ids, capacity, n_matches, hist_steps, hist_rounds))) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PXB_E_NODEV;
  const uint64_t n = cfg->n_instances, chunk = hooks().sweep_chunk;
  const uint64_t cap = std::min(capacity, n);            // (no more matches than instances)
  const uint64_t nh = q->n_bins_steps, nr = q->n_bins_rounds;
  StagePlan plan;                                 // a chunk's results | ids | matched | bins | bins | cursor | totals
  const StageRegion r_res = plan.add(sizeof(pxb_result), std::min(n, chunk));
  const StageRegion r_ids = plan.add(sizeof(uint64_t), cap), r_matched = plan.add(sizeof(pxb_result), matched ? cap : 0);
  const StageRegion r_hs = plan.add(sizeof(int64_t), nh), r_hr = plan.add(sizeof(int64_t), nr);
  const StageRegion r_cur = plan.add(sizeof(uint64_t), 1), r_tot = plan.add(sizeof(int64_t), PXB_NCOUNTERS);
  host::Staging S(plan);
  S.zero(r_cur), S.zero(r_tot), S.zero(r_hs), S.zero(r_hr);
  pxb_config c = *cfg;
  for (uint64_t k = 0, nk = sweep_n_chunks(n, chunk); k < nk && S.ok(); ++k) {
    const SweepChunk ch = sweep_chunk_at(cfg->first_instance, n, chunk, k);
    c.first_instance = ch.first;
    c.n_instances = ch.count;
    pxb_result* const d_res = S.ptr<pxb_result>(r_res);
    S.note(pxb_run_device(&c, d_res, nullptr, nullptr, S.ptr<int64_t>(r_tot), nullptr));
    if (S.ok())
      S.note(pxb_query_device(d_res, ch.first, ch.count, q, S.ptr<uint64_t>(r_ids), S.ptr<pxb_result>(r_matched), cap,
                              S.ptr<uint64_t>(r_cur), S.ptr<int64_t>(r_hs), S.ptr<int64_t>(r_hr), nullptr));
  }
  // (after a failed chunk, finish() waits: nothing is freed under queued work)
  S.sync();
  S.down(r_cur, n_matches, 1);
  const uint64_t nw = S.ok() ? std::min(*n_matches, cap) : 0;
  S.down(r_ids, ids, nw);
  S.down(r_matched, matched, nw);
  S.down(r_hs, hist_steps, nh);
  S.down(r_hr, hist_rounds, nr);
  S.down(r_tot, totals ? totals->c : nullptr, PXB_NCOUNTERS);
  return S.finish();
}

static int run_hook(bool acceptor, void* st, size_t st_bytes, uint32_t n_acc, const pxb_msg* in, pxb_msg* out,
                    size_t out_n, uint32_t* nb, uint32_t count) {
  if (!st || !in || !out || (!acceptor && !nb)) return PXB_E_INVAL;
  if (count == 0) return PXB_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PXB_E_NODEV;
  StagePlan plan;                                 // states | messages in | messages out | broadcast counts
  const StageRegion r_st = plan.add(st_bytes, count), r_in = plan.add(sizeof(pxb_msg), count);
  const StageRegion r_out = plan.add(sizeof(pxb_msg) * out_n, count);
  const StageRegion r_nb = plan.add(sizeof(uint32_t), acceptor ? 0 : count);
  host::Staging S(plan);
  S.up(r_st, st, count);
  S.up(r_in, in, count);
  if (S.ok()) {
    const unsigned grid = (count + 255) / 256;
    if (acceptor)
      hipLaunchKernelGGL(acceptor_hook_kernel, dim3(grid), dim3(256), 0, 0, S.ptr<pxb_acceptor_rec>(r_st),
                         S.ptr<const pxb_msg>(r_in), S.ptr<pxb_msg>(r_out), count);
    else
      hipLaunchKernelGGL(proposer_hook_kernel, dim3(grid), dim3(256), 0, 0, S.ptr<pxb_proposer_rec>(r_st), n_acc,
                         S.ptr<const pxb_msg>(r_in), S.ptr<pxb_msg>(r_out), S.ptr<uint32_t>(r_nb), count);
    S.note(hipGetLastError());
  }
  S.sync();
  S.down(r_st, st, count);
  S.down(r_out, out, count);
  S.down(r_nb, nb, count);
  return S.finish();
}

int pxb_acceptor_handle(pxb_acceptor_rec* states, const pxb_msg* req, pxb_msg* reply, uint32_t count) {
  return run_hook(true, states, sizeof(pxb_acceptor_rec), 0, req, reply, 1, nullptr, count);
}

int pxb_proposer_handle(pxb_proposer_rec* states, uint32_t n_acceptors, const pxb_msg* msg, pxb_msg* bcast,
                        uint32_t* n_bcast, uint32_t count) {
  if (n_acceptors < PXB_MIN_ACCEPTORS || n_acceptors > PXB_MAX_ACCEPTORS) return PXB_E_INVAL;
  return run_hook(false, states, sizeof(pxb_proposer_rec), n_acceptors, msg, bcast, 2, n_bcast, count);
}

}  // extern "C"
