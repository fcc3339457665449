// events_core.h — per-message handler events of scripted rows
// (include/paxos_batch.h: pxb_trace_events, docs/SEMANTICS.md §13): what the
// event kernels (paxos_events.hip) and the host unit test
// (tests/native/events_host.cpp) share, as plain C++ over the scripted lane
// (script_core.h, script_lane.h).
//
//   EventDraws   ScriptDraws with kTap = true: the acceptor op and the proposer
//                op of paxos_ev.h leave what they handled and produced in its
//                plain members (an iteration runs at most one of each);
//   EventLane    the analogue of TraceLane: one row, one iteration at a time,
//                the taps turned into at most two events that are counted, or
//                written in the lane's own order (the staging order);
//   event_place  the reorder step, one staged event at a time: the lane emits
//                each actor's events in the canonical order but interleaves an
//                acceptor op and a proposer op per iteration, so within a step
//                segment an event goes behind those of a smaller (phase, actor
//                index) and those of its own key emitted before it.
//
// The scripted shapes run the default (end-of-step) variant: all events of step
// s are emitted before any of step s + 1, so a row's step segment is contiguous
// in the staging order.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "script_lane.h"

namespace pxb {
namespace ev {

static_assert(sizeof(pxb_trace_event) == 96 && sizeof(pxb_msg) == 16 && sizeof(pxb_trace_prop) == 32 &&
                  sizeof(pxb_acceptor_rec) == 16,
              "pxb_trace_event: 96 bytes");
constexpr uint32_t EVT_WORDS = 24u;               // a pxb_trace_event as 32-bit words
// a step segment of one row: every request FIFO and every response FIFO of the
// generic shape drained, and a Tick per proposer (P N QC + P (1 + N RC))
constexpr uint32_t EVT_SEG_MAX = 256u;

struct EventDraws : ScriptDraws {
  static constexpr bool kTap = true;
  // the iteration's acceptor op: whether it took a request, which acceptor and
  // proposer, the request, live / dead / isolated, whether it replied, the reply
  // word (paxos_ev.h Layouts) and, in log mode, the Round1OK's 14-bit command
  bool e_acc, e_snd;
  uint32_t e_a, e_ap, e_kind, e_x, e_z, e_fate, e_pw, e_rz;
  // the iteration's proposer op: whether it took an input, which proposer, 0 for
  // its Tick or 1 + the acceptor, the response, the handler's broadcast (kind,
  // ticket), the restart's ticket, the command, whether the restart's
  // AskForTicket follows
  bool e_pin, e_spd;
  uint32_t e_q, e_r, e_rkind, e_px, e_py, e_pz, e_k0, e_x0, e_x1, e_c2n;

  __host__ __device__ __forceinline__ void tap_acc(bool acc, uint32_t a, uint32_t p, uint32_t kind, uint32_t x,
                                                   uint32_t z, uint32_t fate, bool snd, uint32_t pw, uint32_t rz) {
    e_acc = acc, e_a = a, e_ap = p, e_kind = kind, e_x = x, e_z = z, e_fate = fate, e_snd = snd, e_pw = pw, e_rz = rz;
  }
  __host__ __device__ __forceinline__ void tap_prop(bool pin, uint32_t q, uint32_t r, uint32_t rkind, uint32_t px,
                                                    uint32_t py, uint32_t pz, uint32_t k0, uint32_t x0, uint32_t x1,
                                                    uint32_t c2n, bool spd) {
    e_pin = pin, e_q = q, e_r = r, e_rkind = rkind, e_px = px, e_py = py, e_pz = pz, e_k0 = k0, e_x0 = x0, e_x1 = x1,
    e_c2n = c2n, e_spd = spd;
  }
};

// 24 words to an event: six 16-byte stores on the device (the entry points check
// the alignment); on the host the caller's buffer, of which none is known
__host__ __device__ __forceinline__ void event_store(pxb_trace_event* o, const uint32_t (&w)[EVT_WORDS]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* const q = reinterpret_cast<uint4*>(o);
#pragma unroll
  for (int i = 0; i < 6; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
#else
  memcpy(reinterpret_cast<unsigned char*>(o), w, sizeof(pxb_trace_event));
#endif
}

// One row of pxb_trace_events on one lane.  The caller runs
//   begin_count / begin_write;  script_begin(L, ...);  while (E.iter(L, p)) {}
// Count pass: n = the events whose step lies in [smin, smax]; status and result
// are the row's.  Write pass (the lane is deterministic: the same events again):
// in-window event j goes to out[j] while j < room, and the lane stops once no
// later event can be kept.
template <class Lane>
struct EventLane {
  static_assert(!Lane::kEarly, "the end-of-step variant: a step's events before the next step's");
  static_assert(!Lane::S::SP, "every Tick passes the proposer op");
  static_assert((uint32_t)Lane::S::PM * Lane::S::N * Lane::S::QC +
                        (uint32_t)Lane::S::PM * (1u + (uint32_t)Lane::S::N * Lane::S::RC) <= 246u,
                "a step segment: at most 246 events");
  uint32_t smin, smax;
  uint32_t n;                       // in-window events so far
  pxb_trace_event* out;             // write pass: this row's first staged event (count pass: null)
  uint32_t total;                   // write pass: the count pass's n
  uint64_t room;
  uint32_t status;
  uint32_t res[4];

  __host__ __device__ void begin_count(uint32_t step_min, uint32_t step_max) {
    smin = step_min;
    smax = step_max;
    n = 0u;
    out = nullptr;
    total = 0u;
    room = 0ull;
    status = PXB_TRACE_OK;
    res[0] = res[1] = res[2] = res[3] = 0u;
  }
  // cnt: the count pass's n of this row (> 0), o: where its first event is
  // staged, room_: events that fit from there (> 0)
  __host__ __device__ void begin_write(uint32_t step_min, uint32_t step_max, uint32_t cnt, pxb_trace_event* o,
                                       uint64_t room_) {
    begin_count(step_min, step_max);
    out = o;
    total = cnt;
    room = room_;
  }

  // a command of the lane (2 bits, log mode 14) as the ABI's code; 0: Nothing
  __host__ __device__ static __forceinline__ uint32_t code(uint32_t v) { return v ? Lane::code_of(v) : 0u; }

  __host__ __device__ __forceinline__ void put(const uint32_t (&w)[EVT_WORDS], bool on) {
    if (on) {
      if (out && (uint64_t)n < room) event_store(out + n, w);
      n += 1u;
    }
  }

  // The acceptor op's event.  The state after: the acceptor's words through the
  // lane's own selects (a per-lane index into its register arrays would move
  // them to scratch memory), decoded by what record_of / digest_of decode them with.
  __host__ __device__ __forceinline__ void acc_event(const Lane& L, uint32_t step, uint32_t (&w)[EVT_WORDS]) const {
    constexpr bool LG = Lane::S::LG;
    const uint32_t a = L.e_a;
    const bool prop = L.e_kind == PROPOSE;
    w[0] = step;
    w[1] = PXB_EVT_ACCEPTOR | (a << 8) | (L.e_ap << 16) | (L.e_fate << 24);
    w[2] = L.e_snd ? 1u : 0u;
    w[3] = 0u;
    w[4] = L.e_kind, w[5] = L.e_x, w[6] = 0u, w[7] = prop ? code(L.e_z) : 0u;
    const uint32_t pw = L.e_pw, rk = pw >> 30;
    const bool r1 = L.e_snd & (rk == R1OK);
    const uint32_t rz = LG ? L.e_rz : (pw >> 24) & 3u;
    w[8] = L.e_snd ? rk : 0u;
    w[9] = (L.e_snd & (rk != R2S)) ? pw & 0xFFFu : 0u;
    w[10] = r1 ? (pw >> 12) & 0xFFFu : 0u;
    w[11] = r1 ? code(rz) : 0u;
    w[12] = w[13] = w[14] = w[15] = 0u;
    const uint32_t A = Lane::get(L.accw, a), D = Lane::get(L.accd, a);
    uint32_t V = A;
    if constexpr (LG) V = Lane::get(L.accv, a);
    uint32_t r[4];
    Lane::w_record(A, V, r);
    w[16] = r[0], w[17] = r[1], w[18] = r[2], w[19] = r[3];
    w[20] = Lane::w_digest(D, Lane::w_log_len(V));
    w[21] = w[22] = w[23] = 0u;
  }

  // The proposer op's event; the state after is trace_record's conversion of proposer q's words
  __host__ __device__ __forceinline__ void prop_event(const Lane& L, uint32_t step, uint32_t (&w)[EVT_WORDS]) const {
    constexpr bool LG = Lane::S::LG;
    const uint32_t q = L.e_q;
    const bool tick = L.e_r == 0u, r1 = !tick & (L.e_rkind == R1OK);
    const bool b0 = L.e_k0 != NONE;
    w[0] = step;
    w[1] = PXB_EVT_PROPOSER | (q << 8) | ((tick ? PXB_EVT_PEER_TICK : L.e_r - 1u) << 16) | (PXB_EVT_HANDLED << 24);
    w[2] = (b0 ? 1u : 0u) + (L.e_spd ? 1u : 0u);
    w[3] = 0u;
    w[4] = tick ? 3u : L.e_rkind;
    w[5] = (tick | (L.e_rkind == R2S)) ? 0u : L.e_px;
    w[6] = r1 ? L.e_py : 0u;
    w[7] = r1 ? code(L.e_pz) : 0u;
    w[8] = b0 ? L.e_k0 : 0u, w[9] = b0 ? L.e_x0 : 0u, w[10] = 0u;
    w[11] = (b0 & (L.e_k0 == PROPOSE)) ? code(L.e_c2n) : 0u;
    w[12] = 0u /* ASK */, w[13] = L.e_spd ? L.e_x1 : 0u, w[14] = w[15] = 0u;
    uint32_t w2 = 0u;
    if constexpr (LG) w2 = Lane::get(L.pw2, q);
    pxb_trace_prop t = {0, 0, 0, 0, 0, 0, 0, 0};
    trace_prop<Lane>(Lane::get(L.pw0, q), Lane::get(L.pw1, q), w2, q, t);
    w[16] = (uint32_t)t.ticket, w[17] = t.cmd, w[18] = t.acks, w[19] = t.state;
    w[20] = (uint32_t)t.mr_t, w[21] = t.mr_v, w[22] = t.r2_v, w[23] = t.pending;
  }

  // one iteration of the state machine; false once the lane has nothing left to do
  __host__ __device__ __forceinline__ bool iter(Lane& L, const EvParams& p) {
    const uint32_t s0 = (uint32_t)L.s;
    // write pass: past the window, the count or the room, nothing later is kept
    if (out && (n == total || s0 > smax || (uint64_t)n >= room)) return false;
    EvOut o;
    const bool done = L.step(p, o);
    if (L.bailed) {                 // beyond the link capacities: no events, a zeroed result
      status = PXB_TRACE_BAILED;
      n = 0u;
      return false;
    }
    const bool in = (s0 >= smin) & (s0 <= smax);
    uint32_t w[EVT_WORDS];
    if (any_lane(in & L.e_acc)) {
      acc_event(L, s0, w);
      put(w, in & L.e_acc);
    }
    if (any_lane(in & L.e_pin)) {
      prop_event(L, s0, w);
      put(w, in & L.e_pin);
    }
    if (done) {
      res[0] = o.res[0];
      res[1] = o.res[1];
      res[2] = o.res[2];
      res[3] = o.res[3];
      return false;
    }
    return true;
  }
};

// ---- the reorder step ----
// the sort key of a staged event within its step segment: phase, then actor index
__host__ __device__ __forceinline__ uint32_t event_key(const pxb_trace_event* e) {
  return ((uint32_t)e->actor << 8) | e->index;
}

// Staged event t (t < staged; staging holds the first `staged` events of the
// call in the lanes' order, offsets[0 .. count] are the rows' first events):
// copied to its canonical place in out unless that is at or past `capacity`.
// Its row is the last one that starts at or before t; its segment, the staged
// events of that row with its step, is whole in the staging whenever it starts
// below capacity (staged >= min(total, capacity + EVT_SEG_MAX)).
__host__ __device__ inline void event_place(const pxb_trace_event* staging, uint64_t staged, const uint64_t* offsets,
                                            uint64_t count, uint64_t t, pxb_trace_event* out, uint64_t capacity) {
  uint64_t lo = 0, hi = count;      // the last row with offsets[row] <= t (offsets ascend, offsets[0] = 0)
  while (hi - lo > 1u) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (offsets[mid] <= t) lo = mid;
    else hi = mid;
  }
  const uint64_t r0 = offsets[lo], r1e = offsets[lo + 1u], r1 = r1e < staged ? r1e : staged;
  const uint32_t step = staging[t].step, key = event_key(staging + t);
  uint64_t s0 = t;
  while (s0 > r0 && staging[s0 - 1u].step == step) --s0;
  if (s0 >= capacity) return;       // (nothing of this segment is kept)
  uint64_t rank = 0;
  for (uint64_t j = s0; j < r1 && staging[j].step == step; ++j) {
    const uint32_t kj = event_key(staging + j);
    rank += (kj < key || (kj == key && j < t)) ? 1u : 0u;
  }
  const uint64_t dst = s0 + rank;
  if (dst >= capacity) return;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* const a = reinterpret_cast<const uint4*>(staging + t);
  uint4* const b = reinterpret_cast<uint4*>(out + dst);
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = a[i];
#else
  memcpy(reinterpret_cast<unsigned char*>(out + dst), staging + t, sizeof(pxb_trace_event));
#endif
}

}  // namespace ev
}  // namespace pxb
