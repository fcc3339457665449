// cover_core.h — handler-path coverage of scripted rows (include/paxos_batch.h:
// pxb_cover, docs/SEMANTICS.md §14): what the cover kernels (paxos_cover.hip)
// and the host unit test (tests/native/cover_host.cpp) share, as plain C++ over
// the scripted lane with the tapped draw source (events_core.h: EventDraws).
//
//   CoverLane    in EventLane's place: one row, one iteration at a time, the
//                taps of the iteration's acceptor op and proposer op turned into
//                the class bits of §14 and ORed into the row's mask.  Nothing is
//                stored per event.
//
// Every class depends on the event and on earlier events of the same actor
// only, so the lane's interleaved order (an acceptor op and a proposer op per
// iteration) gives the mask of the canonical order.  What a class needs of
// earlier events is kept packed:
//   granted   2 bits an acceptor: the peer of the last AskForTicket it granted (3: none)
//   accbits   bit a: fresh[a], the stored proposal is of the acceptor's current
//             ticket; bit 9 + a: the parity of its log length (a handled
//             Execute appends at most one entry)
//   seen      9 bits a proposer: the acceptors whose Round2Success it counted
//             since it last broadcast a Propose
// A proposer's state before its event is its words before L.step, copied
// through compile-time indices and selected by the tap's proposer afterwards.
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "events_core.h"

namespace pxb {
namespace ev {

static_assert(sizeof(pxb_cover_summary) == 4 * 8 + 32 * 8 + 32 * 8 + 32 * 4 + 8, "pxb_cover_summary: 680 bytes");
static_assert(sizeof(pxb_cover_query) == 16, "pxb_cover_query: 16 bytes");
static_assert(PXB_COVER_CLASSES == 29, "bits 0..28");

// a mask against a query (the row is PXB_TRACE_OK)
__host__ __device__ __forceinline__ bool cover_match(uint32_t m, uint32_t all, uint32_t any, uint32_t none) {
  return ((m & all) == all) & ((any == 0u) | ((m & any) != 0u)) & ((m & none) == 0u);
}

template <class Lane>
struct CoverLane {
  static_assert(!Lane::kEarly, "the end-of-step variant, as the event lane");
  static_assert(!Lane::S::SP, "every Tick passes the proposer op");
  static constexpr int PM = Lane::S::PM, N = Lane::S::N;
  static constexpr bool LG = Lane::S::LG;
  static_assert(N <= 9 && PM <= 3, "granted: 2 bits x 9, seen: 9 bits x 3");
  uint32_t mask;
  uint32_t granted, accbits, seen;
  uint32_t status;
  uint32_t res[4];

  __host__ __device__ void begin() {
    mask = 0u;
    granted = 0x3FFFFu;
    accbits = seen = 0u;
    status = PXB_TRACE_OK;
    res[0] = res[1] = res[2] = res[3] = 0u;
  }

  // the classes of the iteration's acceptor event (0 without one), and the acceptor's memory after it
  __host__ __device__ __forceinline__ uint32_t acc_class(const Lane& L) {
    const bool on = L.e_acc;
    const uint32_t a = on ? L.e_a : 0u, p = L.e_ap, kind = L.e_kind;
    const bool handled = on & (L.e_fate == PXB_EVT_HANDLED);
    // (a handled AskForTicket or Propose always replies: the reply word is the op's)
    const uint32_t rk = L.e_pw >> 30;
    const uint32_t rz = LG ? L.e_rz : (L.e_pw >> 24) & 3u;
    const uint32_t A = Lane::get(L.accw, a);
    uint32_t V = A;
    if constexpr (LG) V = Lane::get(L.accv, a);
    const uint32_t val = LG ? V & 0x3FFFu : (A >> 24) & 3u;
    const uint32_t len = Lane::w_log_len(V);
    const bool dead = ((A >> Lane::A_DEAD) & 1u) != 0u;
    const uint32_t g = (granted >> (2u * a)) & 3u;
    const bool fr = ((accbits >> a) & 1u) != 0u;
    const bool grew = ((accbits >> (9u + a)) & 1u) != (len & 1u);
    const bool ask = handled & (kind == ASK), prop = handled & (kind == PROPOSE), exec = handled & (kind == EXECUTE);
    const bool grant = ask & (rk == R1OK), accept = prop & (rk == R2S);
    uint32_t c = 0u;
    c |= (grant & (rz == 0u)) ? PXB_COVER_ASK_GRANT_EMPTY : 0u;
    c |= (grant & (rz != 0u)) ? PXB_COVER_ASK_GRANT_STORED : 0u;
    c |= (ask & !grant) ? PXB_COVER_ASK_NACK : 0u;
    c |= accept ? PXB_COVER_PROPOSE_ACCEPT : 0u;
    c |= (prop & !accept) ? PXB_COVER_PROPOSE_NACK : 0u;
    c |= (exec & grew) ? PXB_COVER_EXEC_APPLY : 0u;
    c |= (exec & !grew & !dead) ? PXB_COVER_EXEC_IGNORED : 0u;
    c |= (exec & dead) ? PXB_COVER_EXEC_PANIC : 0u;
    c |= (on & (L.e_fate == PXB_EVT_DISCARDED_DEAD)) ? PXB_COVER_DISCARD_DEAD : 0u;
    c |= (on & (L.e_fate == PXB_EVT_DISCARDED_ISOL)) ? PXB_COVER_DISCARD_ISOLATED : 0u;
    c |= (accept & (g != p)) ? PXB_COVER_Q1_FOREIGN_ACCEPT : 0u;
    c |= (exec & grew & !fr) ? PXB_COVER_Q7_STALE_EXEC : 0u;
    granted = grant ? (granted & ~(3u << (2u * a))) | (p << (2u * a)) : granted;
    const bool fresh = (val != 0u) & (((A >> 12) & 0xFFFu) == (A & 0xFFFu));
    const uint32_t nb = (accbits & ~((1u | (1u << 9)) << a)) | (((fresh ? 1u : 0u) | ((len & 1u) << 9)) << a);
    accbits = handled ? nb : accbits;
    return c;
  }

  // the classes of the iteration's proposer event (0 without one); b0, b1: the proposers' words before the iteration
  __host__ __device__ __forceinline__ uint32_t prop_class(const Lane& L, const uint32_t (&b0)[PM],
                                                          const uint32_t (&b1)[PM]) {
    const bool on = L.e_pin;
    const uint32_t q = on ? L.e_q : 0u;
    const bool tick = L.e_r == 0u;
    const uint32_t peer = tick ? 0u : L.e_r - 1u, rkind = L.e_rkind;
    const uint32_t w0 = Lane::get(b0, q), w1 = Lane::get(b1, q);
    const uint32_t bst = Lane::w_state(w0);
    const bool bmv = (LG ? w1 & 0x3FFFu : Lane::w_mr_v(w1)) != 0u;
    const uint32_t n_out = (L.e_k0 != NONE ? 1u : 0u) + (L.e_spd ? 1u : 0u);
    uint32_t w2 = 0u;
    if constexpr (LG) w2 = Lane::get(L.pw2, q);
    pxb_trace_prop t = {0, 0, 0, 0, 0, 0, 0, 0};
    trace_prop<Lane>(Lane::get(L.pw0, q), Lane::get(L.pw1, q), w2, q, t);
    const bool tk = on & tick, have = on & !tick & (rkind == HAVE), r1 = on & !tick & (rkind == R1OK);
    const bool r2 = on & !tick & (rkind == R2S);
    const bool r1c = r1 & (bst == ROUND1) & (Lane::w_ticket(w0) == L.e_px);
    const bool r1p = r1c & (n_out != 0u);
    const bool adopted = r1p & (t.pending != 0u);
    const bool r2c = r2 & (bst == ROUND2);
    const uint32_t sq = (seen >> (9u * q)) & 0x1FFu;
    uint32_t c = 0u;
    c |= (tk & (n_out != 0u)) ? PXB_COVER_TICK_START : 0u;
    c |= (tk & (n_out == 0u)) ? PXB_COVER_TICK_BUSY : 0u;
    c |= (have & (bst == IDLE)) ? PXB_COVER_HAVE_IDLE : 0u;
    c |= (have & (bst != IDLE) & (n_out == 0u)) ? PXB_COVER_HAVE_BELOW : 0u;
    c |= (have & (n_out != 0u) & (bst == ROUND1)) ? PXB_COVER_HAVE_RESTART_R1 : 0u;
    c |= (have & (n_out != 0u) & (bst == ROUND2)) ? PXB_COVER_HAVE_ABORT_R2 : 0u;
    c |= (r1 & !r1c) ? PXB_COVER_R1OK_STALE : 0u;
    c |= (r1c & (n_out == 0u)) ? PXB_COVER_R1OK_ACK : 0u;
    c |= (r1p & !adopted) ? PXB_COVER_R1OK_PROPOSE_OWN : 0u;
    c |= adopted ? PXB_COVER_R1OK_PROPOSE_ADOPTED : 0u;
    c |= (adopted & (t.r2_v == t.cmd)) ? PXB_COVER_Q5_ADOPTED_OWN : 0u;
    c |= (r1c & (L.e_pz != 0u) & bmv & (Lane::w_mr_t(w0) == L.e_py)) ? PXB_COVER_Q4_TIE : 0u;
    c |= (r2 & !r2c) ? PXB_COVER_R2S_DROPPED : 0u;
    c |= (r2c & (n_out == 0u)) ? PXB_COVER_R2S_ACK : 0u;
    c |= (r2c & (n_out == 1u)) ? PXB_COVER_R2S_DONE : 0u;
    c |= (r2c & (n_out == 2u)) ? PXB_COVER_R2S_RESTART : 0u;
    c |= (r2c & (((sq >> peer) & 1u) != 0u)) ? PXB_COVER_R2S_REPEAT : 0u;
    const uint32_t clr = seen & ~(0x1FFu << (9u * q)), add = seen | (1u << (9u * q + peer));
    seen = (on & (L.e_k0 == PROPOSE)) ? clr : (r2c ? add : seen);
    return c;
  }

  // one iteration of the state machine; false once the lane has nothing left to do
  __host__ __device__ __forceinline__ bool iter(Lane& L, const EvParams& p) {
    uint32_t b0[PM], b1[PM];
#pragma unroll
    for (int q = 0; q < PM; ++q) b0[q] = L.pw0[q], b1[q] = L.pw1[q];
    EvOut o;
    const bool done = L.step(p, o);
    if (L.bailed) {                 // beyond the link capacities: mask 0, a zeroed result
      status = PXB_TRACE_BAILED;
      mask = 0u;
      return false;
    }
    mask |= acc_class(L);
    mask |= prop_class(L, b0, b1);
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

}  // namespace ev
}  // namespace pxb
