// script_core.h — scripted schedules: what the script kernels
// (paxos_script.hip) and the host unit test (tests/native/script_host.cpp)
// share, as plain C++ over the per-lane state machine (paxos_ev.h).
//
// A script row (include/paxos_batch.h, docs/SEMANTICS.md §10) is one instance:
// a Philox base id plus overrides of its schedule draws, every field with a
// "keep" value that takes what Philox gives (cfg->seed, base).  Here:
//   the row layout (script_stride, offsets);
//   the instance's own draws by purpose (script_inst, script_skew,
//   script_window, script_link), the per-entry functions of the extract kernel
//   (script_row_byte: the fully explicit row, one byte at a time);
//   ScriptDraws, the draw source of a scripted lane (EvLane's Src), and
//   script_begin / script_sent, the lane's start and its per-link send counts.
// The draw and the start take what reads a link byte and what reads a skew or
// a window as neutral as template parameters (source_draw_over,
// script_begin_sel): the shrinker's candidates (shrink_core.h) are the same
// lane over a row read through a rank table.
//
// The scripted lane leaves the state machine as it is: it runs with
// lossy = true, loss_m1 = 0, dmax = 16 and no Tick-skew or window draws of its
// own, and its draw source hands back synthetic words that decode to the
// resolved outcome: w.x = lost ? 0 : 1 (lost iff w.x <= 0), w.y = (d - 1) << 28
// (1 + mulhi(w.y, 16) = d, d <= 15), skews as skew << 16 against skew_max =
// 0xFFFF.  The resolved outcome is the row's override, or the real draw
// against the instance's own thresholds.
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "paxos_ev.h"

namespace pxb {
namespace ev {

constexpr uint32_t SCR_HDR = 16u;                 // base, n_proposers, reserved, skew[3]
constexpr uint32_t SCR_KEEP8 = 0xFFu, SCR_KEEP16 = 0xFFFFu;

__host__ __device__ inline uint64_t script_links_off(uint32_t N) { return SCR_HDR + 4ull * N; }
__host__ __device__ inline uint64_t script_links_bytes(uint32_t P, uint32_t N, uint32_t depth) {
  return 2ull * P * N * depth;
}
__host__ __device__ inline uint64_t script_stride(uint32_t P, uint32_t N, uint32_t depth) {
  return (script_links_off(N) + script_links_bytes(P, N, depth) + 7ull) & ~7ull;
}
__host__ __device__ __forceinline__ uint32_t script_ld16(const uint8_t* r, uint32_t off) {
  return (uint32_t)r[off] | ((uint32_t)r[off + 1u] << 8);
}

// ---- what Philox gives (seed, lo | hi << 32), by purpose (SEMANTICS §4) ----
struct ScriptInst {
  uint32_t P, dmax, loss_m1, crash_m1;
  bool lossy, crashy;
};
// the instance's own parameters: the launch's, or (fuzzed batches) its draw, as EvLane::init takes it
__host__ __device__ inline ScriptInst script_inst(const EvParams& kp, uint32_t lo, uint32_t hi) {
  ScriptInst si;
  si.P = kp.n_prop;
  si.dmax = kp.delay_max;
  si.lossy = (kp.cfg & EV_CFG_LOSSY) != 0u;
  si.crashy = (kp.cfg & EV_CFG_CRASHY) != 0u;
  si.loss_m1 = kp.loss_m1;
  si.crash_m1 = kp.crash_m1;
  if (kp.cfg & EV_CFG_RANDOMIZE) {
    const uint4 w = philox(lo, hi, 0u, 4u << 24, kp.k0, kp.k1);
    si.P = 1u + mulhi_n(w.x, kp.n_prop);
    const uint64_t lt = ev_threshold(mulhi_n(w.y, kp.loss_ppm + 1u));
    si.dmax = 1u + mulhi_n(w.z, kp.delay_max);
    const uint64_t ct = ev_threshold(mulhi_n(w.w, kp.crash_ppm + 1u));
    si.lossy = lt != 0ull;
    si.loss_m1 = (uint32_t)(lt - 1ull);
    si.crashy = ct != 0ull;
    si.crash_m1 = (uint32_t)(ct - 1ull);
  }
  return si;
}
// the Tick step of proposer p (p < 3)
__host__ __device__ inline uint32_t script_skew(const EvParams& kp, uint32_t lo, uint32_t hi, uint32_t p) {
  if (kp.skew_max == 0u) return 0u;
  const uint4 w = philox(lo, hi, 0u, 2u << 24, kp.k0, kp.k1);
  return mulhi_n(p == 0u ? w.x : p == 1u ? w.y : w.z, kp.skew_max + 1u);
}
// the isolation window of acceptor a: c0 | c1 << 16, clamped to 4096 (0: none)
__host__ __device__ inline uint32_t script_window(const EvParams& kp, const ScriptInst& si, uint32_t lo, uint32_t hi,
                                                  uint32_t a) {
  if (!si.crashy) return 0u;
  return window_of(kp, philox(lo, hi, 0u, (3u << 24) | a, kp.k0, kp.k1), si.crash_m1);
}
// a message draw as a link byte: 0 = lost, else its delay (1..15)
__host__ __device__ __forceinline__ uint32_t script_link(const ScriptInst& si, const uint4& w) {
  const bool lost = si.lossy & (w.x <= si.loss_m1);
  return lost ? 0u : 1u + mulhi_n(w.y, si.dmax);
}
__host__ __device__ __forceinline__ uint32_t script_msg_ctr(uint32_t dirn, uint32_t p, uint32_t a) {
  return (1u << 24) | (dirn << 16) | (p << 8) | a;
}

// Byte j (j < script_stride) of the fully explicit row of instance `id`: the
// drawn P, the skews, the windows and every link byte of the proposers the
// instance has; links of absent proposers are 0xFF, skews of absent proposers
// and the padding 0.  Pure Philox; no state machine runs.
__host__ __device__ inline uint8_t script_row_byte(const EvParams& kp, uint32_t P, uint32_t N, uint32_t depth,
                                                   uint64_t id, uint64_t j) {
  const uint32_t lo = (uint32_t)id, hi = (uint32_t)(id >> 32);
  if (j < 8u) return (uint8_t)(id >> (8u * (uint32_t)j));
  if (j == 9u) return 0u;
  const ScriptInst si = script_inst(kp, lo, hi);
  if (j == 8u) return (uint8_t)si.P;
  if (j < SCR_HDR) {
    const uint32_t p = ((uint32_t)j - 10u) >> 1;
    const uint32_t v = p < si.P ? script_skew(kp, lo, hi, p) : 0u;
    return (uint8_t)(v >> (8u * ((uint32_t)j & 1u)));
  }
  const uint64_t loff = script_links_off(N);
  if (j < loff) {
    const uint32_t o = (uint32_t)j - SCR_HDR;
    return (uint8_t)(script_window(kp, si, lo, hi, o >> 2) >> (8u * (o & 3u)));
  }
  const uint64_t e = j - loff;
  if (depth == 0u || e >= script_links_bytes(P, N, depth)) return 0u;
  const uint32_t k = (uint32_t)(e % depth), l = (uint32_t)(e / depth);   // l = (dirn * P + p) * N + a
  const uint32_t a = l % N, dp = l / N, p = dp % P, dirn = dp / P;
  if (p >= si.P) return (uint8_t)SCR_KEEP8;
  return (uint8_t)script_link(si, philox(lo, hi, k, script_msg_ctr(dirn, p, a), kp.k0, kp.k1));
}

// ---- the scripted lane ----
// The draw source (EvLane's Src).  Message draws (purpose 1) decode (c2, c3) to
// (dirn, p, a, k) and resolve the row's byte; the Tick-skew draw (purpose 2)
// hands back the resolved skews.  Any counter the lane asks for is answered
// without a load outside the row: an index beyond the table is "keep".
// (a base class of the lane, EvLane : Src: the s_ names keep clear of the lane's own)
struct ScriptDraws {
  static constexpr bool kPhilox = false;
  const uint8_t* s_links;             // [dirn][p][a][k]
  uint32_t s_depth, s_P, s_N;         // the table's dimensions (the call's)
  uint32_t s_dclamp;                  // cfg->delay_max: what an override's delay is clamped to
  uint32_t s_skew[3];                 // the resolved Tick steps
  uint32_t s_dmax, s_loss_m1;         // the instance's own thresholds (keep entries)
  bool s_lossy;

  // the draw over `byte_at(index)`, what reads a link byte of the table (the
  // shrinker's candidates read it beside their rank table: shrink_core.h)
  template <class ByteAt>
  __host__ __device__ __forceinline__ uint4 source_draw_over(uint32_t lo, uint32_t hi, uint32_t c2, uint32_t c3,
                                                             const uint32_t (&rk)[20], const ByteAt& byte_at) const {
    if ((c3 >> 24) == 2u) return make_uint4(s_skew[0] << 16, s_skew[1] << 16, s_skew[2] << 16, 0u);
    const uint32_t dirn = (c3 >> 16) & 0xFFu, p = (c3 >> 8) & 0xFFu, a = c3 & 0xFFu, k = c2;
    const bool in = ((c3 >> 24) == 1u) & (dirn < 2u) & (p < s_P) & (a < s_N) & (k < s_depth);
    uint32_t b = SCR_KEEP8;
    if (in) b = byte_at(((uint64_t)((dirn * s_P + p) * s_N + a)) * s_depth + k);
    // an override: lost, or its delay clamped; keep: the real draw against the
    // instance's own thresholds.  The Philox rounds run for every entry, beside
    // the byte's load.  (Running them only for keep entries, a branch behind the
    // load, is not settled: separate MI355X sessions at depth 64 differ by more
    // than the variants do; DESIGN §3 has the figures)
    const uint4 w = philox_rk(lo, hi, c2, c3, rk);
    const bool keep = b == SCR_KEEP8;
    const bool lost = keep ? s_lossy & (w.x <= s_loss_m1) : b == 0u;
    uint32_t d = keep ? 1u + mulhi_n(w.y, s_dmax) : (b < s_dclamp ? b : s_dclamp);
    d = d < 1u ? 1u : (d > 15u ? 15u : d);         // (a lost message's delay is unused; PXB_MAX_DELAY = 15)
    return make_uint4(lost ? 0u : 1u, (d - 1u) << 28, 0u, 0u);
  }
  struct RowByte {
    const uint8_t* links;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return links[i]; }
  };
  __host__ __device__ __forceinline__ uint4 source_draw(uint32_t lo, uint32_t hi, uint32_t c2, uint32_t c3,
                                                        const uint32_t (&rk)[20]) const {
    return source_draw_over(lo, hi, c2, c3, rk, RowByte{s_links});
  }
};

// Starts the lane on `row` (L.m and L.set_keys(kp) done): PXB_TRACE_OK, or
// PXB_SCRIPT_BAD for a malformed row (the lane is then not started).  P, N:
// the call's; the lane's shape holds P proposers.  `neutral(t)`: the skew of
// proposer t (t < 3) or the window of acceptor t - 3 reads as 0 / none (the
// shrinker's virtual candidates, shrink_core.h); script_begin: never.
struct ScriptNoNeutral {
  __host__ __device__ __forceinline__ bool operator()(uint32_t) const { return false; }
};
template <class Lane, class Neutral>
__host__ __device__ __forceinline__ uint32_t script_begin_sel(Lane& L, const EvParams& kp, uint32_t depth,
                                                              const uint8_t* row, const Neutral& neutral) {
  constexpr uint32_t P = Lane::S::PM, N = Lane::S::N;
  static_assert(!Lane::S::SP && !Lane::S::CMP && !Lane::S::SL, "the generic shape");
  const uint32_t lo = script_ld16(row, 0) | (script_ld16(row, 2) << 16);
  const uint32_t hi = script_ld16(row, 4) | (script_ld16(row, 6) << 16);
  const uint32_t np = row[8];
  if ((np > P) | (row[9] != 0u)) return PXB_SCRIPT_BAD;
  const ScriptInst si = script_inst(kp, lo, hi);
  ScriptDraws& D = L;                 // (the lane's draw source: its base class, or that one's)
  D.s_links = row + script_links_off(N);
  D.s_depth = depth;
  D.s_P = P;
  D.s_N = N;
  D.s_dclamp = kp.delay_max;
  D.s_dmax = si.dmax;
  D.s_loss_m1 = si.loss_m1;
  D.s_lossy = si.lossy;
#pragma unroll
  for (uint32_t p = 0; p < 3u; ++p) {
    const uint32_t v = script_ld16(row, 10u + 2u * p);
    D.s_skew[p] = neutral(p) ? 0u : v == SCR_KEEP16 ? script_skew(kp, lo, hi, p) : v;
  }
  // the lane's own parameters: no draws of its own, synthetic thresholds
  EvParams pl = kp;
  pl.first_instance = (uint64_t)lo | ((uint64_t)hi << 32);
  pl.cfg = EV_CFG_LOSSY | EV_CFG_DRAWS;
  pl.n_prop = np ? np : si.P;
  pl.delay_max = 16u;
  pl.loss_m1 = 0u;
  pl.skew_max = 0xFFFFu;
  L.init(pl, 0u);
  // (the windows are first read by the acceptor op: set after init)
#pragma unroll
  for (uint32_t a = 0; a < N; ++a) {
    uint32_t c0 = script_ld16(row, SCR_HDR + 4u * a), c1 = script_ld16(row, SCR_HDR + 4u * a + 2u);
    uint32_t wv;
    if ((c0 == SCR_KEEP16) & (c1 == SCR_KEEP16)) {
      wv = script_window(kp, si, lo, hi, a);
    } else {
      c0 = c0 < 4096u ? c0 : 4096u;
      c1 = c1 < 4096u ? c1 : 4096u;
      wv = c0 >= c1 ? 0u : c0 | (c1 << 16);
    }
    L.win[a] = neutral(3u + a) ? 0u : wv;
  }
  return PXB_TRACE_OK;
}
template <class Lane>
__host__ __device__ __forceinline__ uint32_t script_begin(Lane& L, const EvParams& kp, uint32_t depth,
                                                          const uint8_t* row) {
  return script_begin_sel(L, kp, depth, row, ScriptNoNeutral{});
}

// messages sent on each link of an ended instance (the seqs consumed), in the
// row's link order [dirn][p][a]: the broadcasts of p (each tries every
// acceptor), the replies of a to p
template <class Lane>
__host__ __device__ __forceinline__ void script_sent(const Lane& L, uint16_t* out) {
  constexpr uint32_t P = Lane::S::PM, N = Lane::S::N;
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t a = 0; a < N; ++a) {
      out[p * N + a] = (uint16_t)(p < L.P ? L.nsent_of(p) : 0u);
      out[(P + p) * N + a] = (uint16_t)(p < L.P ? L.m.ld16(Lane::S::RSEQ, a * P + p) : 0u);
    }
}

}  // namespace ev
}  // namespace pxb
