// shrink_core.h — the batched shrinker (include/paxos_batch.h, docs/SEMANTICS.md
// §11): what the shrink kernels (paxos_shrink.hip) and the host unit test
// (tests/native/shrink_host.cpp) share, as plain C++ over script_core.h.
//
// A PARENT is one row being shrunk.  Its RANK TABLE has one uint16 per schedule
// entry of the row: the three skews (t = 0..2), the N windows (t = 3..3 + N - 1)
// and every link byte (t = 3 + N + e, e the byte's index in [dirn][p][a][k]
// order): ascending t is ascending row offset, the order of pxb.script_faults.
// An entry's rank is its index among the parent's candidates of the coming
// launch (singles: among its faults; prefixes: among the removable ones), or
// SHR_NONE.  CANDIDATE j of a parent is the parent's row with the entries of
// rank == j (singles) or rank <= j (prefixes) read as neutralised (skew 0,
// window none, link byte 1): ShrinkDraws and shrink_begin read the row and the
// table side by side, and no candidate row exists anywhere.
//
// Here: the entry decode, the per-entry fault test, the per-entry
// apply / settle step, a fault's signature record and the FNV-1a-64 fold, the
// candidate's draw source and start, the predicate, and the candidate kernel's
// parameters with what one lane does before its run (ShrParams::begin: the lane
// job of paxos_trace_core.h).  The walk over a
// parent's entries (a 64-lane wave with ballots on the device, a loop on the
// host) is the caller's.  The draw source and the start are written over the
// draw source beneath them, so that shrink_cover_core.h puts them on the tapped
// one (pxb_shrink_cover_batch).
#pragma once
#include <stdint.h>

#include "script_core.h"

namespace pxb {
namespace ev {

constexpr uint32_t SHR_NONE = 0xFFFFu;            // rank: not a candidate
constexpr uint32_t SHR_MAX_FAULTS = 65534u;       // (so that every rank and every j is < SHR_NONE)
constexpr uint64_t SHR_FNV_BASIS = 0xCBF29CE484222325ull, SHR_FNV_PRIME = 0x100000001B3ull;

struct ShrinkDims {
  uint32_t P, N, depth, dmax;                     // the call's cfg->n_proposers, n_acceptors, depth, delay_max
};
// entries of a rank table (at most 3 + 9 + 2 * 3 * 9 * 4096)
__host__ __device__ inline uint32_t shrink_entries(const ShrinkDims& d) { return 3u + d.N + 2u * d.P * d.N * d.depth; }
// halfwords between the tables of two parents (tables are 8-byte aligned)
__host__ __device__ inline uint64_t shrink_tstride(const ShrinkDims& d) { return ((uint64_t)shrink_entries(d) + 3ull) & ~3ull; }
// the row's proposer count as pxb.script_faults takes it
__host__ __device__ inline uint32_t shrink_row_P(const ShrinkDims& d, const uint8_t* row) { return row[8] ? row[8] : d.P; }

struct ShrinkEntry {
  uint32_t kind;                                  // 0 skew, 1 window, 2 link
  uint32_t dirn, p, a, k;
  uint32_t off;                                   // the entry's byte offset in the row
  uint32_t link;                                  // its link's index in `sent` ((dirn * P + p) * N + a)
};
__host__ __device__ inline ShrinkEntry shrink_entry(const ShrinkDims& d, uint32_t t) {
  ShrinkEntry e{};
  if (t < 3u) {
    e.kind = 0u, e.p = t, e.off = 10u + 2u * t;
  } else if (t < 3u + d.N) {
    e.kind = 1u, e.a = t - 3u, e.off = SCR_HDR + 4u * e.a;
  } else {
    const uint32_t i = t - 3u - d.N;              // (depth > 0: a table of depth 0 has no link entries)
    e.kind = 2u;
    e.k = i % d.depth;
    e.link = i / d.depth;
    e.a = e.link % d.N;
    const uint32_t dp = e.link / d.N;
    e.p = dp % d.P;
    e.dirn = dp / d.P;
    e.off = SCR_HDR + 4u * d.N + i;
  }
  return e;
}
__host__ __device__ __forceinline__ uint32_t shrink_clamp_win(uint32_t c) { return c < 4096u ? c : 4096u; }
__host__ __device__ __forceinline__ bool shrink_link_fault(const ShrinkDims& d, uint32_t b) {
  return (b == 0u) | ((b != SCR_KEEP8) & ((b < d.dmax ? b : d.dmax) > 1u));
}
__host__ __device__ __forceinline__ uint32_t shrink_consumed(const ShrinkDims& d, const uint16_t* sent, uint32_t link) {
  const uint32_t s = sent[link];
  return s < d.depth ? s : d.depth;
}

// pxb.script_faults, one entry: is entry t of `row` a fault, given the send
// counts of the row's run (2 P N halfwords) and Pi = shrink_row_P
__host__ __device__ inline bool shrink_is_fault(const ShrinkDims& d, const uint8_t* row, uint32_t Pi,
                                                const uint16_t* sent, uint32_t t) {
  const ShrinkEntry e = shrink_entry(d, t);
  if (e.kind == 0u) {
    const uint32_t v = script_ld16(row, e.off);
    return (e.p < Pi) & (v != 0u) & (v != SCR_KEEP16);
  }
  if (e.kind == 1u) return shrink_clamp_win(script_ld16(row, e.off)) < shrink_clamp_win(script_ld16(row, e.off + 2u));
  return (e.p < Pi) & (e.k < shrink_consumed(d, sent, e.link)) & shrink_link_fault(d, row[e.off]);
}

// An accepted row, one entry: neutralises entry t when `neutral` (pxb.
// script_neutralise), settles it against the accepted run's `sent` (a link
// entry with k >= sent becomes 1, absent proposers' included; any other that is
// neither 0 nor 0xFF is clamped to delay_max), stores what changed, and answers
// whether the entry is a fault of the new row.  An entry is touched by its own
// call alone, so the calls of a row may run in any order or side by side.
__host__ __device__ inline bool shrink_accept_entry(const ShrinkDims& d, uint8_t* row, uint32_t Pi,
                                                    const uint16_t* sent, uint32_t t, bool neutral) {
  const ShrinkEntry e = shrink_entry(d, t);
  if (e.kind == 0u) {
    if (neutral) row[e.off] = 0u, row[e.off + 1u] = 0u;
    const uint32_t v = neutral ? 0u : script_ld16(row, e.off);
    return (e.p < Pi) & (v != 0u) & (v != SCR_KEEP16);
  }
  if (e.kind == 1u) {
    if (neutral) {
      row[e.off] = row[e.off + 1u] = row[e.off + 2u] = row[e.off + 3u] = 0u;
      return false;
    }
    return shrink_clamp_win(script_ld16(row, e.off)) < shrink_clamp_win(script_ld16(row, e.off + 2u));
  }
  const uint32_t b = row[e.off];
  uint32_t nb = neutral ? 1u : b;
  if (e.k >= (uint32_t)sent[e.link]) nb = 1u;
  if ((nb != 0u) & (nb != SCR_KEEP8)) nb = nb < d.dmax ? nb : d.dmax;
  if (nb != b) row[e.off] = (uint8_t)nb;
  return (e.p < Pi) & (e.k < shrink_consumed(d, sent, e.link)) & shrink_link_fault(d, nb);
}

// the 8 signature bytes of fault t, little-endian in a uint64:
//   skew (0, 0, p, 0, skew u16, 0 u16), window (1, 0, 0, a, c0 u16, c1 u16; as
//   clamped), link (2, dirn, p, a, k u16, byte u16)
__host__ __device__ inline uint64_t shrink_fault_record(const ShrinkDims& d, const uint8_t* row, uint32_t t) {
  const ShrinkEntry e = shrink_entry(d, t);
  uint64_t v0, v1 = 0u;
  if (e.kind == 0u) {
    v0 = script_ld16(row, e.off);
  } else if (e.kind == 1u) {
    v0 = shrink_clamp_win(script_ld16(row, e.off));
    v1 = shrink_clamp_win(script_ld16(row, e.off + 2u));
  } else {
    v0 = e.k;
    v1 = row[e.off];
  }
  return (uint64_t)e.kind | ((uint64_t)e.dirn << 8) | ((uint64_t)e.p << 16) | ((uint64_t)e.a << 24) | (v0 << 32) |
         (v1 << 48);
}
__host__ __device__ __forceinline__ uint64_t shrink_fnv_byte(uint64_t h, uint32_t b) { return (h ^ b) * SHR_FNV_PRIME; }
__host__ __device__ inline uint64_t shrink_fnv_record(uint64_t h, uint64_t rec) {
  for (uint32_t i = 0; i < 8u; ++i) h = shrink_fnv_byte(h, (uint32_t)(rec >> (8u * i)) & 0xFFu);
  return h;
}
// the signature of a row with no faults folded in yet
__host__ __device__ inline uint64_t shrink_fnv_begin(const uint8_t* row) { return shrink_fnv_byte(SHR_FNV_BASIS, row[8]); }

// ---- the candidate's lane ----
// ScriptDraws over (row, rank table, j): a link byte whose rank selects it
// reads as 1.  The byte and the rank come from the same index, two loads that
// do not wait for each other; a neutralised entry resolves as the override 1,
// never as a Philox draw.  Base: ScriptDraws, or a draw source on top of it
// (shrink_cover_core.h: the tapped one).
template <class Base>
struct ShrinkDrawsOver : Base {
  const uint16_t* r_links;            // the table's link part, [dirn][p][a][k]
  uint32_t r_j;                       // the candidate's index among its parent's
  bool r_prefix;                      // ranks <= j (else == j)

  __host__ __device__ __forceinline__ bool selects(uint32_t rank) const {
    return r_prefix ? rank <= r_j : rank == r_j;  // (j < SHR_NONE: SHR_NONE is never selected)
  }
  struct RankedByte {
    const ShrinkDrawsOver& d;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
      const uint32_t b = d.s_links[i], r = d.r_links[i];
      return d.selects(r) ? 1u : b;
    }
  };
  __host__ __device__ __forceinline__ uint4 source_draw(uint32_t lo, uint32_t hi, uint32_t c2, uint32_t c3,
                                                        const uint32_t (&rk)[20]) const {
    return this->source_draw_over(lo, hi, c2, c3, rk, RankedByte{*this});
  }
};
typedef ShrinkDrawsOver<ScriptDraws> ShrinkDraws;

// script_begin for candidate j of the parent (row, table): the same rule for the
// three skews and the N windows.  Draws: the lane's ShrinkDrawsOver.
template <class Draws, class Lane>
__host__ __device__ __forceinline__ uint32_t shrink_begin_over(Lane& L, const EvParams& kp, uint32_t depth,
                                                               const uint8_t* row, const uint16_t* table, uint32_t j,
                                                               bool prefix) {
  Draws& D = L;
  D.r_links = table + 3u + Lane::S::N;
  D.r_j = j;
  D.r_prefix = prefix;
  struct Sel {
    const Draws& d;
    const uint16_t* t;
    __host__ __device__ __forceinline__ bool operator()(uint32_t i) const { return d.selects(t[i]); }
  };
  return script_begin_sel(L, kp, depth, row, Sel{D, table});
}
template <class Lane>
__host__ __device__ __forceinline__ uint32_t shrink_begin(Lane& L, const EvParams& kp, uint32_t depth,
                                                          const uint8_t* row, const uint16_t* table, uint32_t j,
                                                          bool prefix) {
  return shrink_begin_over<ShrinkDraws>(L, kp, depth, row, table, j, prefix);
}

// the predicate of an ended candidate: status, the result's flags word, and its
// send counts (script_sent's 2 P N halfwords)
__host__ __device__ inline bool shrink_holds(uint32_t status, uint32_t flags, const uint16_t* sent, uint32_t n_links,
                                             uint32_t depth, uint32_t flag_mask) {
  uint32_t mx = 0u;
  for (uint32_t i = 0; i < n_links; ++i) mx = sent[i] > mx ? sent[i] : mx;
  return (status == PXB_TRACE_OK) & ((flags & 0xFFu & flag_mask) != 0u) & (mx <= depth);
}

// ---- the lane job (paxos_trace_core.h) of the candidate kernel: job c is candidate c of the launch ----
struct ShrParams {
  EvParams p;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  const uint16_t* table;            // their rank tables
  uint64_t tstride;                 // (halfwords)
  const uint64_t* offsets;          // count + 1: the first candidate of each parent
  uint64_t count;                   // parents
  uint64_t total;                   // candidates of this launch (offsets[count])
  uint32_t depth, flag_mask;
  uint32_t prefix;                  // ranks <= j (else == j)
  uint8_t* held;                    // total
  uint16_t* csent;                  // total * 2 P N (nullable)
  uint4* cres;                      // total (nullable)

  // Starts the lane as candidate c (< total) of the launch: its status as
  // shrink_begin gives it (PXB_SCRIPT_BAD: a malformed row, the lane not started)
  template <class Draws, class Lane>
  __host__ __device__ __forceinline__ uint32_t start(Lane& L, uint64_t c) const {
    // the parent: the last i with offsets[i] <= c (offsets[0] = 0, offsets[count] = total > c)
    uint64_t lo = 0u, hi = count;
    while (hi - lo > 1u) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (offsets[mid] <= c) lo = mid;
      else hi = mid;
    }
    const uint32_t j = (uint32_t)(c - offsets[lo]);
    return shrink_begin_over<Draws>(L, p, depth, rows + lo * stride, table + lo * tstride, j, prefix != 0u);
  }

  template <class Lane, class Trace>
  __host__ __device__ __forceinline__ bool begin(Lane& L, Trace& T, uint64_t c) const {
    T.begin_count(1u, 0u);          // (an empty window: no records are counted)
    bool run = c < total;
    if (run) {
      const uint32_t st = start<ShrinkDraws>(L, c);
      if (st != PXB_TRACE_OK) {     // a malformed row: not run
        T.status = st;
        run = false;
      }
    }
    return run;
  }
};

}  // namespace ev
}  // namespace pxb
