// explore_core.h — bounded exhaustive exploration (include/paxos_batch.h,
// docs/SEMANTICS.md §12): what the explore kernels (paxos_explore.hip) and the
// host unit test (tests/native/explore_host.cpp) share, as plain C++ over
// script_core.h.
//
// A PARENT is one script row.  Its SITES are the first site_depth entries of
// every link: site s is byte (s / site_depth) * depth + s % site_depth of the
// link table, S = 2 P N site_depth of them.  A CANDIDATE changes at most R
// (<= 3) sites: candidate c of a parent is a radius r, a combination of r
// sites s_1 < .. < s_r and one digit (< A = delay_max) per site, ordered by
// radius, then by the combination's rank in the combinatorial number system
// (m = sum C(s_i, i)), then by the digits (site s_1's the least significant).
// Digit j of a site whose parent byte is b reads as (min(b, A) + 1 + j) mod
// (A + 1): every value in 0..A but the parent's own.  Candidate 0 is the parent.
// A site whose parent byte is 0xFF (keep) has no alternatives: a candidate that
// changes one is skipped.
//
// Here: the space's sizes, unrank and rank, the byte accessor a candidate's lane
// reads its parent's row through (no candidate row exists anywhere), the
// keep-site and bad-parent tests, the lane's draw source and start, the
// minimality test over the candidates' flag bytes, and the space's policy for
// the shared driver (ExploreLinkX).
#pragma once
#include <stdint.h>

#include "script_core.h"
#include "shrink_core.h"

namespace pxb {
namespace ev {

constexpr uint32_t EXP_MAX_RADIUS = 3u;
constexpr uint64_t EXP_MAX_TOTAL = 1ull << 30;
constexpr uint32_t EXP_NO_SITE = 0xFFFFFFFFu;
// a candidate's flag byte
constexpr uint32_t EXP_RAN = 1u, EXP_HELD = 2u, EXP_MINIMAL = 4u;

// C(s, i) for i <= 3 (s < 2^18: below 2^52)
__host__ __device__ __forceinline__ uint64_t explore_choose(uint64_t s, uint32_t i) {
  if (i == 0u) return 1ull;
  if (i == 1u) return s;
  if (i == 2u) return s < 2ull ? 0ull : s * (s - 1ull) / 2ull;
  return s < 3ull ? 0ull : s * (s - 1ull) * (s - 2ull) / 6ull;
}

struct ExploreSpace {
  uint32_t S, A, R;                 // sites, alternatives per site, radius
  uint32_t apow[4];                 // A^r
  uint64_t base[5];                 // base[r]: the first candidate of radius r; base[R + 1 ..] = T
  uint64_t T;                       // candidates per parent (0: no valid space)
};
// the space of S sites with A alternatives each within radius R; T = 0 when a
// parameter is out of range or T would exceed 2^30
__host__ __device__ inline ExploreSpace explore_space(uint64_t S, uint32_t A, uint32_t R) {
  ExploreSpace e{};
  if (S == 0ull || S > 2ull * 3ull * 9ull * 4096ull || A == 0u || A > 15u || R > EXP_MAX_RADIUS) return e;
  e.S = (uint32_t)S, e.A = A, e.R = R;
  e.apow[0] = 1u;
  for (uint32_t r = 1; r < 4u; ++r) e.apow[r] = e.apow[r - 1u] * A;
  uint64_t t = 0ull;
  for (uint32_t r = 0; r <= 4u; ++r) {
    e.base[r] = t;
    if (r > R) continue;
    const uint64_t cmb = explore_choose(S, r);   // (C <= 2^30 before the product: no overflow)
    if (cmb > EXP_MAX_TOTAL || (t += cmb * e.apow[r]) > EXP_MAX_TOTAL) return ExploreSpace{};
  }
  e.T = t;
  return e;
}
// the sites of a call: 0 for a shape the scripted lane does not have
__host__ __device__ inline uint64_t explore_sites(uint32_t P, uint32_t N, uint32_t site_depth) {
  if (P < 1u || P > 3u || N < 1u || N > 9u || site_depth < 1u || site_depth > PXB_SCRIPT_MAX_DEPTH) return 0ull;
  return 2ull * P * N * site_depth;
}

struct ExploreCand {
  uint32_t r;                       // changed sites
  uint32_t site[3], digit[3];       // site[0] < site[1] < site[2] (the first r)
};
// (the space is a kernel argument and a candidate lives in registers: every
// index below is a compile-time one after unrolling, selects otherwise, so that
// neither is copied to scratch memory)
__host__ __device__ __forceinline__ uint64_t explore_base(const ExploreSpace& e, uint32_t r) {
  return r == 0u ? e.base[0] : r == 1u ? e.base[1] : r == 2u ? e.base[2] : e.base[3];
}
__host__ __device__ __forceinline__ uint32_t explore_apow(const ExploreSpace& e, uint32_t r) {
  return r == 0u ? 1u : r == 1u ? e.apow[1] : r == 2u ? e.apow[2] : e.apow[3];
}
// the radius of candidate c (< T): base_r <= c < base_(r+1) (base_q = T above the space's radius)
__host__ __device__ __forceinline__ uint32_t explore_radius(const ExploreSpace& e, uint64_t c) {
  return (c >= e.base[1] ? 1u : 0u) + (c >= e.base[2] ? 1u : 0u) + (c >= e.base[3] ? 1u : 0u);
}
// candidate c (< T) of the space
__host__ __device__ __forceinline__ ExploreCand explore_unrank(const ExploreSpace& e, uint64_t c) {
  ExploreCand k{};
  const uint32_t r = explore_radius(e, c), ap = explore_apow(e, r);
  k.r = r;
  const uint32_t x = (uint32_t)(c - explore_base(e, r));
  uint64_t m = x / ap;
  uint32_t v = x % ap;
  uint32_t hi = e.S;                // s_i < hi
#pragma unroll
  for (uint32_t i = 3u; i >= 1u; --i) {
    if (i > r) continue;
    // the largest s in [i - 1, hi) with C(s, i) <= m (C(i - 1, i) = 0)
    uint32_t lo = i - 1u, up = hi;
    while (up - lo > 1u) {
      const uint32_t mid = lo + ((up - lo) >> 1);
      if (explore_choose(mid, i) <= m) lo = mid;
      else up = mid;
    }
    k.site[i - 1u] = lo;
    m -= explore_choose(lo, i);
    hi = lo;
  }
#pragma unroll
  for (uint32_t i = 0; i < 3u; ++i) {
    if (i >= r) continue;
    k.digit[i] = v % e.A;
    v /= e.A;
  }
  return k;
}
// the candidate of the sites of `k` picked by `subset` (bit i: site[i], with its digit)
__host__ __device__ __forceinline__ uint64_t explore_rank_subset(const ExploreSpace& e, const ExploreCand& k, uint32_t subset) {
  uint64_t m = 0ull;
  uint32_t v = 0u, n = 0u;
#pragma unroll
  for (uint32_t i = 0; i < 3u; ++i)
    if ((i < k.r) & ((subset >> i) & 1u)) {
      m += explore_choose(k.site[i], n + 1u);
      v += k.digit[i] * explore_apow(e, n);
      ++n;
    }
  return explore_base(e, n) + m * explore_apow(e, n) + v;
}
__host__ __device__ __forceinline__ uint64_t explore_rank(const ExploreSpace& e, const ExploreCand& k) {
  return explore_rank_subset(e, k, (1u << k.r) - 1u);
}

// digit j of a site whose parent byte is b (!= 0xFF)
__host__ __device__ __forceinline__ uint32_t explore_alt(uint32_t b, uint32_t j, uint32_t A) {
  const uint32_t t = (b < A ? b : A) + 1u + j;
  return t > A ? t - (A + 1u) : t;
}
// the link-table index of site s
__host__ __device__ __forceinline__ uint32_t explore_site_index(uint32_t s, uint32_t site_depth, uint32_t depth) {
  return (s / site_depth) * depth + s % site_depth;
}

// The byte accessor of a candidate's lane: the parent's link byte, rewritten
// when its index is one of the at most three changed ones.  No table, no load
// beside the byte's own.
struct ExploreByte {
  const uint8_t* links;             // the parent's link table
  uint32_t idx[3], dig[3];          // (EXP_NO_SITE: unused)
  uint32_t A;
  __host__ __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    const uint32_t b = links[i], j = (uint32_t)i;
    const bool h0 = j == idx[0], h1 = j == idx[1], h2 = j == idx[2];
    // (the sites differ, so at most one hits; no select between the digits' addresses, which
    // would keep the whole lane in scratch memory)
    const uint32_t d = (h0 ? dig[0] : 0u) | (h1 ? dig[1] : 0u) | (h2 ? dig[2] : 0u);
    return (h0 | h1 | h2) ? explore_alt(b, d, A) : b;
  }
};
__host__ __device__ __forceinline__ ExploreByte explore_byte(const ExploreSpace& e, const ExploreCand& k, const uint8_t* row,
                                                    uint32_t N, uint32_t site_depth, uint32_t depth) {
  ExploreByte x;
  x.links = row + script_links_off(N);
  x.A = e.A;
#pragma unroll
  for (uint32_t i = 0; i < 3u; ++i) {
    x.idx[i] = i < k.r ? explore_site_index(k.site[i], site_depth, depth) : EXP_NO_SITE;
    x.dig[i] = i < k.r ? k.digit[i] : 0u;
  }
  return x;
}
// does the candidate change a keep site of its parent (then it is skipped)
__host__ __device__ __forceinline__ bool explore_changes_keep(const ExploreByte& x) {
  bool keep = false;
#pragma unroll
  for (uint32_t i = 0; i < 3u; ++i)
    if (x.idx[i] != EXP_NO_SITE) keep |= x.links[x.idx[i]] == SCR_KEEP8;
  return keep;
}
// script_begin's test of a malformed row (P: the call's)
__host__ __device__ __forceinline__ bool explore_parent_bad(const uint8_t* row, uint32_t P) {
  return (row[8] > P) | (row[9] != 0u);
}

// ---- the candidate's lane ----
// ScriptDraws whose link bytes go through ExploreByte
struct ExploreDraws : ScriptDraws {
  ExploreByte x_byte;
  __host__ __device__ __forceinline__ uint4 source_draw(uint32_t lo, uint32_t hi, uint32_t c2, uint32_t c3,
                                                        const uint32_t (&rk)[20]) const {
    return source_draw_over(lo, hi, c2, c3, rk, x_byte);
  }
};
// script_begin for the candidate `x` of the parent `row`
template <class Lane>
__host__ __device__ __forceinline__ uint32_t explore_begin(Lane& L, const EvParams& kp, uint32_t depth,
                                                           const uint8_t* row, const ExploreByte& x) {
  ExploreDraws& D = L;
  D.x_byte = x;
  return script_begin(L, kp, depth, row);
}
// the flag byte of an ended candidate: EXP_RAN (status OK, no link past depth) and EXP_HELD (the shrinker's predicate)
__host__ __device__ __forceinline__ uint32_t explore_flags(uint32_t status, uint32_t flags, const uint16_t* sent,
                                                  uint32_t n_links, uint32_t depth, uint32_t flag_mask) {
  uint32_t mx = 0u;
  for (uint32_t i = 0; i < n_links; ++i) mx = sent[i] > mx ? sent[i] : mx;
  const bool ran = (status == PXB_TRACE_OK) & (mx <= depth);
  const bool held = shrink_holds(status, flags, sent, n_links, depth, flag_mask);
  return (ran ? EXP_RAN : 0u) | (held ? EXP_HELD : 0u);
}

// Is the held candidate `k` minimal: no candidate of a proper subset of its
// changes (same digits; the empty one, candidate 0, included) holds.  `bytes`:
// the T flag bytes of its parent.
__host__ __device__ __forceinline__ bool explore_is_minimal(const ExploreSpace& e, const ExploreCand& k, const uint8_t* bytes) {
  const uint32_t full = (1u << k.r) - 1u;
  bool any = false;
  for (uint32_t sub = 0u; sub < full; ++sub) any |= (bytes[explore_rank_subset(e, k, sub)] & EXP_HELD) != 0u;
  return !any;
}

// ---- the space policy of the link space ----
// What explore_driver.h, the reach reduction (explore_reach.h) and the host
// programs (tests/native/explore_host.h) ask of a space: candidate g (< 2^32)
// of a call is candidate cw (< total) of parent i, which is a window choice h
// with a link candidate c; it lies in one of CELLS cells, and is counted in a
// reach record per cell.  Here h = 0 always; explore_win_core.h's ExploreWinX
// is the joint space's.
struct ExploreSplit {
  uint32_t i, cw, h, c;
};
struct ExploreLinkX {
  typedef ExploreSpace Space;
  typedef pxb_explore_reach Reach;
  static constexpr uint32_t CELLS = 4u;                            // radii
  static constexpr uint32_t COUNT_WORDS = CELLS * 32u, FIRST_WORDS = 32u;   // of Reach, in front of its two masks
  static constexpr uint32_t FLAGS = PXB_EXPLORE_MINIMAL;           // what the space struct's flags may hold
  __host__ __device__ static __forceinline__ uint64_t total(const Space& e) { return e.T; }
  __host__ __device__ static __forceinline__ const ExploreSpace& links(const Space& e) { return e; }
  __host__ __device__ static __forceinline__ ExploreSplit split(const Space& e, uint32_t g) {
    const uint32_t tt = (uint32_t)e.T, i = g / tt, c = g - i * tt;
    return ExploreSplit{i, c, 0u, c};
  }
  __host__ __device__ static __forceinline__ uint32_t cell(const Space& e, uint32_t, uint32_t c) {
    return explore_radius(e, c);
  }
  // (`bytes`: the parent's `total` flag bytes)
  __host__ __device__ static __forceinline__ bool is_minimal(const Space& e, uint32_t, uint32_t c, const uint8_t* bytes) {
    return explore_is_minimal(e, explore_unrank(e, c), bytes);
  }
  __host__ __device__ static __forceinline__ uint32_t* count(Reach* o, uint32_t cell) {
    return &o->count[0][0] + cell * 32u;
  }
  __host__ __device__ static __forceinline__ uint32_t* first(Reach* o, uint32_t) { return &o->first[0]; }
  // behind the begin: nothing
  template <class Lane>
  __host__ __device__ static __forceinline__ void apply(Lane&, const Space&, uint32_t) {}
};
static_assert(sizeof(pxb_explore_reach) == (ExploreLinkX::COUNT_WORDS + ExploreLinkX::FIRST_WORDS + 2u) * 4u, "Reach words");

}  // namespace ev
}  // namespace pxb
