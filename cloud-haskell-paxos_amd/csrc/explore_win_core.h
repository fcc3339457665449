// explore_win_core.h — isolation windows as sites of the exploration
// (include/paxos_batch.h: pxb_explore_win, docs/SEMANTICS.md §17): what the
// kernels (paxos_explore_win.hip) and the host unit test
// (tests/native/explore_win_host.cpp) share, as plain C++ over
// explore_cover_core.h (the link space of §12 with the predicate of §15).
//
// A WINDOW CHOICE h of a parent replaces the isolation window of at most
// win_radius (<= 2) acceptors.  An acceptor has W = win_starts * L alternatives,
// L = win_lens + (open ? 1 : 0): digit d is start i = d / L and length index
// j = d % L, the window [c0, c1) with c0 = win_first + i and c1 = c0 + 1 + j
// (j < win_lens) or 4096 (the open one).  Choices are ordered as §12 orders link
// candidates over N sites with W alternatives: by radius, by the acceptor
// combination's rank (a_1 < a_2: m = C(a_1, 1) + C(a_2, 2)), then by the digits
// (a_1's the least significant); choice 0 leaves the parent's windows alone.
// A CANDIDATE c' = h T + c pairs a choice with a §12 link candidate c (< T);
// T_w = H T of them per parent.
//
// Here: the window space's sizes, unrank and rank, the window word a digit
// stands for, the overwrite of a started lane's windows, the two-axis
// minimality test over the candidates' flag bytes, and the joint space's policy
// for the shared driver (ExploreWinX).
#pragma once
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "explore_cover_core.h"

namespace pxb {
namespace ev {

static_assert(sizeof(pxb_explore_win_space) == 48, "pxb_explore_win_space: 48 bytes");
static_assert(sizeof(pxb_explore_win_reach) == 2 * 3 * 4 * 32 * 4 + 8, "pxb_explore_win_reach: 3,080 bytes");

constexpr uint32_t EXW_MAX_RADIUS = 2u;
constexpr uint32_t EXW_CELLS = 12u;               // (r_w, r_l) pairs: 3 x 4

struct WinSpace {
  uint32_t N, L, nlen, first, R;    // acceptors, lengths per start (the open one included), win_lens, win_first, win_radius
  // (32-bit, so that a lane's unrank is 32-bit divisions: H <= 2^30, W < 2^25,
  // and W^2 <= 2^30 wherever two windows change)
  uint32_t W, W2;                   // alternatives per acceptor; W^2 (0 below radius 2)
  uint32_t base[4];                 // base[r]: the first choice of radius r; base[R + 1 ..] = H
  uint32_t H;                       // choices per parent (0: no valid space)
};
// the window space of N acceptors; H = 0 when a field is out of range or H
// would exceed 2^30
__host__ __device__ inline WinSpace explore_win_space(uint32_t N, uint32_t win_radius, uint32_t win_first,
                                                      uint32_t win_starts, uint32_t win_lens, bool open) {
  WinSpace w{};
  if (N < 1u || N > 9u || win_radius > EXW_MAX_RADIUS || win_starts == 0u) return w;
  if (win_first > 4096u || win_starts > 4096u || win_lens > 4096u) return w;
  if (win_first + win_starts - 1u + win_lens > 4096u) return w;
  const uint32_t L = win_lens + (open ? 1u : 0u);
  if (L == 0u) return w;
  w.N = N, w.L = L, w.nlen = win_lens, w.first = win_first, w.R = win_radius;
  w.W = win_starts * L;             // (<= 2^12 * (2^12 + 1))
  uint64_t t = 0ull, wp = 1ull;
  for (uint32_t r = 0; r < 4u; ++r) {
    w.base[r] = (uint32_t)t;
    if (r > win_radius) continue;
    // (C(9, 2) W^2 < 2^54: no overflow before the test)
    if ((t += explore_choose(N, r) * wp) > EXP_MAX_TOTAL) return WinSpace{};
    wp *= w.W;
  }
  w.W2 = win_radius >= 2u ? w.W * w.W : 0u;
  w.H = (uint32_t)t;
  return w;
}

struct WinCand {
  uint32_t r;                       // changed acceptors
  uint32_t acc[2], digit[2];        // acc[0] < acc[1] (the first r)
};
__host__ __device__ __forceinline__ uint32_t explore_win_radius(const WinSpace& w, uint32_t h) {
  return (h >= w.base[1] ? 1u : 0u) + (h >= w.base[2] ? 1u : 0u);
}
__host__ __device__ __forceinline__ uint32_t explore_win_base(const WinSpace& w, uint32_t r) {
  return r == 0u ? w.base[0] : r == 1u ? w.base[1] : w.base[2];
}
// choice h (< H) of the space
__host__ __device__ __forceinline__ WinCand explore_win_unrank(const WinSpace& w, uint32_t h) {
  WinCand k{};
  const uint32_t r = explore_win_radius(w, h);
  k.r = r;
  const uint32_t x = h - explore_win_base(w, r);
  if (r == 1u) {
    k.acc[0] = x / w.W;
    k.digit[0] = x % w.W;
  } else if (r == 2u) {
    const uint32_t m = x / w.W2;                  // C(a_1, 1) + C(a_2, 2) < C(9, 2)
    const uint32_t v = x % w.W2;
    uint32_t a2 = 1u;                             // the largest s with C(s, 2) <= m
#pragma unroll
    for (uint32_t s = 2u; s < 9u; ++s) a2 = (s * (s - 1u) / 2u <= m) ? s : a2;
    k.acc[1] = a2;
    k.acc[0] = m - a2 * (a2 - 1u) / 2u;
    k.digit[0] = v % w.W;
    k.digit[1] = v / w.W;
  }
  return k;
}
// the choice of the acceptors of `k` picked by `subset` (bit i: acc[i], with its digit)
__host__ __device__ __forceinline__ uint32_t explore_win_rank_subset(const WinSpace& w, const WinCand& k, uint32_t subset) {
  const bool p0 = (k.r > 0u) & ((subset & 1u) != 0u), p1 = (k.r > 1u) & ((subset & 2u) != 0u);
  if (p0 & p1)
    return w.base[2] + (k.acc[0] + k.acc[1] * (k.acc[1] - 1u) / 2u) * w.W2 + k.digit[0] + k.digit[1] * w.W;
  if (p0 | p1) return w.base[1] + (p0 ? k.acc[0] : k.acc[1]) * w.W + (p0 ? k.digit[0] : k.digit[1]);
  return 0u;
}
__host__ __device__ __forceinline__ uint32_t explore_win_rank(const WinSpace& w, const WinCand& k) {
  return explore_win_rank_subset(w, k, (1u << k.r) - 1u);
}

// the window [c0, c1) of digit d
__host__ __device__ __forceinline__ void explore_win_bounds(const WinSpace& w, uint32_t d, uint32_t* c0, uint32_t* c1) {
  const uint32_t i = d / w.L, j = d % w.L;
  *c0 = w.first + i;
  *c1 = j < w.nlen ? *c0 + 1u + j : 4096u;
}
// the same as the lane's window word, c0 | c1 << 16 (0: none, where c0 >= c1)
__host__ __device__ __forceinline__ uint32_t explore_win_word(const WinSpace& w, uint32_t d) {
  uint32_t c0, c1;
  explore_win_bounds(w, d, &c0, &c1);
  return c0 >= c1 ? 0u : c0 | (c1 << 16);
}
// Behind script_begin: the windows of the changed acceptors replace what the
// parent's row gave (explicit, none or keep).  (an unrolled walk over the
// acceptors with selects: no dynamic index into the lane's state)
template <class Lane>
__host__ __device__ __forceinline__ void explore_win_apply(Lane& L, const WinSpace& w, const WinCand& k) {
  constexpr uint32_t N = Lane::S::N;
  const uint32_t v0 = explore_win_word(w, k.digit[0]), v1 = explore_win_word(w, k.digit[1]);
  const bool u0 = k.r > 0u, u1 = k.r > 1u;
#pragma unroll
  for (uint32_t a = 0; a < N; ++a) {
    const bool h0 = u0 & (k.acc[0] == a), h1 = u1 & (k.acc[1] == a);
    // (opaque: the selected word is made here, once; otherwise the select may
    // sink to the acceptor op's read and keep its operands live across the run)
    L.win[a] = Lane::opaque(h0 ? v0 : h1 ? v1 : L.win[a]);
  }
}

// ---- the joint space ----
struct ExploreWin {
  ExploreSpace e;                   // the link part (§12)
  WinSpace w;                       // the window part
  uint64_t Tw;                      // H T (0: no valid space)
};
__host__ __device__ inline ExploreWin explore_win_make(const ExploreSpace& e, const WinSpace& w) {
  ExploreWin x{};
  x.e = e, x.w = w;
  x.Tw = (e.T && w.H && (uint64_t)w.H * e.T <= EXP_MAX_TOTAL) ? (uint64_t)w.H * e.T : 0ull;   // (both <= 2^30)
  return x;
}
// the cell r_w * 4 + r_l of candidate c' = h T + c
__host__ __device__ __forceinline__ uint32_t explore_win_cell(const ExploreWin& x, uint32_t h, uint32_t c) {
  return explore_win_radius(x.w, h) * 4u + explore_radius(x.e, c);
}
// Is the held candidate (kw, kl) minimal: no candidate made of a subset of its
// window changes and a subset of its link changes (same digits; the empty ones
// included), other than itself, holds.  `bytes`: the T_w flag bytes of its parent.
__host__ __device__ __forceinline__ bool explore_win_is_minimal(const ExploreWin& x, const WinCand& kw,
                                                                const ExploreCand& kl, const uint8_t* bytes) {
  const uint32_t fw = (1u << kw.r) - 1u, fl = (1u << kl.r) - 1u;
  bool any = false;
  for (uint32_t sw = 0u; sw <= fw; ++sw) {
    const uint64_t hb = (uint64_t)explore_win_rank_subset(x.w, kw, sw) * x.e.T;
    for (uint32_t sl = 0u; sl <= fl; ++sl) {
      if ((sw == fw) & (sl == fl)) continue;
      any |= (bytes[hb + explore_rank_subset(x.e, kl, sl)] & EXP_HELD) != 0u;
    }
  }
  return !any;
}

// ---- the space policy of the joint space (explore_core.h: ExploreLinkX) ----
// cw = h T + c; the cell is (r_w, r_l); the record holds a first per cell.
struct ExploreWinX {
  typedef ExploreWin Space;
  typedef pxb_explore_win_reach Reach;
  static constexpr uint32_t CELLS = EXW_CELLS;
  static constexpr uint32_t COUNT_WORDS = CELLS * 32u, FIRST_WORDS = CELLS * 32u;
  static constexpr uint32_t FLAGS = PXB_EXPLORE_MINIMAL | PXB_EXPLORE_WIN_OPEN;
  __host__ __device__ static __forceinline__ uint64_t total(const Space& x) { return x.Tw; }
  __host__ __device__ static __forceinline__ const ExploreSpace& links(const Space& x) { return x.e; }
  __host__ __device__ static __forceinline__ ExploreSplit split(const Space& x, uint32_t g) {
    const uint32_t tw = (uint32_t)x.Tw, tt = (uint32_t)x.e.T;
    const uint32_t i = g / tw, cw = g - i * tw, h = cw / tt, c = cw - h * tt;
    return ExploreSplit{i, cw, h, c};
  }
  __host__ __device__ static __forceinline__ uint32_t cell(const Space& x, uint32_t h, uint32_t c) {
    return explore_win_cell(x, h, c);
  }
  __host__ __device__ static __forceinline__ bool is_minimal(const Space& x, uint32_t h, uint32_t c, const uint8_t* bytes) {
    return explore_win_is_minimal(x, explore_win_unrank(x.w, h), explore_unrank(x.e, c), bytes);
  }
  __host__ __device__ static __forceinline__ uint32_t* count(Reach* o, uint32_t cell) {
    return &o->count[0][0][0] + cell * 32u;
  }
  __host__ __device__ static __forceinline__ uint32_t* first(Reach* o, uint32_t cell) {
    return &o->first[0][0][0] + cell * 32u;
  }
  // behind the begin: the windows of choice h
  template <class Lane>
  __host__ __device__ static __forceinline__ void apply(Lane& L, const Space& x, uint32_t h) {
    explore_win_apply(L, x.w, explore_win_unrank(x.w, h));
  }
};
static_assert(sizeof(pxb_explore_win_reach) == (ExploreWinX::COUNT_WORDS + ExploreWinX::FIRST_WORDS + 2u) * 4u, "Reach words");

}  // namespace ev
}  // namespace pxb
