// explore_reach.h — the reach records of a covering exploration
// (include/paxos_batch.h, docs/SEMANTICS.md §15, §17): what pxb_explore_cover
// (paxos_explore_cover.hip) and pxb_explore_win (paxos_explore_win.hip) share on
// the device, over a space policy X (explore_core.h: ExploreLinkX;
// explore_win_core.h: ExploreWinX).
//   ReachParams<X>   the candidate kernels' parameters;
//   reach_reduce<X>  behind a candidate kernel's flag byte the wave reduces into
//                    the parents' records: 64 consecutive candidates can
//                    straddle parents and cells, so it walks its distinct
//                    (parent, cell) keys as the minimal kernel does, and per key
//                    the 29 classes as the cover kernel does: one ballot, and
//                    where a lane has the class one atomic add to the cell's
//                    count and one atomic minimum to its first with the cw of
//                    the lowest such lane (within one parent cw ascends with the
//                    lane).  Integer adds and minima only: the records do not
//                    depend on the order the waves end in;
//   reach_init_kernel, reach_finish_kernel, ReachHooks<X>
//                    the records set in front of the candidates and union_mask
//                    behind them, as explore_device's hooks (explore_driver.h).
// The candidate kernels themselves stay spelled out in the two .hip files: in
// one template over X, or with the flag byte and the key behind shared members,
// the same text compiled to other register and instruction counts in up to 93
// of the 144 shapes.  No block waits for another; plain vector
// stores only.  Device code: included by the two families' units only (the
// kernels here are templates: a unit holds what it instantiates).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/paxos_batch.h"
#include "explore_cover_core.h"

namespace pxb {
namespace ev {

template <class X>
struct ReachParams {
  EvParams p;
  typename X::Space x;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  uint64_t total;                   // candidates of this call (count * X::total <= 2^32)
  uint32_t depth, site_depth, flag_mask;
  pxb_cover_query q;
  uint8_t* bytes;                   // total flag bytes
  typename X::Reach* reach;         // count records, initialised (nullable)
};

// lane `lane` of a wave: its mask m (0: nothing to count), its key parent *
// X::CELLS + cell and its cw
template <class X>
__device__ __forceinline__ void reach_reduce(typename X::Reach* reach, uint32_t lane, uint32_t m, uint32_t key,
                                             uint32_t cw) {
  unsigned long long act = __ballot(m != 0u);
  while (act != 0ull) {             // (wave-uniform) one distinct (parent, cell) a turn
    const int lead = __ffsll(act) - 1;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const bool same = (m != 0u) & (key == k0);
    typename X::Reach* const o = reach + k0 / X::CELLS;
    uint32_t* const cnt = X::count(o, k0 % X::CELLS);
    uint32_t* const fst = X::first(o, k0 % X::CELLS);
#pragma unroll 1
    for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b) {
      const unsigned long long bal = __ballot(same & (((m >> b) & 1u) != 0u));
      if (bal == 0ull) continue;    // (wave-uniform: no candidate of the key has the class)
      // (within one parent cw ascends with the lane: the lowest such lane has the least)
      const uint32_t cmin = (uint32_t)__builtin_amdgcn_readlane((int)cw, __ffsll(bal) - 1);
      if ((int)lane == lead) {
        atomicAdd(cnt + b, (uint32_t)__popcll(bal));
        atomicMin(fst + b, cmin);
      }
    }
    act &= ~__ballot(same);
  }
}

// ---- the records: CW count words | FW first words | parent_mask | union_mask ----
// one thread per word of the records: counts 0, firsts all-ones, masks 0
template <uint32_t CW, uint32_t FW>
__global__ __launch_bounds__(256) void reach_init_kernel(uint32_t* words, uint64_t n_words) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_words) return;
  const uint32_t w = (uint32_t)(t % (CW + FW + 2u));
  words[t] = (w >= CW && w < CW + FW) ? 0xFFFFFFFFu : 0u;
}

// behind the candidate kernel, 32 threads a parent, thread b: the union of the
// counted classes (a first is all-ones where nothing was counted: only a count
// comes with a minimum)
template <uint32_t CW, uint32_t FW>
__global__ __launch_bounds__(32) void reach_finish_kernel(uint32_t* words) {
  uint32_t* const o = words + (uint64_t)blockIdx.x * (CW + FW + 2u);
  const uint32_t b = threadIdx.x;
  uint32_t any = 0u;
#pragma unroll
  for (uint32_t cell = 0; cell < CW / 32u; ++cell) any |= o[cell * 32u + b];
  const unsigned long long bal = __ballot(any != 0u);
  if (b == 0u) o[CW + FW + 1u] = (uint32_t)bal;
}

// explore_device's hooks over the `count` records at d_reach (nullable: none)
template <class X>
struct ReachHooks {
  typename X::Reach* d_reach;
  uint64_t count;
  bool aligned() const { return ((uintptr_t)d_reach & 7u) == 0u; }
  hipError_t before(hipStream_t st) const {
    if (!d_reach) return hipSuccess;
    const uint64_t n_words = count * (X::COUNT_WORDS + X::FIRST_WORDS + 2u);
    hipLaunchKernelGGL((reach_init_kernel<X::COUNT_WORDS, X::FIRST_WORDS>), dim3((unsigned)((n_words + 255u) / 256u)),
                       dim3(256), 0, st, reinterpret_cast<uint32_t*>(d_reach), n_words);
    return hipGetLastError();
  }
  hipError_t after(hipStream_t st) const {
    if (!d_reach) return hipSuccess;
    hipLaunchKernelGGL((reach_finish_kernel<X::COUNT_WORDS, X::FIRST_WORDS>), dim3((unsigned)count), dim3(32), 0, st,
                       reinterpret_cast<uint32_t*>(d_reach));
    return hipGetLastError();
  }
};

}  // namespace ev
}  // namespace pxb
