// paxos_query.hip — on-device queries over pxb_result arrays (pxb_query_device).
//
// Ordered stream compaction + histograms in three passes; the kernels below
// never wait for another block (no look-back, no flag to spin on), and the
// scan of the tile counts is hipCUB's DeviceScan, as in the wire codec:
//   1. count_kernel    every wave takes tiles of WTILE results (WLOADS coalesced
//                      16-B loads per lane), counts its matches with 64-bit
//                      ballots and writes one count per tile; the matches also
//                      go into the block's LDS bins (32-bit), flushed to the
//                      64-bit global bins once per block;
//   2. hipCUB          exclusive sum of the tile counts (64-bit offsets), and a
//                      one-thread kernel that reads the caller's cursor as the
//                      list's base and adds the call's total to it;
//   3. scatter_kernel  every wave re-reads its tile -- only if the tile holds
//                      matches that land below `capacity` -- ranks them with
//                      ballot + popcount of the lower lanes and writes ids and
//                      records contiguously from the tile's offset.
// HBM: the results once, plus once more for the tiles that hold matches; 12 B
// of scratch per tile.
//
// Contended bins: real runs put most instances in one bin (BASELINE config 4:
// 84 % at the step cap; config 2: every instance in bin 6), and 64 lanes adding
// to one LDS word serialise.  So a wave first combines: the lanes that share the
// first matching lane's bin are counted with a ballot and added once, twice
// over; what is left (values spread over many bins) goes in one by one.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "host_util.h"

namespace pxq {
using namespace pxb::host;

constexpr int QBLOCK = 512;                      // 8 waves
constexpr int WAVES = QBLOCK / 64;
constexpr int WLOADS = 16;                       // 16-B loads per lane and tile, 8 in flight at a time
constexpr int WTILE = 64 * WLOADS;               // results per tile (one wave)
constexpr int BTILE = WAVES * WTILE;             // results per block and iteration
// A block's LDS bins are 32-bit: no block may see 2^32 results.  The count
// grid is sized so that a block takes at most 2^18 iterations = 2^31 results.
constexpr uint64_t MAX_BLOCK_ITERS = 1ull << 18;
constexpr int SMALL_BINS = 1024;                 // bins per histogram of the small-LDS shape

__device__ __forceinline__ bool matches(const pxb_query& q, const uint4& r) {
  const uint32_t f = r.w & q.flag_mask, steps = PXB_RESULT_STEPS(r.w);
  const bool fl = (q.flag_mode == PXB_Q_ANY) ? (f != 0u) : (q.flag_mode == PXB_Q_ALL) ? (f == q.flag_mask) : (f == 0u);
  return fl & (steps >= q.steps_min) & (steps <= q.steps_max) & (r.z >= q.rounds_min) & (r.z <= q.rounds_max);
}

// bins[bin] += 1 for every lane with m set (whole wave active)
__device__ __forceinline__ void hist_add(uint32_t* bins, uint32_t bin, bool m, int lane) {
  unsigned long long act = __ballot(m);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (act == 0ull) break;                      // (wave-uniform)
    const int lead = __ffsll(act) - 1;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
    const bool same = m & (bin == b0);
    const unsigned long long sm = __ballot(same);
    if (lane == lead) atomicAdd(&bins[b0], (uint32_t)__popcll(sm));
    m = m & !same;
    act &= ~sm;
  }
  if (m) atomicAdd(&bins[bin], 1u);
}

// CAP: LDS bins per histogram (0: no histogram asked for)
template <int CAP>
__global__ __launch_bounds__(QBLOCK) void count_kernel(const uint4* __restrict__ res, uint64_t n, pxb_query q,
                                                       uint64_t iters, uint32_t* __restrict__ tcount,
                                                       unsigned long long* __restrict__ hist_steps,
                                                       unsigned long long* __restrict__ hist_rounds) {
  __shared__ uint32_t s_bins[2][CAP ? CAP : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (CAP) {
    for (uint32_t b = threadIdx.x; b < q.n_bins_steps; b += QBLOCK) s_bins[0][b] = 0u;
    for (uint32_t b = threadIdx.x; b < q.n_bins_rounds; b += QBLOCK) s_bins[1][b] = 0u;
    __syncthreads();
  }
  for (uint64_t it = blockIdx.x; it < iters; it += gridDim.x) {
    const uint64_t tile = it * WAVES + w;
    const uint64_t base = tile * WTILE;
    if (base >= n) continue;                     // (wave-uniform; no barrier inside the loop)
    uint32_t cnt = 0;
    for (int h = 0; h < WLOADS; h += 8) {
      uint4 r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint64_t i = base + (uint64_t)(h + j) * 64 + lane;
        r[j] = (i < n) ? res[i] : uint4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint64_t i = base + (uint64_t)(h + j) * 64 + lane;
        const bool m = (i < n) & matches(q, r[j]);
        cnt += (uint32_t)__popcll(__ballot(m));
        if (CAP) {
          if (q.n_bins_steps) hist_add(s_bins[0], min(PXB_RESULT_STEPS(r[j].w), q.n_bins_steps - 1u), m, lane);
          if (q.n_bins_rounds) hist_add(s_bins[1], min(r[j].z, q.n_bins_rounds - 1u), m, lane);
        }
      }
    }
    if (lane == 0) tcount[tile] = cnt;
  }
  if (CAP) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < q.n_bins_steps; b += QBLOCK)
      if (const uint32_t v = s_bins[0][b]) atomicAdd(&hist_steps[b], (unsigned long long)v);
    for (uint32_t b = threadIdx.x; b < q.n_bins_rounds; b += QBLOCK)
      if (const uint32_t v = s_bins[1][b]) atomicAdd(&hist_rounds[b], (unsigned long long)v);
  }
}

// the list's base for this call = the caller's cursor; cursor += the call's matches
__global__ void cursor_kernel(uint64_t* __restrict__ cursor, const uint32_t* __restrict__ tcount,
                              const uint64_t* __restrict__ toff, uint64_t ntiles, uint64_t* __restrict__ list_base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t b = *cursor;
    *list_base = b;
    *cursor = b + toff[ntiles - 1] + tcount[ntiles - 1];
  }
}

__global__ __launch_bounds__(QBLOCK) void scatter_kernel(const uint4* __restrict__ res, uint64_t n, uint64_t first,
                                                         pxb_query q, const uint32_t* __restrict__ tcount,
                                                         const uint64_t* __restrict__ toff,
                                                         const uint64_t* __restrict__ list_base,
                                                         uint64_t* __restrict__ ids, uint4* __restrict__ matched,
                                                         uint64_t capacity) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile = (uint64_t)blockIdx.x * WAVES + w;
  const uint64_t base = tile * WTILE;
  // (all three wave-uniform) past the end, no match in the tile, or the list is full
  if (base >= n || tcount[tile] == 0u) return;
  uint64_t pos = *list_base + toff[tile];
  if (pos >= capacity) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int h = 0; h < WLOADS; h += 8) {
    uint4 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t i = base + (uint64_t)(h + j) * 64 + lane;
      r[j] = (i < n) ? res[i] : uint4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t i = base + (uint64_t)(h + j) * 64 + lane;
      const bool m = (i < n) & matches(q, r[j]);
      const unsigned long long bal = __ballot(m);
      const uint64_t at = pos + (uint64_t)__popcll(bal & below);
      if (m && at < capacity) {
        ids[at] = first + i;
        if (matched) matched[at] = r[j];
      }
      pos += (uint64_t)__popcll(bal);
    }
    if (pos >= capacity) return;
  }
}

}  // namespace pxq

using namespace pxq;

extern "C" {

// internal (pxb_sweep too): the argument rules of a query, host or device form
int pxb_query_validate(const pxb_query* q, const void* ids, uint64_t capacity, const void* n_matches,
                       const void* hist_steps, const void* hist_rounds) {
  if (!q || !n_matches) return PXB_E_INVAL;
  if (q->flag_mode > PXB_Q_NONE || q->flag_mask > 0xFFu) return PXB_E_INVAL;
  if (q->n_bins_steps > PXB_HIST_MAX_BINS || q->n_bins_rounds > PXB_HIST_MAX_BINS) return PXB_E_INVAL;
  if (capacity && !ids) return PXB_E_INVAL;
  if ((q->n_bins_steps && !hist_steps) || (q->n_bins_rounds && !hist_rounds)) return PXB_E_INVAL;
  return PXB_OK;
}

int pxb_query_device(const pxb_result* d_results, uint64_t first_instance, uint64_t count, const pxb_query* q,
                     uint64_t* d_ids, pxb_result* d_matched, uint64_t capacity, uint64_t* d_n_matches,
                     int64_t* d_hist_steps, int64_t* d_hist_rounds, void* stream) {
  if (int rc = pxb_query_validate(q, d_ids, capacity, d_n_matches, d_hist_steps, d_hist_rounds)) return rc;
  if (count > (1ull << 40) || (count && !d_results)) return PXB_E_INVAL;
  // (the records move as 16-B words)
  if (((uintptr_t)d_results & 15u) || ((uintptr_t)d_matched & 15u) || ((uintptr_t)d_ids & 7u)) return PXB_E_INVAL;
  if (count == 0) return PXB_OK;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev)) return rc;
  if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) return hip_fail(e);
  if (cus < 1) return hip_fail(hipErrorInvalidDevice);

  const uint64_t ntiles = (count + WTILE - 1) / WTILE;
  const uint64_t iters = (count + BTILE - 1) / BTILE;
  widen_iter counts(nullptr, Widen{});
  size_t need = 0;
  if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, counts, (uint64_t*)nullptr, (int64_t)ntiles, st))
    return hip_fail(e);
  const size_t cnt_b = pad256(ntiles * sizeof(uint32_t)), off_b = pad256(ntiles * sizeof(uint64_t));
  void* buf = nullptr;
  if (int rc = pxw::scratch(dev, 256 + cnt_b + off_b + need, st, &buf)) return rc;
  uint64_t* list_base = reinterpret_cast<uint64_t*>(buf);
  uint32_t* tcount = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(buf) + 256);
  uint64_t* toff = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(buf) + 256 + cnt_b);
  void* tmp = reinterpret_cast<char*>(buf) + 256 + cnt_b + off_b;
  counts = widen_iter(tcount, Widen{});

  const uint32_t nb = (q->n_bins_steps > q->n_bins_rounds) ? q->n_bins_steps : q->n_bins_rounds;
  // resident blocks: 4 per CU by waves, 2 with both full histograms in LDS (64 KiB a block)
  const uint64_t resident = (uint64_t)cus * ((nb > SMALL_BINS) ? 2u : 4u);
  uint64_t grid = (iters < resident) ? iters : resident;
  const uint64_t least = (iters + MAX_BLOCK_ITERS - 1) / MAX_BLOCK_ITERS;   // (32-bit LDS bins: see MAX_BLOCK_ITERS)
  if (grid < least) grid = least;
  const uint4* res = reinterpret_cast<const uint4*>(d_results);
  unsigned long long* hs = reinterpret_cast<unsigned long long*>(d_hist_steps);
  unsigned long long* hr = reinterpret_cast<unsigned long long*>(d_hist_rounds);
  if (nb == 0)
    hipLaunchKernelGGL(count_kernel<0>, dim3((unsigned)grid), dim3(QBLOCK), 0, st, res, count, *q, iters, tcount, hs, hr);
  else if (nb <= SMALL_BINS)
    hipLaunchKernelGGL(count_kernel<SMALL_BINS>, dim3((unsigned)grid), dim3(QBLOCK), 0, st, res, count, *q, iters,
                       tcount, hs, hr);
  else
    hipLaunchKernelGGL(count_kernel<PXB_HIST_MAX_BINS>, dim3((unsigned)grid), dim3(QBLOCK), 0, st, res, count, *q,
                       iters, tcount, hs, hr);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, need, counts, toff, (int64_t)ntiles, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(cursor_kernel, dim3(1), dim3(64), 0, st, d_n_matches, tcount, toff, ntiles, list_base);
    e = hipGetLastError();
  }
  if (e == hipSuccess && capacity) {
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)iters), dim3(QBLOCK), 0, st, res, count, first_instance, *q,
                       tcount, toff, list_base, d_ids, reinterpret_cast<uint4*>(d_matched), capacity);
    e = hipGetLastError();
  }
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

}  // extern "C"
