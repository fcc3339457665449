// explore_list.h — what follows the candidate kernel of an exploration, shared
// by pxb_explore (paxos_explore.hip) and pxb_explore_cover
// (paxos_explore_cover.hip) over the candidates' flag bytes: the minimal kernel
// with the per-(parent, radius) counts and the status, hipCUB's exclusive sum
// over the tiles, the cursor kernel and the scatter kernel, the call's scratch
// and the rules of a space.  The kernels live in an unnamed namespace: each of
// the two units has its own.  Included only where entry points are (hipCUB).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/paxos_batch.h"
#include "explore_core.h"
#include "host_util.h"

namespace pxx {
namespace {
using namespace pxb::ev;
using namespace pxb::host;

constexpr int XBLOCK = 256;                       // candidates per tile of the list (4 waves)
constexpr int XWAVES = XBLOCK / 64;
constexpr uint64_t MAX_CALL = 1ull << 32;         // candidates of one device call

struct ExpList {
  ExploreSpace e;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t total;
  uint32_t P;                       // the call's proposer count
  uint32_t sel;                     // the listed bit: EXP_MINIMAL or EXP_HELD
  uint8_t* bytes;
  uint32_t* tcount;                 // listed candidates per tile
  uint32_t* counts;                 // count * 4 * 3, zeroed (nullable)
  uint32_t* status;                 // count (nullable)
};

__device__ __forceinline__ uint32_t block_sum(uint32_t wave_value, uint32_t* s_w) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0u) s_w[w] = wave_value;
  __syncthreads();
  uint32_t t = 0u;
#pragma unroll
  for (int j = 0; j < XWAVES; ++j) t += s_w[j];
  return t;
}

__global__ __launch_bounds__(XBLOCK) void explore_minimal_kernel(ExpList k) {
  __shared__ uint32_t s_w[XWAVES];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t g = (uint64_t)blockIdx.x * XBLOCK + threadIdx.x;
  const bool in = g < k.total;
  uint32_t f = 0u, key = 0u;
  if (in) {
    const uint32_t tt = (uint32_t)k.e.T, i = (uint32_t)g / tt, c = (uint32_t)g - i * tt;   // (g < 2^32)
    key = i * 4u + explore_radius(k.e, c);
    f = k.bytes[g];
    // (the other candidates' held bits are final: this kernel only ever adds the minimal bit)
    if ((f & EXP_HELD) && explore_is_minimal(k.e, explore_unrank(k.e, c), k.bytes + (uint64_t)i * tt)) {
      f |= EXP_MINIMAL;
      k.bytes[g] = (uint8_t)f;
    }
    if (c == 0u && k.status)
      k.status[i] = explore_parent_bad(k.rows + (uint64_t)i * k.stride, k.P) ? PXB_SCRIPT_BAD : PXB_TRACE_OK;
  }
  if (k.counts) {
    // {ran OK, held, minimal} per (parent, radius): one add per distinct key of the wave and column
    unsigned long long act = __ballot(f != 0u);
    while (act != 0ull) {                         // (wave-uniform)
      const int lead = __ffsll(act) - 1;
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
      const bool same = (f != 0u) & (key == k0);
      const uint32_t n0 = (uint32_t)__popcll(__ballot(same & ((f & EXP_RAN) != 0u)));
      const uint32_t n1 = (uint32_t)__popcll(__ballot(same & ((f & EXP_HELD) != 0u)));
      const uint32_t n2 = (uint32_t)__popcll(__ballot(same & ((f & EXP_MINIMAL) != 0u)));
      if ((int)lane == lead) {
        uint32_t* const o = k.counts + (uint64_t)k0 * 3u;
        if (n0) atomicAdd(o, n0);
        if (n1) atomicAdd(o + 1, n1);
        if (n2) atomicAdd(o + 2, n2);
      }
      act &= ~__ballot(same);
    }
  }
  const uint32_t n = block_sum((uint32_t)__popcll(__ballot((f & k.sel) != 0u)), s_w);
  if (threadIdx.x == 0u) k.tcount[blockIdx.x] = n;
}

// the list's base for this call = the caller's cursor; cursor += the call's matches
__global__ void explore_cursor_kernel(uint64_t* __restrict__ cursor, const uint32_t* __restrict__ tcount,
                                      const uint64_t* __restrict__ toff, uint64_t ntiles,
                                      uint64_t* __restrict__ list_base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t b = *cursor;
    *list_base = b;
    *cursor = b + toff[ntiles - 1] + tcount[ntiles - 1];
  }
}

__global__ __launch_bounds__(XBLOCK) void explore_scatter_kernel(const uint8_t* __restrict__ bytes, uint64_t total,
                                                                 uint32_t sel, uint64_t first_g,
                                                                 const uint32_t* __restrict__ tcount,
                                                                 const uint64_t* __restrict__ toff,
                                                                 const uint64_t* __restrict__ list_base,
                                                                 uint64_t* __restrict__ ids, uint64_t capacity) {
  __shared__ uint32_t s_w[XWAVES];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  // (both block-uniform) no listed candidate in the tile, or the list is full
  if (tcount[blockIdx.x] == 0u) return;
  const uint64_t pos = *list_base + toff[blockIdx.x];
  if (pos >= capacity) return;
  const uint64_t g = (uint64_t)blockIdx.x * XBLOCK + threadIdx.x;
  const bool m = g < total && (bytes[g] & sel) != 0u;
  const unsigned long long bal = __ballot(m);
  if (lane == 0u) s_w[w] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0u;
#pragma unroll
  for (int j = 0; j < XWAVES; ++j) before += (j < (int)w) ? s_w[j] : 0u;
  const uint64_t at = pos + before + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (m && at < capacity) ids[at] = first_g + g;
}

// the space of a call (T = 0: none)
inline ExploreSpace space_of(const pxb_config* cfg, uint32_t site_depth, uint32_t radius) {
  return explore_space(explore_sites(cfg->n_proposers, cfg->n_acceptors, site_depth), cfg->delay_max, radius);
}
// the rules of a row's space: pxb_explore_row's, and part of the calls'
inline int validate_space_of(const pxb_config* cfg, uint32_t depth, uint32_t site_depth, uint32_t radius,
                             ExploreSpace* e) {
  if (!cfg || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  if (site_depth == 0u || site_depth > depth || radius > PXB_EXPLORE_MAX_RADIUS) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  *e = space_of(cfg, site_depth, radius);
  return e->T ? PXB_OK : PXB_E_INVAL;
}

// the scratch of a device call over `total` candidates, from the stream-ordered
// pool: list base | flag bytes | tile counts | tile offsets | scan
struct ExpScratch {
  char* buf;
  uint64_t ntiles;
  size_t scan_b;
  uint64_t* list_base;
  uint8_t* bytes;
  uint32_t* tcount;
  uint64_t* toff;
  void* scan_tmp;
};
inline int explore_scratch(int dev, uint64_t total, hipStream_t st, ExpScratch* s) {
  s->buf = nullptr;
  s->ntiles = (total + XBLOCK - 1) / XBLOCK;
  s->scan_b = 0;
  if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, s->scan_b, widen_iter(nullptr, Widen{}),
                                                      (uint64_t*)nullptr, (int64_t)s->ntiles, st))
    return hip_fail(e);
  const size_t bytes_b = pad256((size_t)total), cnt_b = pad256((size_t)(s->ntiles * 4u)),
               off_b = pad256((size_t)(s->ntiles * 8u));
  if (int rc = pxw::scratch(dev, 256u + bytes_b + cnt_b + off_b + s->scan_b, st, reinterpret_cast<void**>(&s->buf)))
    return rc;
  s->list_base = reinterpret_cast<uint64_t*>(s->buf);
  s->bytes = reinterpret_cast<uint8_t*>(s->buf + 256u);
  s->tcount = reinterpret_cast<uint32_t*>(s->buf + 256u + bytes_b);
  s->toff = reinterpret_cast<uint64_t*>(s->buf + 256u + bytes_b + cnt_b);
  s->scan_tmp = s->buf + 256u + bytes_b + cnt_b + off_b;
  return PXB_OK;
}

// behind the candidate kernel on st: the minimal bits, counts and status, then the list
inline hipError_t explore_list(const ExpList& l, const ExpScratch& s, uint64_t first_g, uint64_t* d_ids,
                               uint64_t capacity, uint64_t* d_n_matches, hipStream_t st) {
  hipError_t err = hipSuccess;
  hipLaunchKernelGGL(explore_minimal_kernel, dim3((unsigned)s.ntiles), dim3(XBLOCK), 0, st, l);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  size_t scan_b = s.scan_b;
  err = hipcub::DeviceScan::ExclusiveSum(s.scan_tmp, scan_b, widen_iter(s.tcount, Widen{}), s.toff, (int64_t)s.ntiles, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(explore_cursor_kernel, dim3(1), dim3(64), 0, st, d_n_matches, s.tcount, s.toff, s.ntiles,
                     s.list_base);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  if (capacity) {
    hipLaunchKernelGGL(explore_scatter_kernel, dim3((unsigned)s.ntiles), dim3(XBLOCK), 0, st, s.bytes, l.total, l.sel,
                       first_g, s.tcount, s.toff, s.list_base, d_ids, capacity);
    err = hipGetLastError();
  }
  return err;
}

}  // namespace
}  // namespace pxx
