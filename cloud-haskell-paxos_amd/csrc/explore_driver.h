// explore_driver.h — the explorers' driver (include/paxos_batch.h,
// docs/SEMANTICS.md §12, §15, §17): what pxb_explore (paxos_explore.hip),
// pxb_explore_cover (paxos_explore_cover.hip) and pxb_explore_win
// (paxos_explore_win.hip) share around their candidate kernels, as
// shrink_driver.h is the shrinkers'.  Everything is over a space policy X
// (explore_core.h: ExploreLinkX; explore_win_core.h: ExploreWinX): the
// candidates of a parent, their split, their cell, the minimality rule.
//   What follows the candidate kernel, over the candidates' flag bytes: the
//     minimal kernel with the per-(parent, cell) counts and the status,
//     hipCUB's exclusive sum over the tiles, the cursor kernel and the scatter
//     kernel.
//   explore_validate<X>: the argument rules of every exploring call, the bits
//     the space's flags may hold among them (a family's own rules, how its
//     space is made, and the kernel of the shape, stay with the family).
//   explore_device<X>: the one device form after validation.  Parameterised by
//     the candidate launch: the kernel, and its parameter struct, of which the
//     family has set its own fields and the driver fills those every such
//     struct has under the same names; and by hooks that may queue kernels in
//     front of and behind the candidate launch and test a column's alignment.
//   explore_staged<X>: the chunked host-buffer form around a device form given
//     as a callable, with one optional per-parent column of the family's.
// The kernels live in an unnamed namespace: each of the including units has its own.
// Included only where entry points are (hipCUB).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "explore_core.h"
#include "host_util.h"

extern "C" uint64_t explore_chunk_hook(void);   // paxos_batch.hip: PXB_EXPLORE_CHUNK

namespace pxx {
namespace {
using namespace pxb::ev;
using namespace pxb::host;

constexpr int XBLOCK = 256;                       // candidates per tile of the list (4 waves)
constexpr int XWAVES = XBLOCK / 64;
constexpr uint64_t MAX_CALL = 1ull << 32;         // candidates of one device call

template <class X>
struct ExpList {
  typename X::Space x;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t total;
  uint32_t P;                       // the call's proposer count
  uint32_t sel;                     // the listed bit: EXP_MINIMAL or EXP_HELD
  uint8_t* bytes;
  uint32_t* tcount;                 // listed candidates per tile
  uint32_t* counts;                 // count * X::CELLS * 3, zeroed (nullable)
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

template <class X>
__global__ __launch_bounds__(XBLOCK) void explore_minimal_kernel(ExpList<X> k) {
  __shared__ uint32_t s_w[XWAVES];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t g = (uint64_t)blockIdx.x * XBLOCK + threadIdx.x;
  const bool in = g < k.total;
  uint32_t f = 0u, key = 0u;
  if (in) {
    const ExploreSplit s = X::split(k.x, (uint32_t)g);   // (g < 2^32)
    const uint32_t i = s.i;
    key = i * X::CELLS + X::cell(k.x, s.h, s.c);
    f = k.bytes[g];
    // (the other candidates' held bits are final: this kernel only ever adds the minimal bit)
    if ((f & EXP_HELD) && X::is_minimal(k.x, s.h, s.c, k.bytes + (uint64_t)i * (uint32_t)X::total(k.x))) {
      f |= EXP_MINIMAL;
      k.bytes[g] = (uint8_t)f;
    }
    if (s.cw == 0u && k.status)
      k.status[i] = explore_parent_bad(k.rows + (uint64_t)i * k.stride, k.P) ? PXB_SCRIPT_BAD : PXB_TRACE_OK;
  }
  if (k.counts) {
    // {ran OK, held, minimal} per (parent, cell): one add per distinct key of the wave and column
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
// the *_row entry points' link part: out_row (which may be `parent`) = the
// parent's row with the links of link candidate c (< e.T) rewritten
inline int explore_row_links(const pxb_config* cfg, uint32_t depth, uint32_t site_depth, const ExploreSpace& e,
                             const uint8_t* parent, uint64_t c, uint8_t* out_row) {
  const uint32_t N = cfg->n_acceptors;
  const ExploreByte x = explore_byte(e, explore_unrank(e, c), parent, N, site_depth, depth);
  if (explore_changes_keep(x)) return PXB_E_INVAL;
  if (out_row != parent) memcpy(out_row, parent, (size_t)script_stride(cfg->n_proposers, N, depth));
  uint8_t* const links = out_row + script_links_off(N);
  for (uint32_t i = 0; i < 3u; ++i)
    if (x.idx[i] != EXP_NO_SITE) links[x.idx[i]] = (uint8_t)explore_alt(x.links[x.idx[i]], x.dig[i], x.A);
  return PXB_OK;
}

// an exploring call's arguments, whichever the family: device pointers in a
// device form, host pointers in a host-buffer form
struct ExpArgs {
  const pxb_config* cfg;
  const uint8_t* rows;
  uint64_t count;
  uint32_t depth;
  uint64_t first_parent;
  uint64_t* ids;
  uint64_t capacity;
  uint64_t* n_matches;
  uint32_t* counts;                 // (nullable, as status)
  uint32_t* status;
};
// the argument rules every exploring call shares, behind the rules of the
// family's space (validate_space_of, and what the family adds); Space: the
// call's space struct (what flag_mask may be is the family's rule)
template <class X, class Space>
inline int explore_validate(const ExpArgs& a, const Space* sp) {
  if ((a.count && !a.rows) || a.count > MAX_COUNT || !a.n_matches || (a.capacity && !a.ids)) return PXB_E_INVAL;
  return (sp->flags & ~X::FLAGS) ? PXB_E_INVAL : PXB_OK;
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
template <class X>
inline hipError_t explore_list(const ExpList<X>& l, const ExpScratch& s, uint64_t first_g, uint64_t* d_ids,
                               uint64_t capacity, uint64_t* d_n_matches, hipStream_t st) {
  hipLaunchKernelGGL(explore_minimal_kernel<X>, dim3((unsigned)s.ntiles), dim3(XBLOCK), 0, st, l);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
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

// (a family with nothing around its candidate kernel)
struct ExploreNoHooks {
  bool aligned() const { return true; }
  hipError_t before(hipStream_t) const { return hipSuccess; }
  hipError_t after(hipStream_t) const { return hipSuccess; }
};

// The device form over validated arguments `a` and the space `x` on stream st:
// one call's bound and the pointers' alignment (hooks.aligned(): the family's
// own column's), then the counts zeroed | hooks.before(st) | fn(c) over the
// candidates | hooks.after(st) | the minimal bits, counts, status and list, in
// this order on st.  `c`: the candidate kernel's parameters with the family's
// own fields set; p, x, rows, stride, total, depth, site_depth, flag_mask and
// bytes are set here.
template <class X, class Params, class Space, class Hooks>
int explore_device(const ExpArgs& a, const Space* sp, const typename X::Space& x, hipStream_t st, void (*fn)(Params),
                   Params& c, const Hooks& hooks) {
  const uint64_t T = X::total(x);
  if (a.count * T > MAX_CALL) return PXB_E_INVAL;                       // (count <= 2^30, T <= 2^30)
  if (((uintptr_t)a.rows & 7u) || ((uintptr_t)a.ids & 7u) || ((uintptr_t)a.n_matches & 7u) ||
      ((uintptr_t)a.counts & 3u) || ((uintptr_t)a.status & 3u) || !hooks.aligned())
    return PXB_E_INVAL;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (a.count == 0) return PXB_OK;

  const uint64_t total = a.count * T;
  ExpScratch s;
  if (int rc = explore_scratch(dev, total, st, &s)) return rc;

  c.p = make_params(a.cfg);
  c.p.first_instance = 0;
  c.x = x;
  c.rows = a.rows;
  c.stride = script_stride(a.cfg->n_proposers, a.cfg->n_acceptors, a.depth);
  c.total = total;
  c.depth = a.depth;
  c.site_depth = sp->site_depth;
  c.flag_mask = sp->flag_mask;
  c.bytes = s.bytes;
  ExpList<X> l{};
  l.x = x;
  l.rows = a.rows;
  l.stride = c.stride;
  l.total = total;
  l.P = a.cfg->n_proposers;
  l.sel = (sp->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  l.bytes = s.bytes;
  l.tcount = s.tcount;
  l.counts = a.counts;
  l.status = a.status;

  hipError_t err = hipSuccess;
  do {
    if (a.counts && (err = hipMemsetAsync(a.counts, 0, (size_t)(a.count * X::CELLS * 3u * 4u), st)) != hipSuccess) break;
    if ((err = hooks.before(st)) != hipSuccess) break;
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 63u) / 64u)), dim3(64), 0, st, c);
    if ((err = hipGetLastError()) != hipSuccess) break;
    if ((err = hooks.after(st)) != hipSuccess) break;
    err = explore_list(l, s, a.first_parent * T, a.ids, a.capacity, a.n_matches, st);
  } while (0);
  const hipError_t f = hipFreeAsync(s.buf, st);   // (stream-ordered: after the launches above)
  if (err == hipSuccess) err = f;
  return (err == hipSuccess) ? PXB_OK : hip_fail(err);
}

// The host-buffer form over validated host arguments `h`, around a device form:
// whole parents, at most PXB_EXPLORE_CHUNK candidates a chunk (and at least one
// parent); call(d, d_extra) runs the device form on the null stream over the
// chunk's device arguments `d`.  `extra` (nullable), of extra_elem bytes a
// parent (0: the family has none): the family's own per-parent output column.
// An output the caller did not ask for reaches the device form as null.
template <class X, class Call>
int explore_staged(const ExpArgs& h, const typename X::Space& x, void* extra, uint64_t extra_elem, const Call& call) {
  const uint64_t T = X::total(x), cnt_words = X::CELLS * 3u;
  if (device_count() == 0) return PXB_E_NODEV;
  *h.n_matches = 0;
  if (h.count == 0) return PXB_OK;
  const uint64_t chunk = explore_chunk_hook();
  const uint64_t per = chunk / T ? chunk / T : 1u, m_max = per < h.count ? per : h.count;
  const uint64_t stride = script_stride(h.cfg->n_proposers, h.cfg->n_acceptors, h.depth);
  const uint64_t cap = h.capacity < h.count * T ? h.capacity : h.count * T;
  pxb::StagePlan plan;                            // rows (one chunk) | cursor | ids | counts | [extra] | status
  const pxb::StageRegion r_rows = plan.add(stride, m_max), r_n = plan.add(sizeof(uint64_t), 1);
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), cap), r_cnt = plan.add(cnt_words * sizeof(uint32_t), h.count);
  const pxb::StageRegion r_x = plan.add(extra_elem, h.count), r_st = plan.add(sizeof(uint32_t), h.count);
  Staging S(plan);
  S.zero(r_n);
  uint32_t* const d_cnt = S.ptr<uint32_t>(r_cnt, h.counts);
  char* const d_x = S.ptr<char>(r_x, extra);
  uint32_t* const d_st = S.ptr<uint32_t>(r_st, h.status);
  for (uint64_t a = 0; a < h.count && S.ok(); a += m_max) {
    const uint64_t m = h.count - a < m_max ? h.count - a : m_max;
    S.up(r_rows, h.rows + a * stride, m);
    const ExpArgs d{h.cfg, S.ptr<uint8_t>(r_rows), m, h.depth, a, S.ptr<uint64_t>(r_ids), cap, S.ptr<uint64_t>(r_n),
                    d_cnt ? d_cnt + a * cnt_words : nullptr, d_st ? d_st + a : nullptr};
    if (S.ok()) S.note(call(d, d_x ? d_x + a * extra_elem : nullptr));
    // (the next chunk's rows overwrite these: wait for the kernels that read them)
    if (S.ok()) S.note(hipStreamSynchronize(nullptr));
  }
  S.down(r_n, h.n_matches, 1);
  if (S.ok()) S.down(r_ids, h.ids, *h.n_matches < cap ? *h.n_matches : cap);
  S.down(r_cnt, h.counts, h.count);
  S.down(r_x, extra, h.count);
  S.down(r_st, h.status, h.count);
  return S.finish();
}
}  // namespace
}  // namespace pxx
