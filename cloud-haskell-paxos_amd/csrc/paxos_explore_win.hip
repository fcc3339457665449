// paxos_explore_win.hip — isolation windows as sites of the exploration
// (include/paxos_batch.h, docs/SEMANTICS.md §17): pxb_explore_win,
// pxb_explore_win_device, pxb_explore_win_row and pxb_explore_win_total.
//
// pxb_explore_cover's candidate kernel with three changes.  Lane l of block b is
// candidate 64 b + l of the call, g = i T_w + h T + c: it unranks the link part c
// as there and the window choice h into at most two (acceptor, digit) pairs in
// registers; behind explore_cover_begin it overwrites the lane's windows of the
// changed acceptors (explore_win_core.h: an unrolled walk with selects); and its
// wave reduction walks (parent, r_w, r_l) keys, 12 per parent in place of 4,
// with first[r_w][r_l][b] per cell.  No candidate row, event or mask is stored;
// integer adds and minima only; no block waits for another; plain vector stores.
// The family has its own minimal kernel (the two-axis subset rule, the 12-cell
// counts); the list, the scratch and the host side are explore_driver.h's.
//
// Built as three units by proposer count (-DPXB_EXW_P=1|2|3); the unit of P = 1
// also holds the other kernels and the entry points.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "explore_win_core.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_EXW_P
#error "PXB_EXW_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct ExwParams {
  EvParams p;
  ExploreWin x;
  const uint8_t* rows;              // the parents' rows
  uint64_t stride;
  uint64_t total;                   // candidates of this call (count * T_w <= 2^32)
  uint32_t depth, site_depth, flag_mask;
  pxb_cover_query q;
  uint8_t* bytes;                   // total flag bytes
  pxb_explore_win_reach* reach;     // count records, initialised (nullable)
};

template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_explore_win_kernel(ExwParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ExploreEventDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
  constexpr uint32_t NL = 2u * PM * N;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 64u + lane;
  const bool in = g < k.total;
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  L.e_acc = L.e_pin = false;
  CoverLane<Lane> E;
  E.begin();
  bool run = in;
  if (run) {
    const uint32_t tw = (uint32_t)k.x.Tw, tt = (uint32_t)k.x.e.T;   // (g < 2^32)
    const uint32_t i = (uint32_t)g / tw, cw = (uint32_t)g - i * tw, h = cw / tt, c = cw - h * tt;
    const uint8_t* const row = k.rows + (uint64_t)i * k.stride;
    const ExploreByte x = explore_byte(k.x.e, explore_unrank(k.x.e, c), row, N, k.site_depth, k.depth);
    // a malformed parent runs nothing; a candidate that changes a keep site is skipped
    run = !explore_parent_bad(row, PM) && !explore_changes_keep(x);
    if (run) run = explore_cover_begin(L, k.p, k.depth, row, x) == PXB_TRACE_OK;
    if (run) explore_win_apply(L, k.x.w, explore_win_unrank(k.x.w, h));
  }
  const bool started = run;
  script_run(L, E, k.p, run);
  uint32_t f = 0u, m = 0u;
  if (started && E.status == PXB_TRACE_OK) {
    uint16_t snt[NL];
    script_sent(L, snt);
    f = explore_cover_flags(E.res[3], E.mask, snt, NL, k.depth, k.flag_mask, k.q);
    m = (f & EXP_RAN) ? E.mask : 0u;
  }
  if (in) k.bytes[g] = (uint8_t)f;
  if (k.reach == nullptr) return;   // (wave-uniform)
  // ---- the wave's reduction into the reach records ----
  // (the key is worked out again here, as the coverage kernel does)
  uint32_t key = 0u, cw = 0u;
  if (in) {
    const uint32_t tw = (uint32_t)k.x.Tw, tt = (uint32_t)k.x.e.T, i = (uint32_t)g / tw;
    cw = (uint32_t)g - i * tw;
    const uint32_t h = cw / tt;
    key = i * EXW_CELLS + explore_win_cell(k.x, h, cw - h * tt);
    if (cw == 0u) k.reach[i].parent_mask = m;
  }
  unsigned long long act = __ballot(m != 0u);
  while (act != 0ull) {             // (wave-uniform) one distinct (parent, r_w, r_l) a turn
    const int lead = __ffsll(act) - 1;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const bool same = (m != 0u) & (key == k0);
    pxb_explore_win_reach* const o = k.reach + k0 / EXW_CELLS;
    const uint32_t off = (k0 % EXW_CELLS) * 32u;
    uint32_t* const cnt = &o->count[0][0][0] + off;
    uint32_t* const fst = &o->first[0][0][0] + off;
#pragma unroll 1
    for (uint32_t b = 0; b < (uint32_t)PXB_COVER_CLASSES; ++b) {
      const unsigned long long bal = __ballot(same & (((m >> b) & 1u) != 0u));
      if (bal == 0ull) continue;    // (wave-uniform: no candidate of the key has the class)
      // (within one parent c' ascends with the lane: the lowest such lane has the least)
      const uint32_t cmin = (uint32_t)__builtin_amdgcn_readlane((int)cw, __ffsll(bal) - 1);
      if ((int)lane == lead) {
        atomicAdd(cnt + b, (uint32_t)__popcll(bal));
        atomicMin(fst + b, cmin);
      }
    }
    act &= ~__ballot(same);
  }
}

typedef void (*exw_ptr)(ExwParams);
struct ExwFamily {                  // (lane_shapes.h)
  typedef exw_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_explore_win_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ExwFamily, PXB_EXW_P)

}  // namespace ev
}  // namespace pxb

#if PXB_EXW_P == 1
#include "explore_driver.h"

namespace pxx {

constexpr uint32_t WREACH_WORDS = (uint32_t)(sizeof(pxb_explore_win_reach) / 4u);   // 384 counts | 384 firsts | 2 masks
constexpr uint32_t WCOUNT_WORDS = EXW_CELLS * 3u;

struct ExwList {
  ExploreWin x;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t total;
  uint32_t P;                       // the call's proposer count
  uint32_t sel;                     // the listed bit: EXP_MINIMAL or EXP_HELD
  uint8_t* bytes;
  uint32_t* tcount;                 // listed candidates per tile
  uint32_t* counts;                 // count * 12 * 3, zeroed (nullable)
  uint32_t* status;                 // count (nullable)
};

// explore_minimal_kernel over the joint space: the two-axis subset rule, and
// {ran OK, held, minimal} per (parent, r_w, r_l)
__global__ __launch_bounds__(XBLOCK) void explore_win_minimal_kernel(ExwList k) {
  __shared__ uint32_t s_w[XWAVES];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t g = (uint64_t)blockIdx.x * XBLOCK + threadIdx.x;
  const bool in = g < k.total;
  uint32_t f = 0u, key = 0u;
  if (in) {
    const uint32_t tw = (uint32_t)k.x.Tw, tt = (uint32_t)k.x.e.T;   // (g < 2^32)
    const uint32_t i = (uint32_t)g / tw, cw = (uint32_t)g - i * tw, h = cw / tt, c = cw - h * tt;
    key = i * EXW_CELLS + explore_win_cell(k.x, h, c);
    f = k.bytes[g];
    // (the other candidates' held bits are final: this kernel only ever adds the minimal bit)
    if ((f & EXP_HELD) && explore_win_is_minimal(k.x, explore_win_unrank(k.x.w, h), explore_unrank(k.x.e, c),
                                                 k.bytes + (uint64_t)i * tw)) {
      f |= EXP_MINIMAL;
      k.bytes[g] = (uint8_t)f;
    }
    if (cw == 0u && k.status)
      k.status[i] = explore_parent_bad(k.rows + (uint64_t)i * k.stride, k.P) ? PXB_SCRIPT_BAD : PXB_TRACE_OK;
  }
  if (k.counts) {
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

// one thread per word of the records: counts 0, firsts all-ones, masks 0
__global__ __launch_bounds__(256) void win_reach_init_kernel(uint32_t* words, uint64_t n_words) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_words) return;
  const uint32_t w = (uint32_t)(t % WREACH_WORDS);
  words[t] = (w >= 384u && w < 768u) ? 0xFFFFFFFFu : 0u;
}

// behind the candidate kernel, 32 threads a parent, thread b: the union of the counted classes
__global__ __launch_bounds__(32) void win_reach_finish_kernel(pxb_explore_win_reach* reach) {
  pxb_explore_win_reach* const o = reach + blockIdx.x;
  const uint32_t b = threadIdx.x;
  uint32_t any = 0u;
#pragma unroll
  for (uint32_t cell = 0; cell < EXW_CELLS; ++cell) any |= (&o->count[0][0][0])[cell * 32u + b];
  const unsigned long long bal = __ballot(any != 0u);
  if (b == 0u) o->union_mask = (uint32_t)bal;
}

// the joint space of a call (Tw = 0: none); the link part's rules are validate_space_of's
static int win_space_of(const pxb_config* cfg, uint32_t depth, const pxb_explore_win_space* sp, ExploreWin* x) {
  if (!sp) return PXB_E_INVAL;
  ExploreSpace e;
  if (int rc = validate_space_of(cfg, depth, sp->site_depth, sp->radius, &e)) return rc;
  *x = explore_win_make(e, explore_win_space(cfg->n_acceptors, sp->win_radius, sp->win_first, sp->win_starts,
                                             sp->win_lens, (sp->flags & PXB_EXPLORE_WIN_OPEN) != 0u));
  return x->Tw ? PXB_OK : PXB_E_INVAL;
}

// pxb_explore_cover's rules with the window fields'; *fn: the shape's kernel
static int validate(const ExpArgs& a, const pxb_explore_win_space* sp, ExploreWin* x, exw_ptr* fn) {
  if (int rc = win_space_of(a.cfg, a.depth, sp, x)) return rc;
  if ((a.count && !a.rows) || a.count > MAX_COUNT || !a.n_matches || (a.capacity && !a.ids)) return PXB_E_INVAL;
  if (sp->flags & ~(PXB_EXPLORE_MINIMAL | PXB_EXPLORE_WIN_OPEN)) return PXB_E_INVAL;
  if ((sp->flag_mask != 0u && (sp->flag_mask & 0xFFu) == 0u) || sp->q.reserved != 0u) return PXB_E_INVAL;
  if (a.cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  *fn = lane_kernel<ExwFamily>(a.cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

}  // namespace pxx

extern "C" {

uint64_t pxb_explore_win_total(uint32_t P, uint32_t N, uint32_t delay_max, const pxb_explore_win_space* sp) {
  using namespace pxb::ev;
  if (!sp) return 0ull;
  return explore_win_make(explore_space(explore_sites(P, N, sp->site_depth), delay_max, sp->radius),
                          explore_win_space(N, sp->win_radius, sp->win_first, sp->win_starts, sp->win_lens,
                                            (sp->flags & PXB_EXPLORE_WIN_OPEN) != 0u))
      .Tw;
}

int pxb_explore_win_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_win_space* space,
                        const uint8_t* parent, uint64_t c, uint8_t* out_row) {
  using namespace pxx;
  ExploreWin x;
  if (int rc = win_space_of(cfg, depth, space, &x)) return rc;
  if (!parent || !out_row || c >= x.Tw) return PXB_E_INVAL;
  const uint32_t N = cfg->n_acceptors;
  const uint64_t h = c / x.e.T;
  const ExploreByte b = explore_byte(x.e, explore_unrank(x.e, c - h * x.e.T), parent, N, space->site_depth, depth);
  if (explore_changes_keep(b)) return PXB_E_INVAL;
  if (out_row != parent) memcpy(out_row, parent, (size_t)script_stride(cfg->n_proposers, N, depth));
  uint8_t* const links = out_row + script_links_off(N);
  for (uint32_t i = 0; i < 3u; ++i)
    if (b.idx[i] != EXP_NO_SITE) links[b.idx[i]] = (uint8_t)explore_alt(b.links[b.idx[i]], b.dig[i], b.A);
  const WinCand k = explore_win_unrank(x.w, h);
  for (uint32_t i = 0; i < k.r; ++i) {
    uint32_t c0, c1;
    explore_win_bounds(x.w, k.digit[i], &c0, &c1);
    uint8_t* const o = out_row + SCR_HDR + 4u * k.acc[i];
    o[0] = (uint8_t)c0, o[1] = (uint8_t)(c0 >> 8), o[2] = (uint8_t)c1, o[3] = (uint8_t)(c1 >> 8);
  }
  return PXB_OK;
}

int pxb_explore_win_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                           const pxb_explore_win_space* space, uint64_t first_parent, uint64_t* d_ids,
                           uint64_t capacity, uint64_t* d_n_matches, uint32_t* d_counts,
                           pxb_explore_win_reach* d_reach, uint32_t* d_status, void* stream) {
  using namespace pxx;
  const ExpArgs a{cfg, d_rows, count, depth, first_parent, d_ids, capacity, d_n_matches, d_counts, d_status};
  ExploreWin x;
  exw_ptr fn = nullptr;
  if (int rc = validate(a, space, &x, &fn)) return rc;
  if (count * x.Tw > MAX_CALL) return PXB_E_INVAL;                      // (count <= 2^30, T_w <= 2^30)
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_ids & 7u) || ((uintptr_t)d_n_matches & 7u) ||
      ((uintptr_t)d_counts & 3u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_reach & 7u))
    return PXB_E_INVAL;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;
  hipStream_t st = (hipStream_t)stream;

  const uint64_t total = count * x.Tw;
  ExpScratch s;
  if (int rc = explore_scratch(dev, total, st, &s)) return rc;

  ExwParams c{};
  c.p = make_params(cfg);
  c.p.first_instance = 0;
  c.x = x;
  c.rows = d_rows;
  c.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  c.total = total;
  c.depth = depth;
  c.site_depth = space->site_depth;
  c.flag_mask = space->flag_mask;
  c.q = space->q;
  c.bytes = s.bytes;
  c.reach = d_reach;
  ExwList l{};
  l.x = x;
  l.rows = d_rows;
  l.stride = c.stride;
  l.total = total;
  l.P = cfg->n_proposers;
  l.sel = (space->flags & PXB_EXPLORE_MINIMAL) ? EXP_MINIMAL : EXP_HELD;
  l.bytes = s.bytes;
  l.tcount = s.tcount;
  l.counts = d_counts;
  l.status = d_status;

  // the counts zeroed and the records set | the candidates | union_mask | the
  // minimal bits, counts and status | the list, in this order on st
  hipError_t err = hipSuccess;
  do {
    if (d_counts && (err = hipMemsetAsync(d_counts, 0, (size_t)(count * WCOUNT_WORDS * 4u), st)) != hipSuccess) break;
    if (d_reach) {
      const uint64_t n_words = count * WREACH_WORDS;
      hipLaunchKernelGGL(win_reach_init_kernel, dim3((unsigned)((n_words + 255u) / 256u)), dim3(256), 0, st,
                         reinterpret_cast<uint32_t*>(d_reach), n_words);
      if ((err = hipGetLastError()) != hipSuccess) break;
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 63u) / 64u)), dim3(64), 0, st, c);
    if ((err = hipGetLastError()) != hipSuccess) break;
    if (d_reach) {
      hipLaunchKernelGGL(win_reach_finish_kernel, dim3((unsigned)count), dim3(32), 0, st, d_reach);
      if ((err = hipGetLastError()) != hipSuccess) break;
    }
    hipLaunchKernelGGL(explore_win_minimal_kernel, dim3((unsigned)s.ntiles), dim3(XBLOCK), 0, st, l);
    if ((err = hipGetLastError()) != hipSuccess) break;
    err = explore_list_tail(total, l.sel, s, first_parent * x.Tw, d_ids, capacity, d_n_matches, st);
  } while (0);
  const hipError_t f = hipFreeAsync(s.buf, st);   // (stream-ordered: after the launches above)
  if (err == hipSuccess) err = f;
  return (err == hipSuccess) ? PXB_OK : hip_fail(err);
}

int pxb_explore_win(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                    const pxb_explore_win_space* space, uint64_t* ids, uint64_t capacity, uint64_t* n_matches,
                    uint32_t* counts, pxb_explore_win_reach* reach, uint32_t* status) {
  using namespace pxx;
  const ExpArgs h{cfg, rows, count, depth, 0, ids, capacity, n_matches, counts, status};
  ExploreWin x;
  exw_ptr fn = nullptr;
  if (int rc = validate(h, space, &x, &fn)) return rc;
  return explore_staged_over(h, x.Tw, WCOUNT_WORDS, reach, sizeof(pxb_explore_win_reach),
                             [&](const ExpArgs& d, void* d_reach) {
                               return pxb_explore_win_device(cfg, d.rows, d.count, depth, space, d.first_parent, d.ids,
                                                             d.capacity, d.n_matches, d.counts,
                                                             static_cast<pxb_explore_win_reach*>(d_reach), d.status,
                                                             nullptr);
                             });
}

}  // extern "C"
#endif  // PXB_EXW_P == 1
