// paxos_trace_batch.hip — pxb_trace_batch: many instances through the per-lane
// state machine (paxos_ev.h) in one launch, 64 per wave, with the records a
// selection keeps written contiguously in the order of the id list.
//
// Ordered compaction in the library's usual shape (wire codec, query): two
// passes of one kernel with hipCUB's exclusive sum between them, and no block
// that waits for another:
//   1. count   lane l of block b runs ids[64 b + l] to its end and counts the
//              visited steps inside the window; writes the count (scratch), the
//              status and the result;
//   2. scan    exclusive sum of min(count, tail) (count + 1 entries: the last
//              is the total) into d_offsets;
//   3. write   the same kernel with records on: the state machine is
//              deterministic, so the re-run visits the same steps; in-window
//              record j of instance i goes to d_offsets[i] + j - skip_i.  A
//              block whose first offset is at or past `capacity` exits at once,
//              a lane stops once none of its later records can be kept.
// The wave stays together: lanes that have finished idle, and the loop's back
// edge is one ballot (EvLane::step's any_lane ballots then see the live lanes).
//
// Built as three units by proposer count (-DPXB_TRB_P=1|2|3), as paxos_ev.hip
// is; the unit of P = 1 also holds the entry points.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "paxos_ev_kernel.h"
#include "paxos_trace_core.h"

#ifndef PXB_TRB_P
#error "PXB_TRB_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct TrbParams {
  EvParams p;
  const uint64_t* ids;
  uint64_t count;
  uint32_t smin, smax, tail;
  uint32_t* cnt;                    // in-window records per instance (count pass: out; write pass: in)
  const uint64_t* offsets;          // write pass: d_offsets
  pxb_trace_step* out;              // write pass: d_records (count pass: null)
  uint64_t capacity;
  uint32_t* status;                 // count pass, nullable
  uint4* res;                       // count pass, nullable
};

typedef void (*trb_ptr)(TrbParams);
// one per unit: the kernel of a shape (null: none)
trb_ptr trb_pick_p1(uint32_t n, int w, bool lg, bool prod);
trb_ptr trb_pick_p2(uint32_t n, int w, bool lg, bool prod);
trb_ptr trb_pick_p3(uint32_t n, int w, bool lg, bool prod);

// the shapes and pools of paxos_trace_kernel
template <int PM, int N, int W, bool EARLY, bool LG = false>
__global__ __launch_bounds__(64) void paxos_trace_batch_kernel(TrbParams k) {
  constexpr int POOL = EvPool<PM, N, false, LG>::value;
  using S = Shape<PM, N, POOL, W, false, LG>;
  using Lane = EvLane<PM, N, POOL, W, false, LdsMem, EARLY, LG>;
  __shared__ uint32_t lds[S::WORDS * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * 64u, i = i0 + lane;
  const bool write = k.out != nullptr;
  if (write && k.offsets[i0] >= k.capacity) return;     // (wave-uniform; offsets ascend: nothing of this block fits)
  Lane L;
  L.m = LdsMem{lds, lane};
  L.set_keys(k.p);
  TraceLane<Lane> T;
  T.begin_count(k.smin, k.smax);
  bool run = i < k.count;
  if (run && write) {
    const uint32_t c = k.cnt[i];
    const uint64_t base = k.offsets[i];
    run = (c != 0u) & (base < k.capacity);
    if (run) T.begin_write(k.smin, k.smax, c, k.tail, k.out + base, k.capacity - base);
  }
  if (run) {
    EvParams pl = k.p;              // (the lane's own id: init takes first_instance + g)
    pl.first_instance = k.ids[i];
    L.init(pl, 0u);
  }
  while (any_lane(run)) {
    if (run) run = T.iter(L, k.p);
  }
  if (!write && i < k.count) {
    k.cnt[i] = T.n;
    if (k.status) k.status[i] = T.status;
    if (k.res) k.res[i] = make_uint4(T.res[0], T.res[1], T.res[2], T.res[3]);
  }
}

template <int PM, int W, bool E, bool LG = false>
static trb_ptr pick_n(uint32_t n) {
  switch (n) {
    case 2: return paxos_trace_batch_kernel<PM, 2, W, E, LG>;
    case 3: return paxos_trace_batch_kernel<PM, 3, W, E, LG>;
    case 4: return paxos_trace_batch_kernel<PM, 4, W, E, LG>;
    case 5: return paxos_trace_batch_kernel<PM, 5, W, E, LG>;
    case 6: return paxos_trace_batch_kernel<PM, 6, W, E, LG>;
    case 7: return paxos_trace_batch_kernel<PM, 7, W, E, LG>;
    case 8: return paxos_trace_batch_kernel<PM, 8, W, E, LG>;
    case 9: return paxos_trace_batch_kernel<PM, 9, W, E, LG>;
  }
  return nullptr;
}

// (log mode: the 8-step wheel only, as the batch kernels' LG shape)
template <int PM, bool E>
static trb_ptr pick_w(uint32_t n, int w, bool lg) {
  if (lg) return w == 8 ? pick_n<PM, 8, E, true>(n) : nullptr;
  return w == 8 ? pick_n<PM, 8, E>(n) : w == 16 ? pick_n<PM, 16, E>(n) : nullptr;
}

#if PXB_TRB_P == 1
trb_ptr trb_pick_p1(uint32_t n, int w, bool lg, bool prod) { return prod ? pick_w<1, true>(n, w, lg) : pick_w<1, false>(n, w, lg); }
#elif PXB_TRB_P == 2
trb_ptr trb_pick_p2(uint32_t n, int w, bool lg, bool prod) { return prod ? pick_w<2, true>(n, w, lg) : pick_w<2, false>(n, w, lg); }
#elif PXB_TRB_P == 3
trb_ptr trb_pick_p3(uint32_t n, int w, bool lg, bool prod) { return prod ? pick_w<3, true>(n, w, lg) : pick_w<3, false>(n, w, lg); }
#else
#error "PXB_TRB_P must be 1, 2 or 3"
#endif

}  // namespace ev
}  // namespace pxb

#if PXB_TRB_P == 1
#include <hipcub/hipcub.hpp>

namespace pxw {
// paxos_wire.hip: per-call scratch from the device's stream-ordered pool
// (allocated and freed on the caller's stream; pxb_shutdown destroys the pool)
int scratch(int dev, size_t bytes, hipStream_t st, void** p);
}  // namespace pxw

namespace pxtb {
using namespace pxb::ev;

constexpr uint64_t MAX_COUNT = 1ull << 30;

// the scan's input: what the selection keeps of an instance's in-window records
struct Kept {
  uint32_t tail;
  __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& c) const { return trace_kept(c, tail); }
};
typedef hipcub::TransformInputIterator<uint64_t, Kept, const uint32_t*> kept_iter;

int hip_fail(hipError_t e) { return (e == hipErrorOutOfMemory) ? PXB_E_OOM : PXB_E_HIP; }
size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// the argument rules of both forms; *fn: the shape's kernel
int validate(const pxb_config* cfg, const void* ids, uint64_t count, const pxb_trace_sel* sel, const void* records,
             uint64_t capacity, const void* offsets, trb_ptr* fn) {
  if (!cfg || !offsets || (count && !ids) || count > MAX_COUNT) return PXB_E_INVAL;
  if (sel && sel->reserved != 0u) return PXB_E_INVAL;
  if (!records && capacity) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  const bool prod = (cfg->flags & PXB_CFG_TRACE_PRODUCTION) != 0u, lg = cfg->n_ticks > 1;
  const int w = wheel_for(cfg->delay_max);
  *fn = cfg->n_proposers == 1   ? trb_pick_p1(cfg->n_acceptors, w, lg, prod)
        : cfg->n_proposers == 2 ? trb_pick_p2(cfg->n_acceptors, w, lg, prod)
                                : trb_pick_p3(cfg->n_acceptors, w, lg, prod);
  return *fn ? PXB_OK : PXB_E_INVAL;
}

size_t scan_bytes(uint64_t count, hipStream_t st) {
  size_t need = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, kept_iter(nullptr, Kept{0u}), (uint64_t*)nullptr,
                                       (int64_t)(count + 1), st) != hipSuccess)
    return (size_t)-1;
  return need;
}

// count pass + scan (phase 1), write pass (phase 2) over cnt (count + 1 words) and the scan's tmp
hipError_t launch(trb_ptr fn, const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, const pxb_trace_sel* sel,
                  pxb_trace_step* d_records, uint64_t capacity, uint64_t* d_offsets, uint32_t* d_status,
                  pxb_result* d_results, hipStream_t st, uint32_t* cnt, void* tmp, size_t need, int phases) {
  TrbParams k{};
  k.p = make_params(cfg);
  k.p.first_instance = 0;
  k.ids = d_ids;
  k.count = count;
  k.smin = sel ? sel->step_min : 0u;
  k.smax = sel ? sel->step_max : 0xFFFFFFFFu;
  k.tail = sel ? sel->tail : 0u;
  k.cnt = cnt;
  k.offsets = d_offsets;
  k.capacity = capacity;
  const dim3 grid((unsigned)((count + 63) / 64));
  hipError_t e = hipSuccess;
  if (phases & 1) {
    if ((e = hipMemsetAsync(cnt + count, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
    k.out = nullptr;
    k.status = d_status;
    k.res = reinterpret_cast<uint4*>(d_results);
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, need, kept_iter(cnt, Kept{k.tail}), d_offsets, (int64_t)(count + 1), st);
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && capacity && d_records) {
    k.out = d_records;
    k.status = nullptr;
    k.res = nullptr;
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace pxtb

extern "C" {

int pxb_trace_batch_device(const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, const pxb_trace_sel* sel,
                           pxb_trace_step* d_records, uint64_t capacity, uint64_t* d_offsets, uint32_t* d_status,
                           pxb_result* d_results, void* stream) {
  using namespace pxtb;
  trb_ptr fn = nullptr;
  if (int rc = validate(cfg, d_ids, count, sel, d_records, capacity, d_offsets, &fn)) return rc;
  // (the records move as 4-byte words, the results as 16-byte ones)
  if (((uintptr_t)d_ids & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_records & 3u) ||
      ((uintptr_t)d_status & 3u) || ((uintptr_t)d_results & 15u))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return PXB_E_NODEV;
  if (count == 0) {
    const hipError_t e = hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), st);
    return (e == hipSuccess) ? PXB_OK : hip_fail(e);
  }
  const size_t need = scan_bytes(count, st);
  if (need == (size_t)-1) return PXB_E_HIP;
  const size_t cnt_b = pad256((count + 1) * sizeof(uint32_t));
  void* buf = nullptr;
  if (int rc = pxw::scratch(dev, cnt_b + need, st, &buf)) return rc;
  hipError_t e = launch(fn, cfg, d_ids, count, sel, d_records, capacity, d_offsets, d_status, d_results, st,
                        reinterpret_cast<uint32_t*>(buf), reinterpret_cast<char*>(buf) + cnt_b, need, 3);
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

int pxb_trace_batch(const pxb_config* cfg, const uint64_t* ids, uint64_t count, const pxb_trace_sel* sel,
                    pxb_trace_step* records, uint64_t capacity, uint64_t* offsets, uint32_t* status,
                    pxb_result* results, uint64_t* n_records) {
  using namespace pxtb;
  trb_ptr fn = nullptr;
  if (int rc = validate(cfg, ids, count, sel, records, capacity, offsets, &fn)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PXB_E_NODEV;
  if (count == 0) {
    offsets[0] = 0;
    if (n_records) *n_records = 0;
    return PXB_OK;
  }
  const size_t need = scan_bytes(count, 0);
  if (need == (size_t)-1) return PXB_E_HIP;
  const size_t ids_b = pad256(count * sizeof(uint64_t)), off_b = pad256((count + 1) * sizeof(uint64_t));
  const size_t cnt_b = pad256((count + 1) * sizeof(uint32_t)), st_b = pad256(count * sizeof(uint32_t));
  const size_t res_b = pad256(count * sizeof(pxb_result));
  char* buf = nullptr;                            // ids | offsets | counts | status | results | the scan's
  pxb_trace_step* d_rec = nullptr;
  hipError_t e = hipSuccess;
  do {
    if ((e = hipMalloc(&buf, ids_b + off_b + cnt_b + st_b + res_b + need)) != hipSuccess) break;
    uint64_t* d_ids = reinterpret_cast<uint64_t*>(buf);
    uint64_t* d_off = reinterpret_cast<uint64_t*>(buf + ids_b);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(buf + ids_b + off_b);
    uint32_t* d_st = reinterpret_cast<uint32_t*>(buf + ids_b + off_b + cnt_b);
    pxb_result* d_res = reinterpret_cast<pxb_result*>(buf + ids_b + off_b + cnt_b + st_b);
    void* tmp = buf + ids_b + off_b + cnt_b + st_b + res_b;
    if ((e = hipMemcpy(d_ids, ids, count * sizeof(uint64_t), hipMemcpyHostToDevice)) != hipSuccess) break;
    if ((e = launch(fn, cfg, d_ids, count, sel, nullptr, 0, d_off, status ? d_st : nullptr, results ? d_res : nullptr,
                    0, d_cnt, tmp, need, 1)) != hipSuccess)
      break;
    if ((e = hipMemcpy(offsets, d_off, (count + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost)) != hipSuccess) break;
    const uint64_t total = offsets[count], m = total < capacity ? total : capacity;
    if (m) {
      if ((e = hipMalloc(&d_rec, m * sizeof(pxb_trace_step))) != hipSuccess) break;
      if ((e = launch(fn, cfg, d_ids, count, sel, d_rec, m, d_off, nullptr, nullptr, 0, d_cnt, tmp, need, 2)) != hipSuccess)
        break;
      if ((e = hipMemcpy(records, d_rec, m * sizeof(pxb_trace_step), hipMemcpyDeviceToHost)) != hipSuccess) break;
    }
    if (status && (e = hipMemcpy(status, d_st, count * sizeof(uint32_t), hipMemcpyDeviceToHost)) != hipSuccess) break;
    if (results && (e = hipMemcpy(results, d_res, count * sizeof(pxb_result), hipMemcpyDeviceToHost)) != hipSuccess) break;
    if (n_records) *n_records = total;
  } while (0);
  if (d_rec) (void)hipFree(d_rec);
  if (buf) (void)hipFree(buf);
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

}  // extern "C"
#endif  // PXB_TRB_P == 1
