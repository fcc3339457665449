// paxos_script.hip — scripted schedules (include/paxos_batch.h, docs/SEMANTICS.md
// §10): pxb_schedule_extract, pxb_run_scripted and pxb_trace_scripted.
//
// The run and the trace are one kernel, paxos_trace_batch.hip's with rows in
// place of ids: lane l of block b starts the per-lane state machine on row
// 64 b + l with the scripted draw source (script_core.h) and runs it to its end
// under TraceLane.  The count pass writes the status, the result and, for
// pxb_run_scripted, the digests, the acceptor records and the per-link send
// counts; pxb_trace_scripted adds hipCUB's exclusive sum and the write pass.
// Only the generic shape (every schedule draw tested, 4-entry FIFOs) on the
// wheel of cfg->delay_max: an override may add a loss or a skew to a config
// that has none.  No block waits for another.
//
// The extract is a dense kernel over the rows' bytes: pure Philox.
//
// Built as three units by proposer count (-DPXB_SCR_P=1|2|3) so that the slow
// device compiles overlap; the unit of P = 1 also holds the entry points.  The
// shapes are lane_shapes.h's.  (The kernel spells out what its lane does before
// and after the run, and tests/native/script_host.cpp spells it again: moved into
// shared members, as the trace batch's is, the same text compiled to another
// register allocation and ran 2 - 3 % slower)
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/paxos_batch.h"
#include "lane_shapes.h"
#include "script_lane.h"

#ifndef PXB_SCR_P
#error "PXB_SCR_P: the unit's proposer count (1, 2 or 3)"
#endif

namespace pxb {
namespace ev {

struct ScrParams {
  EvParams p;
  const uint8_t* rows;
  uint64_t stride;
  uint64_t count;
  uint32_t depth;
  uint32_t smin, smax, tail;
  uint32_t* cnt;                    // in-window records per row (count pass: out, nullable; write pass: in)
  const uint64_t* offsets;          // write pass: d_offsets
  pxb_trace_step* out;              // write pass: d_records (count pass: null)
  uint64_t capacity;
  // count pass, all nullable
  uint32_t* status;
  uint4* res;
  uint32_t* digest;                 // count * N
  uint4* acc;                       // count * N acceptor records
  uint16_t* sent;                   // count * 2 P N
};

// the shapes and pools of paxos_trace_batch_kernel's default variant
template <int PM, int N, int W, bool LG = false>
__global__ __launch_bounds__(64) void paxos_script_kernel(ScrParams k) {
  using SL = ScriptLane<PM, N, W, LG, LdsMem, ScriptDraws>;
  using S = typename SL::S;
  using Lane = typename SL::Lane;
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
    const uint32_t st = script_begin(L, k.p, k.depth, k.rows + i * k.stride);
    if (st != PXB_TRACE_OK) {       // a malformed row: not run
      T.status = st;
      run = false;
    }
  }
  script_run(L, T, k.p, run);
  if (!write && i < k.count) {
    if (k.cnt) k.cnt[i] = T.n;
    if (k.status) k.status[i] = T.status;
    if (k.res) k.res[i] = make_uint4(T.res[0], T.res[1], T.res[2], T.res[3]);
    const bool ok = T.status == PXB_TRACE_OK;          // (else the lane's state is not an ended instance's)
    if (k.digest) {
#pragma unroll
      for (int a = 0; a < N; ++a) k.digest[i * N + a] = ok ? L.digest_of(a) : 0u;
    }
    if (k.acc) {
#pragma unroll
      for (int a = 0; a < N; ++a) {
        uint32_t r[4] = {0u, 0u, 0u, 0u};
        if (ok) L.record_of(a, r);
        k.acc[i * N + a] = make_uint4(r[0], r[1], r[2], r[3]);
      }
    }
    if (k.sent) {
      uint16_t* const o = k.sent + i * (2u * PM * N);
      if (ok) {
        script_sent(L, o);
      } else {
#pragma unroll
        for (int j = 0; j < 2 * PM * N; ++j) o[j] = 0u;
      }
    }
  }
}

typedef void (*scr_ptr)(ScrParams);
struct ScrFamily {                  // (lane_shapes.h)
  typedef scr_ptr ptr;
  template <int PM, int N, int W, bool LG>
  static ptr kernel() { return paxos_script_kernel<PM, N, W, LG>; }
};
PXB_LANE_UNIT(ScrFamily, PXB_SCR_P)

}  // namespace ev
}  // namespace pxb

#if PXB_SCR_P == 1
#include "host_util.h"

namespace pxsc {
using namespace pxb::ev;
using namespace pxb::host;

// the extract: byte j of row i, a grid-stride loop over count * stride bytes
__global__ __launch_bounds__(256) void paxos_extract_kernel(EvParams p, uint32_t P, uint32_t N, uint32_t depth,
                                                            const uint64_t* ids, uint64_t count, uint64_t stride,
                                                            uint8_t* rows) {
  const uint64_t total = count * stride, step = (uint64_t)gridDim.x * 256u;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += step) {
    const uint64_t i = t / stride, j = t - i * stride;
    rows[t] = script_row_byte(p, P, N, depth, ids[i], j);
  }
}

// the scan's input: what the selection keeps of a row's in-window records
struct Kept {
  uint32_t tail;
  __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& c) const { return trace_kept(c, tail); }
};
typedef hipcub::TransformInputIterator<uint64_t, Kept, const uint32_t*> kept_iter;

// the argument rules every call shares
static int validate_cfg(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth) {
  if (!cfg || (count && !rows) || count > MAX_COUNT || depth > PXB_SCRIPT_MAX_DEPTH) return PXB_E_INVAL;
  if (!trace_config_ok(cfg)) return PXB_E_INVAL;
  return PXB_OK;
}
static int pick(const pxb_config* cfg, scr_ptr* fn) {
  *fn = lane_kernel<ScrFamily>(cfg);
  return *fn ? PXB_OK : PXB_E_INVAL;
}
static int validate_trace(const pxb_config* cfg, const void* rows, uint64_t count, uint32_t depth,
                          const pxb_trace_sel* sel, const void* records, uint64_t capacity, const void* offsets,
                          scr_ptr* fn) {
  if (int rc = validate_cfg(cfg, rows, count, depth)) return rc;
  if (!offsets || (sel && sel->reserved != 0u) || (!records && capacity)) return PXB_E_INVAL;
  if (cfg->flags & PXB_CFG_TRACE_PRODUCTION) return PXB_E_INVAL;
  return pick(cfg, fn);
}

static ScrParams params(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth) {
  ScrParams k{};
  k.p = make_params(cfg);
  k.p.first_instance = 0;
  k.rows = d_rows;
  k.stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  k.count = count;
  k.depth = depth;
  return k;
}

static hipError_t scan_bytes(uint64_t count, hipStream_t st, size_t* need) {
  *need = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *need, kept_iter(nullptr, Kept{0u}), (uint64_t*)nullptr,
                                          (int64_t)(count + 1), st);
}

}  // namespace pxsc

extern "C" {

uint64_t pxb_script_stride(uint32_t n_proposers, uint32_t n_acceptors, uint32_t depth) {
  return pxb::ev::script_stride(n_proposers, n_acceptors, depth);
}

int pxb_schedule_extract_device(const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, uint32_t depth,
                                uint8_t* d_rows, void* stream) {
  using namespace pxsc;
  if (int rc = validate_cfg(cfg, d_ids, count, depth)) return rc;
  if ((count && !d_rows) || ((uintptr_t)d_ids & 7u) || ((uintptr_t)d_rows & 7u)) return PXB_E_INVAL;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;
  const uint64_t stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  const uint64_t blocks = (count * stride + 255u) / 256u;
  const dim3 grid((unsigned)(blocks < (1ull << 20) ? blocks : (1ull << 20)));
  EvParams p = make_params(cfg);
  p.first_instance = 0;
  hipLaunchKernelGGL(paxos_extract_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, cfg->n_proposers,
                     cfg->n_acceptors, depth, d_ids, count, stride, d_rows);
  const hipError_t e = hipGetLastError();
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

int pxb_run_scripted_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                            pxb_result* d_out, uint32_t* d_log_digest, pxb_acceptor_rec* d_acc,
                            uint32_t* d_status, uint16_t* d_sent, void* stream) {
  using namespace pxsc;
  scr_ptr fn = nullptr;
  if (int rc = validate_cfg(cfg, d_rows, count, depth)) return rc;
  if (int rc = pick(cfg, &fn)) return rc;
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_log_digest & 3u) ||
      ((uintptr_t)d_acc & 15u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_sent & 1u))
    return PXB_E_INVAL;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) return PXB_OK;
  ScrParams k = params(cfg, d_rows, count, depth);
  k.smin = 1u;                      // (an empty window: no records are counted)
  k.smax = 0u;
  k.status = d_status;
  k.res = reinterpret_cast<uint4*>(d_out);
  k.digest = d_log_digest;
  k.acc = reinterpret_cast<uint4*>(d_acc);
  k.sent = d_sent;
  hipLaunchKernelGGL(fn, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, (hipStream_t)stream, k);
  const hipError_t e = hipGetLastError();
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

int pxb_trace_scripted_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                              const pxb_trace_sel* sel, pxb_trace_step* d_records, uint64_t capacity,
                              uint64_t* d_offsets, uint32_t* d_status, pxb_result* d_results, void* stream) {
  using namespace pxsc;
  scr_ptr fn = nullptr;
  if (int rc = validate_trace(cfg, d_rows, count, depth, sel, d_records, capacity, d_offsets, &fn)) return rc;
  // (the records move as 4-byte words, the results as 16-byte ones)
  if (((uintptr_t)d_rows & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_records & 3u) ||
      ((uintptr_t)d_status & 3u) || ((uintptr_t)d_results & 15u))
    return PXB_E_INVAL;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  if (count == 0) {
    const hipError_t e = hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), st);
    return (e == hipSuccess) ? PXB_OK : hip_fail(e);
  }
  size_t need = 0;
  if (hipError_t e = scan_bytes(count, st, &need)) return hip_fail(e);
  const size_t cnt_b = pad256((count + 1) * sizeof(uint32_t));
  void* buf = nullptr;
  if (int rc = pxw::scratch(dev, cnt_b + need, st, &buf)) return rc;
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(buf);
  ScrParams k = params(cfg, d_rows, count, depth);
  k.smin = sel ? sel->step_min : 0u;
  k.smax = sel ? sel->step_max : 0xFFFFFFFFu;
  k.tail = sel ? sel->tail : 0u;
  k.cnt = cnt;
  k.offsets = d_offsets;
  k.capacity = capacity;
  const dim3 grid((unsigned)((count + 63) / 64));
  hipError_t e = hipSuccess;
  do {
    if ((e = hipMemsetAsync(cnt + count, 0, sizeof(uint32_t), st)) != hipSuccess) break;
    k.status = d_status;
    k.res = reinterpret_cast<uint4*>(d_results);
    hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess) break;
    e = hipcub::DeviceScan::ExclusiveSum(reinterpret_cast<char*>(buf) + cnt_b, need,
                                         kept_iter(cnt, Kept{k.tail}), d_offsets, (int64_t)(count + 1), st);
    if (e != hipSuccess) break;
    if (capacity && d_records) {
      k.out = d_records;
      k.status = nullptr;
      k.res = nullptr;
      hipLaunchKernelGGL(fn, grid, dim3(64), 0, st, k);
      e = hipGetLastError();
    }
  } while (0);
  const hipError_t f = hipFreeAsync(buf, st);     // (stream-ordered: after the launches above)
  if (e == hipSuccess) e = f;
  return (e == hipSuccess) ? PXB_OK : hip_fail(e);
}

// ---- HOST-buffer forms: device copies of the buffers (host_stage.h) around the device forms ----
int pxb_schedule_extract(const pxb_config* cfg, const uint64_t* ids, uint64_t count, uint32_t depth, uint8_t* rows) {
  using namespace pxsc;
  if (int rc = validate_cfg(cfg, ids, count, depth)) return rc;
  if (count && !rows) return PXB_E_INVAL;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) return PXB_OK;
  pxb::StagePlan plan;
  const pxb::StageRegion r_ids = plan.add(sizeof(uint64_t), count);
  const pxb::StageRegion r_rows = plan.add(script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count);
  Staging S(plan);
  S.up(r_ids, ids, count);
  if (S.ok())
    S.note(pxb_schedule_extract_device(cfg, S.ptr<uint64_t>(r_ids), count, depth, S.ptr<uint8_t>(r_rows), nullptr));
  S.down(r_rows, rows, count);
  return S.finish();
}

int pxb_run_scripted(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth, pxb_result* out,
                     uint32_t* log_digest, pxb_acceptor_rec* acc, uint32_t* status, uint16_t* sent) {
  using namespace pxsc;
  if (int rc = validate_cfg(cfg, rows, count, depth)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  if (count == 0) return PXB_OK;
  const uint64_t P = cfg->n_proposers, N = cfg->n_acceptors;
  pxb::StagePlan plan;                            // rows | results | digests | records | status | sent
  const pxb::StageRegion r_rows = plan.add(script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count);
  const pxb::StageRegion r_out = plan.add(sizeof(pxb_result), count), r_dig = plan.add(N * sizeof(uint32_t), count);
  const pxb::StageRegion r_acc = plan.add(N * sizeof(pxb_acceptor_rec), count), r_st = plan.add(sizeof(uint32_t), count);
  const pxb::StageRegion r_sent = plan.add(2u * P * N * sizeof(uint16_t), count);
  Staging S(plan);
  S.up(r_rows, rows, count);
  // (an output that was not asked for: null, and the kernel does not store it)
  if (S.ok())
    S.note(pxb_run_scripted_device(cfg, S.ptr<uint8_t>(r_rows), count, depth, S.ptr<pxb_result>(r_out, out),
                                   S.ptr<uint32_t>(r_dig, log_digest), S.ptr<pxb_acceptor_rec>(r_acc, acc),
                                   S.ptr<uint32_t>(r_st, status), S.ptr<uint16_t>(r_sent, sent), nullptr));
  S.down(r_out, out, count);
  S.down(r_dig, log_digest, count);
  S.down(r_acc, acc, count);
  S.down(r_st, status, count);
  S.down(r_sent, sent, count);
  return S.finish();
}

int pxb_trace_scripted(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                       const pxb_trace_sel* sel, pxb_trace_step* records, uint64_t capacity, uint64_t* offsets,
                       uint32_t* status, pxb_result* results, uint64_t* n_records) {
  using namespace pxsc;
  scr_ptr fn = nullptr;
  if (int rc = validate_trace(cfg, rows, count, depth, sel, records, capacity, offsets, &fn)) return rc;
  if (device_count() == 0) return PXB_E_NODEV;
  // (both calls get the status and results buffers, whatever the caller asked for)
  const auto call = [&](Staging&, const TraceBufs& d, pxb_trace_step* d_rec = nullptr, uint64_t m = 0) {
    return pxb_trace_scripted_device(cfg, static_cast<uint8_t*>(d.in), count, depth, sel, d_rec, m, d.off, d.st, d.res,
                                     nullptr);
  };
  pxb::StagePlan plan;                            // rows | offsets | status | results
  return trace_two_call(plan, rows, script_stride(cfg->n_proposers, cfg->n_acceptors, depth), count, records, capacity,
                        offsets, status, results, n_records, call, call);
}

}  // extern "C"
#endif  // PXB_SCR_P == 1
