// host_stage.h — what every HOST-buffer entry point shares: the error mapping
// that pxb_last_hip_error reads, and the staging of host buffers through one
// device allocation carved by a StagePlan (stage_plan.h).  No hipCUB in it:
// host_util.h adds that for the units whose entry points scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/paxos_batch.h"
#include "stage_plan.h"

namespace pxb {
namespace host {

// paxos_batch.hip: the calling thread's last failing HIP code (pxb_last_hip_error)
void set_last_hip_error(int e);

inline int hip_fail(hipError_t e) {
  set_last_hip_error((int)e);
  return (e == hipErrorOutOfMemory) ? PXB_E_OOM : PXB_E_HIP;
}

inline int hip_rc(hipError_t e) { return (e == hipSuccess) ? PXB_OK : hip_fail(e); }

inline int device_count() {
  int n = 0;
  return (hipGetDeviceCount(&n) != hipSuccess) ? 0 : n;
}

// One call's device copies.  It keeps the first failure it meets, a device
// form's code (note) or a HIP error, and every call after that is a no-op, so
// a form reads top to bottom with no ladder of breaks; finish() gives the
// form's code: the device form's first, then the HIP error's, then PXB_OK.
class Staging {
 public:
  explicit Staging(const StagePlan& plan) {
    if (!plan.valid) rc_ = PXB_E_INVAL;
    else if (plan.total) note(hipMalloc(&base_, (size_t)plan.total));
  }
  ~Staging() { (void)finish(); }
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;

  bool ok() const { return rc_ == PXB_OK && err_ == hipSuccess; }
  void note(int rc) { if (ok()) rc_ = rc; }
  void note(hipError_t e) { if (ok()) err_ = e; }
  void sync() { if (ok()) note(hipDeviceSynchronize()); }

  // the region's device pointer (an empty region's: null)
  template <class T>
  T* ptr(const StageRegion& r) const {
    char* const b = r.late ? late_ : base_;
    return (b && r.bytes()) ? reinterpret_cast<T*>(b + r.offset) : nullptr;
  }
  // the same for an optional output: null when the caller did not ask for it
  template <class T>
  T* ptr(const StageRegion& r, const void* wanted) const { return wanted ? ptr<T>(r) : nullptr; }

  // the first `count` elements of the region from / to a host buffer (null: nothing)
  void up(const StageRegion& r, const void* src, uint64_t count) { copy(r, const_cast<void*>(src), count, true); }
  void down(const StageRegion& r, void* dst, uint64_t count) { copy(r, dst, count, false); }
  void zero(const StageRegion& r) {
    if (ok() && r.bytes()) note(hipMemset(ptr<char>(r), 0, (size_t)r.bytes()));
  }
  // the one allocation sized after a first device call (a trace's records, the codec's bytes)
  StageRegion late(uint64_t elem, uint64_t count) {
    uint64_t bytes = 0;
    if (ok() && (late_ || __builtin_mul_overflow(elem, count, &bytes) || bytes > (uint64_t)SIZE_MAX)) rc_ = PXB_E_INVAL;
    if (ok() && bytes) note(hipMalloc(&late_, (size_t)bytes));
    return StageRegion{0, elem, ok() ? count : 0, true};
  }
  // waits for the device (also after a failure: nothing is freed under queued work), frees, and gives the call's code
  int finish() {
    if (base_ || late_) {
      note(hipDeviceSynchronize());
      if (late_) (void)hipFree(late_);
      if (base_) (void)hipFree(base_);
      base_ = late_ = nullptr;
    }
    return rc_ ? rc_ : hip_rc(err_);
  }

 private:
  void copy(const StageRegion& r, void* host, uint64_t count, bool up) {
    if (!ok() || !host || !count) return;
    const size_t bytes = (size_t)(count * r.elem);
    if (count > r.count) rc_ = PXB_E_INVAL;       // (a form's own mistake: never past the region)
    else note(up ? hipMemcpy(ptr<char>(r), host, bytes, hipMemcpyHostToDevice)
                 : hipMemcpy(host, ptr<char>(r), bytes, hipMemcpyDeviceToHost));
  }
  char* base_ = nullptr;
  char* late_ = nullptr;
  int rc_ = PXB_OK;
  hipError_t err_ = hipSuccess;
};

// The three tracing forms (pxb_trace_batch, _scripted, _events) after their
// argument checks: count == 0 answered on the host; else the input up, a sizing
// call, the offsets down, total = offsets[count] and m = min(total, capacity)
// records in a late allocation, the write call, the records and then status and
// results down.  The plan may already hold the caller's own regions.
// size(S, d) and write(S, d, d_records, m) return a PXB_* code or a hipError_t.
struct TraceBufs {                  // the device copies: input | offsets | status | results
  void* in;
  uint64_t* off;
  uint32_t* st;
  pxb_result* res;
};
template <class Rec, class Size, class Write>
int trace_two_call(StagePlan& plan, const void* in, uint64_t in_elem, uint64_t count, Rec* records, uint64_t capacity,
                   uint64_t* offsets, uint32_t* status, pxb_result* results, uint64_t* n_records, Size size,
                   Write write) {
  if (count == 0) {
    offsets[0] = 0;
    if (n_records) *n_records = 0;
    return PXB_OK;
  }
  const StageRegion r_in = plan.add(in_elem, count), r_off = plan.add(sizeof(uint64_t), count + 1);
  const StageRegion r_st = plan.add(sizeof(uint32_t), count), r_res = plan.add(sizeof(pxb_result), count);
  Staging S(plan);
  const TraceBufs d{S.ptr<void>(r_in), S.ptr<uint64_t>(r_off), S.ptr<uint32_t>(r_st), S.ptr<pxb_result>(r_res)};
  S.up(r_in, in, count);
  if (S.ok()) S.note(size(S, d));
  S.down(r_off, offsets, count + 1);
  if (!S.ok()) return S.finish();
  const uint64_t total = offsets[count], m = total < capacity ? total : capacity;
  if (m) {
    const StageRegion rec = S.late(sizeof(Rec), m);
    if (S.ok()) S.note(write(S, d, S.ptr<Rec>(rec), m));
    S.down(rec, records, m);
  }
  S.down(r_st, status, count);
  S.down(r_res, results, count);
  if (S.ok() && n_records) *n_records = total;
  return S.finish();
}

}  // namespace host
}  // namespace pxb
