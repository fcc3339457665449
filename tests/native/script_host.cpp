// script_host.cpp — TEST ONLY: the scripted lane (cloud-haskell-paxos_amd/csrc/
// script_core.h: ScriptDraws, script_begin, script_sent over the per-lane state
// machine and TraceLane) and the extract's per-entry function on the host, one
// row at a time, so tests/test_script_host.py can check them against the Python
// reference model without a GPU.  The product runs the same code on the device
// (paxos_script.hip); nothing here is linked into libpaxos_batch.so.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../cloud-haskell-paxos_amd/csrc/lane_shapes.h"
#include "../../cloud-haskell-paxos_amd/csrc/script_lane.h"
#include "host_lane.h"

using namespace pxb;
using namespace pxb::ev;

// the header's row layout is the one the lane code reads
static_assert(sizeof(pxb_script_head) == SCR_HDR && PXB_SCRIPT_WINDOWS_OFF == SCR_HDR && sizeof(pxb_script_window) == 4,
              "row head");
static_assert(offsetof(pxb_script_head, n_proposers) == 8 && offsetof(pxb_script_head, reserved) == 9 &&
                  offsetof(pxb_script_head, skew) == 10,
              "row head fields");

namespace {

// one row's outputs (every pointer nullable but status)
struct Args {
  const pxb_config* cfg;
  const uint8_t* row;
  uint32_t depth;
  uint32_t smin, smax, tail;
  pxb_trace_step* records;
  uint64_t capacity;
  uint32_t* n_window;
  uint32_t* n_kept;
  uint32_t* status;
  pxb_result* result;
  uint32_t* digest;
  pxb_acceptor_rec* acc;
  uint16_t* sent;
};

// what one lane of paxos_script_kernel does for its row: the count pass with its
// outputs, then (records kept and room for some) the write pass from offset 0
// (spelled out here as in the kernel: paxos_script.hip says why it is not shared)
template <int PM, int N, int W, bool LG>
int run_shape(const Args& a) {
  using Lane = typename ScriptLane<PM, N, W, LG, HostMem, ScriptDraws>::Lane;
  EvParams p = make_params(a.cfg);
  p.first_instance = 0;
  HostLane<Lane> H(p);
  Lane& L = H.L;
  TraceLane<Lane> T;
  const uint64_t guard_max = 100000ull * a.cfg->step_cap;   // a hang is a test failure
  uint64_t guard = 0;
  T.begin_count(a.smin, a.smax);
  const uint32_t st = script_begin(L, p, a.depth, a.row);
  if (st != PXB_TRACE_OK) {
    T.status = st;
  } else {
    while (T.iter(L, p))
      if (++guard > guard_max) return -100;
  }
  const uint32_t cnt = T.n, kept = trace_kept(cnt, a.tail);
  const bool ok = T.status == PXB_TRACE_OK;
  if (a.n_window) *a.n_window = cnt;
  if (a.n_kept) *a.n_kept = kept;
  *a.status = T.status;
  if (a.result) memcpy(a.result, T.res, 16);
  for (int q = 0; q < N; ++q) {
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    if (ok) L.record_of(q, r);
    if (a.digest) a.digest[q] = ok ? L.digest_of(q) : 0u;
    if (a.acc) memcpy(a.acc + q, r, 16);
  }
  if (a.sent) {
    if (ok) script_sent(L, a.sent);
    else memset(a.sent, 0, 2u * PM * N * sizeof(uint16_t));
  }
  if (kept == 0u || a.capacity == 0u || !a.records) return 0;
  std::fill(H.buf.begin(), H.buf.end(), 0xDEADBEEFu);
  T.begin_write(a.smin, a.smax, cnt, a.tail, a.records, a.capacity);
  if (script_begin(L, p, a.depth, a.row) != PXB_TRACE_OK) return -101;
  guard = 0;
  while (T.iter(L, p))
    if (++guard > guard_max) return -100;
  return 0;
}

#ifdef PXB_SCRIPT_HOST_MAIN
// (the sanitizer build: one shape, config 3's)
int dispatch(const Args& a) {
  const pxb_config* c = a.cfg;
  if (c->n_proposers != 2 || c->n_acceptors != 5 || wheel_for(c->delay_max) != 8 || c->n_ticks > 1) return -1;
  return run_shape<2, 5, 8, false>(a);
}
#else
// (the shapes of lane_shapes.h; -1: none)
struct Run {
  const Args& a;
  template <int PM, int N, int W, bool LG>
  int run() const { return run_shape<PM, N, W, LG>(a); }
};
int dispatch(const Args& a) { return host_lane_shape(a.cfg, Run{a}, -1); }
#endif

}  // namespace

extern "C" uint64_t script_host_stride(uint32_t P, uint32_t N, uint32_t depth) { return script_stride(P, N, depth); }

// pxb_schedule_extract on the host: the per-entry function over every byte
extern "C" int script_host_extract(const pxb_config* cfg, const uint64_t* ids, uint64_t count, uint32_t depth,
                                   uint8_t* rows) {
  if (!cfg || !trace_config_ok(cfg) || depth > PXB_SCRIPT_MAX_DEPTH) return -1;
  EvParams p = make_params(cfg);
  p.first_instance = 0;
  const uint64_t stride = script_stride(cfg->n_proposers, cfg->n_acceptors, depth);
  for (uint64_t i = 0; i < count; ++i)
    for (uint64_t j = 0; j < stride; ++j)
      rows[i * stride + j] = script_row_byte(p, cfg->n_proposers, cfg->n_acceptors, depth, ids[i], j);
  return 0;
}

// `count` rows as pxb_run_scripted / pxb_trace_scripted run them, except that
// every row has its own record buffer: row i's kept records go to
// records[i * capacity ...] (nothing at or past `capacity` of them is written);
// n_window[i] = its visited steps inside the window, n_kept[i] = those the tail
// keeps (what its d_offsets entry grows by).  Outputs are nullable but status.
extern "C" int script_host_run(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                               const pxb_trace_sel* sel, pxb_trace_step* records, uint64_t capacity,
                               uint32_t* n_window, uint32_t* n_kept, uint32_t* status, pxb_result* results,
                               uint32_t* digest, pxb_acceptor_rec* acc, uint16_t* sent) {
  if (!cfg || !status || !trace_config_ok(cfg) || (sel && sel->reserved) || depth > PXB_SCRIPT_MAX_DEPTH ||
      (cfg->flags & PXB_CFG_TRACE_PRODUCTION))
    return -1;
  const uint32_t P = cfg->n_proposers, N = cfg->n_acceptors;
  const uint64_t stride = script_stride(P, N, depth);
  for (uint64_t i = 0; i < count; ++i) {
    Args a{cfg, rows + i * stride, depth, sel ? sel->step_min : 0u, sel ? sel->step_max : 0xFFFFFFFFu,
           sel ? sel->tail : 0u, records ? records + i * capacity : nullptr, capacity,
           n_window ? n_window + i : nullptr, n_kept ? n_kept + i : nullptr, status + i,
           results ? results + i : nullptr, digest ? digest + i * N : nullptr, acc ? acc + i * N : nullptr,
           sent ? sent + i * 2u * P * N : nullptr};
    if (int rc = dispatch(a)) return rc;
  }
  return 0;
}

#ifdef PXB_SCRIPT_HOST_MAIN
// Sanitizer-build driver (tests/test_script_host.py): n rows of config 3's shape,
// extracted for ids first .. first + n - 1 at `depth` and then overridden at
// random (about 10 % of the link entries: lost, or a delay in 1 .. delay_max + 3;
// some skews, windows and proposer counts), run with one selection.  Every
// buffer holds exactly what the call may write (so that the sanitizer sees a
// write past it).  To a file of raw bytes: the rows, then per row little-endian
// words n_window, n_kept, status, result x 4, digest x N, acceptor records,
// sent (halfwords, padded to a word), then the written records.
// argv: out seed first n depth rng loss delay skew cap step_min step_max tail capacity
int main(int argc, char** argv) {
  if (argc != 15) {
    fprintf(stderr, "usage: %s out seed first n depth rng loss delay skew cap step_min step_max tail capacity\n", argv[0]);
    return 2;
  }
  pxb_config c{};
  c.seed = strtoull(argv[2], nullptr, 0);
  const uint64_t first = strtoull(argv[3], nullptr, 0), n = strtoull(argv[4], nullptr, 0);
  const uint32_t depth = (uint32_t)strtoul(argv[5], nullptr, 0);
  uint64_t rng = strtoull(argv[6], nullptr, 0);
  c.n_proposers = 2;
  c.n_acceptors = 5;
  c.n_ticks = 1;
  c.tick_period = 1;
  c.crash_len_max = 1;
  uint32_t* f[] = {&c.loss_ppm, &c.delay_max, &c.skew_max, &c.step_cap};
  for (int i = 0; i < 4; ++i) *f[i] = (uint32_t)strtoul(argv[7 + i], nullptr, 0);
  pxb_trace_sel sel{(uint32_t)strtoul(argv[11], nullptr, 0), (uint32_t)strtoul(argv[12], nullptr, 0),
                    (uint32_t)strtoul(argv[13], nullptr, 0), 0u};
  const uint64_t capacity = strtoull(argv[14], nullptr, 0);
  const uint32_t P = 2, N = 5;
  const uint64_t stride = script_stride(P, N, depth);
  auto next = [&rng]() {                                   // (a 64-bit LCG's high word)
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  };
  std::vector<uint64_t> ids(n);
  for (uint64_t g = 0; g < n; ++g) ids[g] = first + g;
  std::vector<uint8_t> rows(n * stride);                   // exactly the rows
  if (script_host_extract(&c, ids.data(), n, depth, rows.data()) != 0) return 4;
  for (uint64_t g = 0; g < n; ++g) {
    uint8_t* r = rows.data() + g * stride;
    uint8_t* lk = r + script_links_off(N);
    for (uint64_t e = 0; e < script_links_bytes(P, N, depth); ++e)
      if (next() % 10u == 0u) lk[e] = (next() % 4u == 0u) ? 0u : (uint8_t)(1u + next() % (c.delay_max + 3u));
    if (next() % 4u == 0u) r[8] = (uint8_t)(1u + next() % P);
    if (next() % 4u == 0u) r[10 + 2 * (next() % 3u)] = (uint8_t)(next() % 6u);
    if (next() % 4u == 0u) {
      uint8_t* w = r + SCR_HDR + 4u * (next() % N);
      const uint32_t c0 = next() % 12u, c1 = c0 + next() % 10u;
      w[0] = (uint8_t)c0, w[1] = 0u, w[2] = (uint8_t)c1, w[3] = 0u;
    }
  }
  FILE* o = fopen(argv[1], "wb");
  if (!o) return 3;
  fwrite(rows.data(), 1, rows.size(), o);
  std::vector<pxb_trace_step> rec(n * capacity);           // exactly `capacity` entries per row
  std::vector<uint32_t> nw(n), nk(n), st(n), dig(n * N);
  std::vector<pxb_result> res(n);
  std::vector<pxb_acceptor_rec> acc(n * N);
  std::vector<uint16_t> sent(n * 2u * P * N);
  const int rc = script_host_run(&c, rows.data(), n, depth, &sel, rec.data(), capacity, nw.data(), nk.data(),
                                 st.data(), res.data(), dig.data(), acc.data(), sent.data());
  if (rc != 0) {
    fclose(o);
    return 4;
  }
  for (uint64_t g = 0; g < n; ++g) {
    const uint32_t hdr[3] = {nw[g], nk[g], st[g]};
    fwrite(hdr, 4, 3, o);
    fwrite(&res[g], 16, 1, o);
    fwrite(&dig[g * N], 4, N, o);
    fwrite(&acc[g * N], 16, N, o);
    fwrite(&sent[g * 2u * P * N], 2, 2u * P * N, o);
    const uint64_t m = nk[g] < capacity ? nk[g] : capacity;
    fwrite(rec.data() + g * capacity, sizeof(pxb_trace_step), m, o);
  }
  fclose(o);
  return 0;
}
#endif
