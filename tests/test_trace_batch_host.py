"""The batched trace (pxb_trace_batch) without a GPU.

The per-lane core the kernel runs (csrc/paxos_trace_core.h: TraceLane with its
window, tail and capacity logic, and trace_record) is compiled for the HOST
(tests/native/trace_host.cpp) over the per-lane state machine and diffed step by
step against the Python reference model (oracle/paxos_ref.py), by the rules of
tests/test_gpu_parity.py::test_trace_matches_oracle_steps.  Then the C-ABI
boundary of the new entry points (struct size, symbols, every PXB_E_INVAL case,
PXB_E_NODEV), and one stand-alone AddressSanitizer + UBSan program (its own
main; nothing is loaded into Python)."""
import ctypes as C
import dataclasses
import os
import subprocess
import tempfile

import numpy as np
import pytest

import paxos_ref as R
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "trace_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libtrace_host.so")
EXE = os.path.join(HERE, "native", "_build", "trace_host_san")
DEPS = [SRC, os.path.join(HERE, "native", "host_lane.h")] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "paxos_trace_core.h", "ev_layouts.h",
              "lane_shapes.h")] + [os.path.join(ROOT, "include", "paxos_batch.h")]
HIPCC = "/opt/rocm/bin/hipcc"
U32 = 0xFFFFFFFF
SELECTIONS = [(0, U32, 0), (10, 40, 0), (0, U32, 1), (5, 5, 0), (7, 3, 0), (20, 200, 3)]
IDS = list(range(64)) + list(range((1 << 32) - 32, (1 << 32) + 32))
_lib = None


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def lib():
    global _lib
    if _lib is None:
        if _stale(OUT):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", tmp, SRC],
                           check=True, timeout=900)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
    return _lib


def host_trace(cfg, inst, sel=None, capacity=4200, production=False, pad=0):
    """One instance through the host build of the batched trace's lane: (rows
    uint32 (capacity + pad, TRACE_WORDS) sentinel-filled, n_window, n_kept,
    status, result)."""
    rec = np.full((capacity + pad, pxb.TRACE_WORDS), 0xA5A5A5A5, dtype=np.uint32)
    nw, nk, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    res = np.zeros(4, np.uint32)
    c = cfg.to_c(0, 1)
    if production:
        c.flags |= pxb.CFG_TRACE_PRODUCTION
    s = pxb.pxb_trace_sel(*sel, 0) if sel is not None else None
    f = lib().trace_host_run
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p]
    rc = f(C.addressof(c), inst, C.addressof(s) if s is not None else None, rec.ctypes.data, capacity,
           C.addressof(nw), C.addressof(nk), C.addressof(st), res.ctypes.data)
    assert rc == 0, "trace_host_run rc=%d" % rc
    return rec, nw.value, nk.value, st.value, res


def _digest(log):
    h = R.FNV_BASIS
    for v in log:
        h = R.fnv1a_u32(h, v)
    return R.fnv1a_u32(h, len(log))


def oracle_trace(cfg, inst):
    recs = []

    def snap(s, accs, props, in_flight):
        recs.append({"step": s, "in_flight": in_flight,
                     "acc": [(a.t_max, a.t_store, a.val, len(a.log) | (int(a.dead) << 31)) for a in accs],
                     "digest": [_digest(a.log) for a in accs],
                     "prop": [(p.ticket, p.cmd, p.acks, p.rs, p.mr_t, p.mr_v, p.r2_v, int(p.pending))
                              for p in props]})
    res = R.run_instance(R.Config(**cfg.__dict__), inst, trace=snap)
    return recs, res


def as_rec(g):
    return {"step": g["step"], "in_flight": g["in_flight"],
            "acc": [tuple(int(x) for x in r) for r in g["acc"]], "digest": [int(x) for x in g["digest"]],
            "prop": [tuple(int(x) for x in r) for r in g["prop"]]}


def check_against_oracle(g, gres, cfg, inst):
    """test_trace_matches_oracle_steps' rules: every recorded step equals the
    oracle's end-of-step state; the steps it skips change nothing."""
    want, res = oracle_trace(cfg, inst)
    keys = ("acc", "digest", "prop", "in_flight")
    prev = None
    gi = iter(as_rec(x) for x in g)
    cur = next(gi)
    for r in want:
        if cur is not None and r["step"] == cur["step"]:
            assert r == cur, "instance %d step %d: oracle %s host %s" % (inst, r["step"], r, cur)
            prev, cur = cur, next(gi, None)
        else:                                          # a skipped step: nothing changed
            assert prev is not None and {k: r[k] for k in keys} == {k: prev[k] for k in keys}, (inst, r["step"])
    assert cur is None and g[-1]["step"] == want[-1]["step"]
    assert list(gres) == [res.decided_val, res.decided_ticket, res.rounds, res.packed_flags()]


@pytest.mark.parametrize("c", [3, 4, 5, 7])
def test_host_core_matches_oracle_steps(c):
    """Every record of every instance (ids 0..63 and 2^32 - 32 .. 2^32 + 31)
    equals the reference model's state at the end of that step, and the result
    its result; instances beyond the link capacities (BAILED: no records, a
    zeroed result) stay within tests/test_ev_host.py's 2 %."""
    cfg = pxb.CONFIGS[c]
    bailed = 0
    for inst in IDS:
        rec, nw, nk, st, res = host_trace(cfg, inst)
        if st == pxb.TRACE_BAILED:
            assert nw == 0 and nk == 0 and not res.any() and (rec == 0xA5A5A5A5).all()
            bailed += 1
            continue
        assert st == pxb.TRACE_OK and nw == nk and 0 < nk <= 4200
        assert (rec[nk:] == 0xA5A5A5A5).all()
        check_against_oracle(pxb.trace_records(rec[:nk]), res, cfg, inst)
    assert bailed <= 0.02 * len(IDS) + 1


def test_host_core_records_the_last_visited_step_of_a_capped_instance():
    """Config 3, id 33 ends at the step cap (256) from step 253: its next
    message falls due past the cap.  Steps 253 and 255 are both recorded, with
    the same state, so the step in which the final state was reached is told
    (the oracle changes state at 253; 254 and 255 change nothing)."""
    cfg = pxb.CONFIGS[3]
    rec, nw, nk, st, res = host_trace(cfg, 33)
    assert st == pxb.TRACE_OK and int(res[3]) & pxb.F_STEP_CAP
    assert [int(r[0]) for r in rec[nk - 3:nk]] == [252, 253, 255]
    assert (rec[nk - 2][1:] == rec[nk - 1][1:]).all() and (rec[nk - 3][1:] != rec[nk - 2][1:]).any()
    # the window sees them as two records: a tail of 2 is 253 and 255, [253, 254] keeps one
    r2, _, nk2, _, _ = host_trace(cfg, 33, sel=(0, U32, 2))
    assert nk2 == 2 and (r2[:2] == rec[nk - 2:nk]).all()
    r1, _, nk1, _, _ = host_trace(cfg, 33, sel=(253, 254, 0))
    assert nk1 == 1 and (r1[0] == rec[nk - 2]).all()
    # (the production variant carries step 253's last copies into 254 and ends from there)
    full, _, nk0, _, _ = host_trace(cfg, 33, production=True)
    steps = [int(r[0]) for r in full[:nk0]]
    assert steps[-1] == 255 and 253 in steps and steps == sorted(set(steps))


def select(full, sel):
    smin, smax, tail = sel
    rows = [r for r in full if smin <= int(r[0]) <= smax]
    return rows[-tail:] if tail else rows


@pytest.mark.parametrize("production", [False, True])
@pytest.mark.parametrize("sel", SELECTIONS)
def test_host_core_selection(sel, production):
    """Window and tail alone: what a selection keeps equals the Python selection
    from the instance's full record list (both variants: the production one
    counts a rewritten last record once); with tail = 1 the one record is the
    final step's, PXB_RESULT_STEPS - 1."""
    cfg = pxb.CONFIGS[3]
    seen = 0
    for inst in list(range(40)) + [(1 << 32) - 1, 1 << 32]:
        full, nw0, nk0, st0, res0 = host_trace(cfg, inst, production=production)
        if st0 == pxb.TRACE_BAILED:
            continue
        want = select(full[:nk0], sel)
        rec, nw, nk, st, res = host_trace(cfg, inst, sel=sel, production=production)
        assert st == pxb.TRACE_OK and (res == res0).all()
        assert nk == len(want) and nw == len(select(full[:nk0], (sel[0], sel[1], 0)))
        assert (rec[nk:] == 0xA5A5A5A5).all()
        if want:
            assert (rec[:nk] == np.array(want)).all(), inst
        if sel == (0, U32, 1):
            assert nk == 1 and int(rec[0][0]) == (int(res[3]) >> 16) - 1
        if sel == (7, 3, 0):
            assert nk == 0
        seen += 1
    assert seen >= 40


def test_host_core_production_counts_rewrite_once():
    """The production variant's step list is strictly ascending (the record it
    takes again at the end replaces the first one), and its final record is the
    result's last step, as in pxb_trace_instance."""
    cfg = pxb.CONFIGS[3]
    for inst in range(64):
        rec, nw, nk, st, res = host_trace(cfg, inst, production=True)
        if st == pxb.TRACE_BAILED:
            continue
        steps = [int(r[0]) for r in rec[:nk]]
        assert steps == sorted(set(steps)) and steps[-1] == (int(res[3]) >> 16) - 1


@pytest.mark.parametrize("sel", [(0, U32, 0), (20, 200, 3)])
def test_host_core_capacity(sel):
    """Records at or past the capacity are counted and not written: the first
    `capacity` kept records are there, every sentinel behind them is intact and
    the counts are the full ones."""
    cfg = pxb.CONFIGS[3]
    for inst in range(24):
        full, _, nk0, st0, _ = host_trace(cfg, inst, sel=sel)
        if st0 == pxb.TRACE_BAILED or nk0 < 2:
            continue
        for cap in (0, 1, nk0 // 2, nk0 - 1):
            rec, nw, nk, st, _ = host_trace(cfg, inst, sel=sel, capacity=cap, pad=8)
            assert nk == nk0 and (rec[:cap] == full[:cap]).all() and (rec[cap:] == 0xA5A5A5A5).all()


# ---- the C-ABI boundary ---------------------------------------------------------
def test_trace_sel_layout_and_symbols(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "paxos_batch.h"
int main(void) {
  printf("%zu %zu %zu %zu %u %u\n", sizeof(pxb_trace_sel), offsetof(pxb_trace_sel, step_max),
         offsetof(pxb_trace_sel, tail), offsetof(pxb_trace_sel, reserved), PXB_TRACE_OK, PXB_TRACE_BAILED);
  return 0;
}'''
    tmp = str(tmp_path / "pxb_sel_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True).stdout.split()]
    assert got == [16, 4, 8, 12, pxb.TRACE_OK, pxb.TRACE_BAILED]
    assert C.sizeof(pxb.pxb_trace_sel) == 16
    assert "#define PXB_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "paxos_batch.h")).read()
    lib_ = pxb.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_trace_batch", "pxb_trace_batch_device"):
        assert " T %s\n" % name in out and hasattr(lib_, name)


def test_trace_batch_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call (so on every
    host); a valid call is PXB_E_NODEV without a GPU."""
    import torch
    L = pxb.load()
    ids = np.arange(8, dtype=np.uint64)
    offs = np.zeros(9, np.uint64)
    rec = np.zeros((4, pxb.TRACE_WORDS), np.uint32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def both(cfg, ids_p, count, sel, rec_p, cap, offs_p):
        c = cfg.to_c(0, 1) if cfg is not None else None
        cp = C.byref(c) if c is not None else None
        sp = C.byref(sel) if sel is not None else None
        return (L.pxb_trace_batch(cp, ids_p, count, sp, rec_p, cap, offs_p, None, None, None),
                L.pxb_trace_batch_device(cp, ids_p, count, sp, rec_p, cap, offs_p, None, None, None))
    cfg = pxb.CONFIGS[3]
    inval = (pxb.PXB_E_INVAL, pxb.PXB_E_INVAL)
    assert both(None, P(ids), 8, None, None, 0, P(offs)) == inval                 # null cfg
    assert both(cfg, P(ids), 8, None, None, 0, None) == inval                     # null offsets
    assert both(cfg, None, 8, None, None, 0, P(offs)) == inval                    # null ids, count > 0
    assert both(cfg, P(ids), (1 << 30) + 1, None, None, 0, P(offs)) == inval      # count > 2^30
    assert both(cfg, P(ids), 8, pxb.pxb_trace_sel(0, U32, 0, 1), None, 0, P(offs)) == inval   # reserved
    assert both(cfg, P(ids), 8, None, None, 4, P(offs)) == inval                  # no records, capacity > 0
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0),
                dataclasses.replace(cfg, step_cap=4096),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, tick_period=0),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, n_ticks=4097)):
        assert both(bad, P(ids), 8, None, P(rec), 4, P(offs)) == inval, bad
    if not torch.cuda.is_available():
        nodev = (pxb.PXB_E_NODEV, pxb.PXB_E_NODEV)
        assert both(cfg, P(ids), 8, None, P(rec), 4, P(offs)) == nodev
        assert both(cfg, P(ids), 8, pxb.pxb_trace_sel(3, 9, 2, 0), None, 0, P(offs)) == nodev
        assert both(pxb.LOG_FAULTY_CONFIG, P(ids), 8, None, None, 0, P(offs)) == nodev
        assert both(cfg, None, 0, None, None, 0, P(offs)) == nodev               # count == 0 is valid
        with pytest.raises(pxb.PaxosError):
            pxb.trace_batch(cfg, [1, 2, 3])


def test_trace_batch_device_checks_buffers_before_the_abi():
    """pxb.trace_batch_device hands raw addresses on: host tensors, short
    buffers and missing required ones raise first."""
    import torch
    cfg = pxb.CONFIGS[3]
    ids = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="required"):
        pxb.trace_batch_device(cfg, ids, 8, None)
    with pytest.raises(ValueError, match="CUDA"):
        pxb.trace_batch_device(cfg, ids, 8, torch.zeros(9, dtype=torch.int64))

    class Fake:   # a stand-in for a device tensor (no GPU here)
        def __init__(self, numel, size):
            self.is_cuda, self._n, self._s = True, numel, size
            self.dtype = torch.int32 if size == 4 else torch.int64

        def element_size(self):
            return self._s

        def is_contiguous(self):
            return True

        def numel(self):
            return self._n
    with pytest.raises(ValueError, match="needed"):
        pxb.trace_batch_device(cfg, Fake(8, 8), 8, Fake(8, 8))
    with pytest.raises(ValueError, match="needed"):
        pxb.trace_batch_device(cfg, Fake(8, 8), 8, Fake(9, 8), d_records=Fake(4 * pxb.TRACE_WORDS - 1, 4), capacity=4)
    with pytest.raises(ValueError, match="required"):
        pxb.trace_batch_device(cfg, Fake(8, 8), 8, Fake(9, 8), capacity=4)
    with pytest.raises(ValueError, match="integer"):
        pxb.trace_batch_device(cfg, Fake(8, 8), 8, Fake(9, 8), d_status=Fake(8, 8))


def test_trace_records_is_trace_instances_decode():
    """trace_records gives the dicts trace_instance always gave."""
    row = np.arange(pxb.TRACE_WORDS, dtype=np.uint32)
    row[2], row[3] = 5, 2
    (d,) = pxb.trace_records(row[None, :])
    assert d["step"] == 0 and d["in_flight"] == 1
    assert (d["acc"] == row[4:24].reshape(5, 4)).all() and (d["digest"] == row[40:45]).all()
    assert (d["prop"] == row[49:65].reshape(2, 8)).all()


# ---- one stand-alone sanitizer program --------------------------------------------
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_TRACE_HOST_MAIN",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
             "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_trace_core_sanitized():
    """trace_host.cpp with its own main (one shape: P = 2, N = 5, W = 8) under
    AddressSanitizer + UBSan, as a subprocess over config 3 ids 0..255 with a
    window and a tail and a capacity that cuts the kept records: every record
    buffer holds exactly `capacity` entries, so a write past it is a report.
    Exit status 0, and the output equals the unsanitized library's."""
    if _stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([HIPCC, *SAN_FLAGS, "-o", tmp, SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    cfg = pxb.CONFIGS[3]
    sel, cap, n = (4, 60, 5), 3, 256
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "o.bin")
        e = dict(os.environ)
        e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
        p = subprocess.run([EXE, out, hex(cfg.seed), "0", str(n), str(cfg.loss_ppm), str(cfg.delay_max),
                            str(cfg.skew_max), str(cfg.step_cap), "0", str(sel[0]), str(sel[1]), str(sel[2]), str(cap)],
                           capture_output=True, text=True, env=e, timeout=600)
        assert p.returncode == 0, "sanitized run failed (rc %d): %s" % (p.returncode, p.stderr[-4000:])
        w = np.fromfile(out, dtype=np.uint32)
    o = 0
    for inst in range(n):
        nw, nk, st = (int(x) for x in w[o:o + 3])
        res = w[o + 3:o + 7]
        m = min(nk, cap)
        rows = w[o + 7:o + 7 + m * pxb.TRACE_WORDS].reshape(m, pxb.TRACE_WORDS)
        o += 7 + m * pxb.TRACE_WORDS
        rec, nw1, nk1, st1, res1 = host_trace(cfg, inst, sel=sel, capacity=cap)
        assert (nw, nk, st) == (nw1, nk1, st1) and (res == res1).all() and (rows == rec[:m]).all(), inst
        assert nk <= 5
    assert o == len(w)
