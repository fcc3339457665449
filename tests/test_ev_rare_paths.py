"""The rarely-needed regions of the per-lane state machine's iteration
(csrc/paxos_ev.h): the decision bookkeeping behind its wave-level branch, the
acceptor word of an Execute at its own ticket selected inside the Execute
branch, the panic flag formed in finish() from the acceptors' dead bits, the
simple schedule's next step, and the bail flag as a per-iteration value.

The host build of EvLane (tests/native/ev_rare_host.cpp) runs pinned instances
one at a time on five shapes and every instance is compared with the CPU
oracle: result words, digests, rounds, executes, messages, canonical bytes,
and whether it is handed on.  The ids were chosen once with the same driver
over the first 20,000 instances of each config; each case the regions exist
for must be present, not only pass: an instance that decides, one that
restarts after its Execute (two broadcasts from one input), one that ends at
the step cap, one that ends quiet and undecided, one that panics, one handed
on with a full response FIFO and one with an empty pool.  The driver also
looks at the bail flag before every iteration: it is never set on entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_c
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ev_rare_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libev_rare_host.so")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")] + [
                    os.path.join(HERE, "..", "include", "paxos_batch.h")]
# a record's words (ev_rare_host.cpp)
(RW_RES, RW_ROUNDS, RW_EXECS, RW_MSGS, RW_CANON, RW_BAILED, RW_PROBES, RW_ITERS, RW_ENTRY_BAILED, RW_FLAGS, RW_STEPS,
 RW_TWO_BCAST, RW_BAIL_AT_INIT, RW_N) = (0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
# the header's probe bits (paxos_ev.h)
EVP_RUN, EVP_EXEC, EVP_RESTART, EVP_HIT = 1 << 2, 1 << 10, 1 << 11, 1 << 12
EVB_RING, EVB_RFIFO, EVB_POOL, EVB_QFIFO = 1 << 16, 1 << 17, 1 << 18, 1 << 19
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC",
                            "-shared", "-o", tmp, SRC], check=True)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
        assert _lib.ev_rare_words() == RW_N
    return _lib


LOG_CFG = pxb.Config(seed=0x1065, n_proposers=2, n_acceptors=5, loss_ppm=100000, delay_max=4, skew_max=3,
                     crash_ppm=200000, crash_len_max=12, crash_start_max=30, step_cap=1024, n_ticks=16, tick_period=4)
FIRST = list(range(96))
# config 5's instances drawn with three proposers: the two-proposer shape hands them on in init
P3_OF_FIRST = [1, 3, 6, 9, 15, 16, 19, 20, 22, 26, 28, 38, 39, 40, 41, 42, 43, 45, 46, 48, 53, 57, 59, 67, 73, 77, 78,
               79, 81, 82, 92, 93, 94]
# shape: layout, proposer capacity, config, ids beyond the first 96, the ids
# handed on, and one pinned id per case
SHAPES = {
    "tight": (7, 2, pxb.CONFIGS[4], [160, 246, 286, 369, 4524, 5133], [49, 67, 160, 246, 286, 369],
              dict(decides=1, restarts=0, capped=2, quiet_undecided=71, panics=33, full_rfifo=49, empty_pool=67)),
    "layout6": (6, 2, pxb.CONFIGS[4], [160, 246, 2770, 4524, 10705], [2770, 10705],
                dict(decides=1, restarts=0, capped=2, quiet_undecided=4524, panics=78, empty_pool=2770)),
    "slim_p2": (5, 2, pxb.CONFIGS[5], [235, 721, 2751, 3971], P3_OF_FIRST + [235, 721, 2751, 3971],
                dict(decides=0, restarts=4, capped=51, quiet_undecided=2, panics=7, full_rfifo=235, empty_pool=2751,
                     at_init=1)),
    "log_p2": (4, 2, LOG_CFG, [], [],
               dict(decides=1, restarts=0, quiet_undecided=13, panics=2)),
    "slim_p3": (5, 3, pxb.CONFIGS[5], [984, 2029, 2390, 2409], [984, 2029, 2390, 2409],
                dict(decides=3, restarts=4, capped=9, quiet_undecided=1, panics=0, empty_pool=2029, ring=984)),
}
_recs = {}


def records(shape):
    """The driver's records of the shape's ids, run once and left unchanged."""
    if shape not in _recs:
        layout, pm, cfg, extra, _, _ = SHAPES[shape]
        ids = np.asarray(FIRST + extra, np.uint32)
        rec = np.zeros((len(ids), RW_N + cfg.n_acceptors), np.uint32)
        c = cfg.to_c(0, 1 << 31)
        rc = lib().ev_rare_run(C.byref(c), layout, pm, C.c_void_p(ids.ctypes.data), len(ids),
                               C.c_void_p(rec.ctypes.data))
        assert rc == 0, "ev_rare_run rc=%d" % rc
        rec.setflags(write=False)
        _recs[shape] = ({int(g): rec[i] for i, g in enumerate(ids)}, [int(g) for g in ids])
    return _recs[shape]


def case_of(r):
    """The cases an instance's record shows."""
    f, pr = int(r[RW_FLAGS]), int(r[RW_PROBES])
    if r[RW_BAILED]:
        return {k for k, on in dict(at_init=r[RW_BAIL_AT_INIT], full_rfifo=pr & EVB_RFIFO, empty_pool=pr & EVB_POOL,
                                    ring=pr & EVB_RING, full_qfifo=pr & EVB_QFIFO).items() if on}
    return {k for k, on in dict(decides=not f & pxb.F_UNDECIDED, restarts=r[RW_TWO_BCAST] > 0,
                                capped=f & pxb.F_STEP_CAP,
                                quiet_undecided=(f & pxb.F_UNDECIDED) and not f & pxb.F_STEP_CAP,
                                panics=f & pxb.F_PANIC).items() if on}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_instance_matches_the_oracle(shape):
    _, _, cfg, _, handed_on, _ = SHAPES[shape]
    recs, ids = records(shape)
    N = cfg.n_acceptors
    assert sorted(g for g in ids if recs[g][RW_BAILED]) == sorted(handed_on)
    for g in ids:
        r = recs[g]
        if r[RW_BAILED]:
            continue
        eres, edig, _, cnt = oracle_c.run_cpu(cfg, g, 1)
        assert list(r[RW_RES:RW_RES + 4]) == list(eres[0]), "instance %d: result words" % g
        assert list(r[RW_N:RW_N + N]) == list(edig[0]), "instance %d: digests" % g
        got = dict(rounds=int(r[RW_ROUNDS]), executes=int(r[RW_EXECS]), messages=int(r[RW_MSGS]),
                   canon_bytes=int(r[RW_CANON]), steps=int(r[RW_STEPS]),
                   panic=int(bool(r[RW_FLAGS] & pxb.F_PANIC)), stuck=int(bool(r[RW_FLAGS] & pxb.F_STUCK)),
                   divergence=int(bool(r[RW_FLAGS] & pxb.F_LOG_DIVERGENCE)),
                   undecided=int(bool(r[RW_FLAGS] & pxb.F_UNDECIDED)),
                   step_cap=int(bool(r[RW_FLAGS] & pxb.F_STEP_CAP)))
        assert got == {k: cnt[k] for k in got}, "instance %d" % g
        assert int(r[RW_ROUNDS]) == int(eres[0][2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_pinned_case_is_present(shape):
    recs, _ = records(shape)
    for case, g in SHAPES[shape][5].items():
        assert case in case_of(recs[g]), "%s: instance %d shows %s" % (case, g, sorted(case_of(recs[g])))


def test_the_tight_shape_has_every_case():
    want = {"decides", "restarts", "capped", "quiet_undecided", "panics", "full_rfifo", "empty_pool"}
    assert want <= set(SHAPES["tight"][5])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rare_regions_were_entered(shape):
    """An Execute broadcast, its restart, and an Execute at its acceptor's
    ticket (a log entry, or the panic) happen in the pinned instances: the
    branches under test ran."""
    recs, ids = records(shape)
    seen = 0
    for g in ids:
        if not recs[g][RW_BAILED]:
            seen |= int(recs[g][RW_PROBES])
    assert seen & EVP_EXEC and seen & EVP_RESTART and seen & EVP_HIT and seen & EVP_RUN
    # a restart is counted from outside exactly when the probe saw one
    for g in ids:
        r = recs[g]
        if not r[RW_BAILED]:
            assert bool(r[RW_TWO_BCAST]) == bool(r[RW_PROBES] & EVP_RESTART), g
            assert not r[RW_EXECS] or r[RW_PROBES] & EVP_EXEC, g


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bail_flag_is_clear_on_entry_to_every_iteration(shape):
    """Seen from outside the lane before each step(): never set, up to and
    including the iteration that sets it (after which the driver stops, as
    the kernel's loop does)."""
    recs, ids = records(shape)
    for g in ids:
        r = recs[g]
        assert r[RW_ENTRY_BAILED] == 0, g
        if r[RW_BAILED] and not r[RW_BAIL_AT_INIT]:
            assert r[RW_ITERS] >= 1 and r[RW_PROBES] & (EVB_RING | EVB_RFIFO | EVB_POOL | EVB_QFIFO), g
