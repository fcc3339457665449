"""Round 10's rewrites of the per-lane state machine (csrc/paxos_ev.h) and of
its driver's run totals (csrc/paxos_ev_kernel.h), on the CPU:

- the selects over the acceptor arrays with the one-hot lane masks made once
  per acceptor op and kept for both reads and the write-back, and the lane
  masks that feed shifts as one shift-and-combine (the host build runs their
  plain C++ forms);
- the instance index derived from the Philox counter word, and the proposer
  count and largest delay of a simple schedule read from the launch
  parameters;
- the six (log mode: seven) 0 / 1-per-instance sums packed as 10-bit fields.

The host build of EvLane (tests/native/ev_valu_host.cpp) runs pinned instances
one at a time on the tight, layout-6, slim P = 2, log-mode and slim P = 3
shapes and on one-proposer shapes over two acceptors (and over one, below: the
smallest arrays a select can get wrong), and every instance is compared with
the CPU oracle: result words, digests, rounds, executes, messages, canonical bytes and
whether it is handed on.  The driver watches the acceptor registers from
outside: on every shape some pinned instance has every acceptor index
0 .. N - 1 both answer a request (its ticket or stored ticket changes) and
take an Execute (its log grows), and no iteration changes two acceptors."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import oracle_c
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ev_valu_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libev_valu_host.so")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")] + [
                    os.path.join(HERE, "..", "include", "paxos_batch.h")]
# a record's words (ev_valu_host.cpp)
(VW_RES, VW_ROUNDS, VW_EXECS, VW_MSGS, VW_CANON, VW_BAILED, VW_FLAGS, VW_STEPS, VW_ANSWERED, VW_EXECUTED, VW_OTHERS,
 VW_GID, VW_N) = (0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
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
        _lib.ev_valu_flush_bound.restype = C.c_uint32
        assert _lib.ev_valu_words() == VW_N
    return _lib


LOG_CFG = pxb.Config(seed=0x1065, n_proposers=2, n_acceptors=5, loss_ppm=100000, delay_max=4, skew_max=3,
                     crash_ppm=200000, crash_len_max=12, crash_start_max=30, step_cap=1024, n_ticks=16, tick_period=4)
# (the ABI and the oracle start at two acceptors: the one-acceptor shape runs a
# fault-free schedule, whose outcome follows from the two-acceptor one's)
P1N1 = pxb.Config(seed=0x10A1, n_proposers=1, n_acceptors=1, step_cap=128)
P1N2 = pxb.Config(seed=0x10A2, n_proposers=1, n_acceptors=2, loss_ppm=100000, delay_max=3, skew_max=2,
                  crash_ppm=200000, crash_len_max=6, crash_start_max=6, step_cap=128)
P1N2_SIMPLE = pxb.Config(seed=0x10A3, n_proposers=1, n_acceptors=2, delay_max=3,
                         crash_ppm=200000, crash_len_max=6, crash_start_max=6, step_cap=128)
FIRST = list(range(48))
# config 5's instances drawn with three proposers: the two-proposer shape hands them on in init
P3_OF_FIRST = [1, 3, 6, 9, 15, 16, 19, 20, 22, 26, 28, 38, 39, 40, 41, 42, 43, 45, 46]
# shape: layout, proposer capacity, config, ids beyond the first 48, the ids
# handed on, an instance in which every acceptor index answers a request and
# takes an Execute, and one that panics (None: the config has none nearby)
SHAPES = {
    "tight": (7, 2, pxb.CONFIGS[4], [49, 67], [49, 67], 1, 33),
    "layout6": (6, 2, pxb.CONFIGS[4], [49, 67], [], 1, 33),
    "slim_p2": (5, 2, pxb.CONFIGS[5], [], P3_OF_FIRST, 7, 0),
    "log_p2": (4, 2, LOG_CFG, [], [], 0, 1),
    "slim_p3": (5, 3, pxb.CONFIGS[5], [], [], 7, 0),
    "p1_n2": (0, 1, P1N2, [], [], 1, None),
    "p1_n2_simple": (6, 1, P1N2_SIMPLE, [], [], 0, None),
}
_recs = {}


def records(shape):
    """The driver's records of the shape's ids, run once and left unchanged."""
    if shape not in _recs:
        layout, pm, cfg, extra = SHAPES[shape][:4]
        ids = np.asarray(FIRST + extra, np.uint32)
        rec = np.zeros((len(ids), VW_N + cfg.n_acceptors), np.uint32)
        c = cfg.to_c(0, 1 << 31)
        rc = lib().ev_valu_run(C.byref(c), layout, pm, C.c_void_p(ids.ctypes.data), len(ids),
                               C.c_void_p(rec.ctypes.data))
        assert rc == 0, "ev_valu_run rc=%d" % rc
        rec.setflags(write=False)
        _recs[shape] = ({int(g): rec[i] for i, g in enumerate(ids)}, [int(g) for g in ids])
    return _recs[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_instance_matches_the_oracle(shape):
    cfg, handed_on = SHAPES[shape][2], SHAPES[shape][4]
    recs, ids = records(shape)
    N = cfg.n_acceptors
    assert sorted(g for g in ids if recs[g][VW_BAILED]) == sorted(handed_on)
    for g in ids:
        r = recs[g]
        assert int(r[VW_GID]) == g, "instance %d: index from the counter word" % g
        if r[VW_BAILED]:
            continue
        eres, edig, _, cnt = oracle_c.run_cpu(cfg, g, 1)
        assert list(r[VW_RES:VW_RES + 4]) == list(eres[0]), "instance %d: result words" % g
        assert list(r[VW_N:VW_N + N]) == list(edig[0]), "instance %d: digests" % g
        got = dict(rounds=int(r[VW_ROUNDS]), executes=int(r[VW_EXECS]), messages=int(r[VW_MSGS]),
                   canon_bytes=int(r[VW_CANON]), steps=int(r[VW_STEPS]),
                   panic=int(bool(r[VW_FLAGS] & pxb.F_PANIC)), stuck=int(bool(r[VW_FLAGS] & pxb.F_STUCK)),
                   divergence=int(bool(r[VW_FLAGS] & pxb.F_LOG_DIVERGENCE)),
                   undecided=int(bool(r[VW_FLAGS] & pxb.F_UNDECIDED)),
                   step_cap=int(bool(r[VW_FLAGS] & pxb.F_STEP_CAP)))
        assert got == {k: cnt[k] for k in got}, "instance %d" % g


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_acceptor_index_answers_and_executes(shape):
    cfg, pinned, panics = SHAPES[shape][2], SHAPES[shape][5], SHAPES[shape][6]
    recs, ids = records(shape)
    full = (1 << cfg.n_acceptors) - 1
    r = recs[pinned]
    assert not r[VW_BAILED]
    assert int(r[VW_ANSWERED]) == full, "instance %d: answered %#x" % (pinned, int(r[VW_ANSWERED]))
    assert int(r[VW_EXECUTED]) == full, "instance %d: executed %#x" % (pinned, int(r[VW_EXECUTED]))
    if panics is not None:      # the Execute branch's other arm: the dead bit through the same write-back
        assert recs[panics][VW_FLAGS] & pxb.F_PANIC and not recs[panics][VW_BAILED]
    # one acceptor op per iteration: a write-back never touches a second element
    assert all(recs[g][VW_OTHERS] == 0 for g in ids)


def test_one_acceptor():
    """Arrays of one element (the host build only: the ABI starts at two
    acceptors, so the oracle cannot run it).  Fault-free, one proposer: the
    acceptor grants ticket 1, accepts c1 and executes it, as each of two
    acceptors does in the same schedule, which the oracle runs: the same
    result words and the same digest, and half the messages (3 broadcasts of
    N copies and 2 N replies)."""
    ids = np.arange(8, dtype=np.uint32)
    rec = np.zeros((len(ids), VW_N + 1), np.uint32)
    c = P1N1.to_c(0, 1 << 31)
    rc = lib().ev_valu_run(C.byref(c), 0, 1, C.c_void_p(ids.ctypes.data), len(ids), C.c_void_p(rec.ctypes.data))
    assert rc == 0
    two = dataclasses.replace(P1N1, n_acceptors=2)
    for i, g in enumerate(ids):
        r = rec[i]
        eres, edig, _, cnt = oracle_c.run_cpu(two, int(g), 1)
        assert cnt["decided"] == 1 and cnt["messages"] == 10 and edig[0][0] == edig[0][1]
        assert not r[VW_BAILED] and int(r[VW_GID]) == g
        assert list(r[VW_RES:VW_RES + 4]) == list(eres[0])
        assert int(r[VW_N]) == int(edig[0][0])
        assert (int(r[VW_ROUNDS]), int(r[VW_EXECS]), int(r[VW_MSGS])) == (cnt["rounds"], cnt["executes"], 5)
        assert int(r[VW_ANSWERED]) == 1 and int(r[VW_EXECUTED]) == 1 and r[VW_OTHERS] == 0


# ---- the packed 0 / 1 sums ----
FLAG_OF_SUM = [None, pxb.F_UNDECIDED, pxb.F_STUCK, pxb.F_PANIC, pxb.F_LOG_DIVERGENCE, pxb.F_STEP_CAP, pxb.F_LOG_TRUNC]


def plain_sums(flags_list, log):
    """Instances, then one sum per flag, in the kernel's total order (log-trunc only in log mode)."""
    out = [len(flags_list)]
    for k in range(1, 7):
        out.append(sum(1 for f in flags_list if f & FLAG_OF_SUM[k]) if (k < 6 or log) else 0)
    return out


@pytest.mark.parametrize("log", [0, 1])
@pytest.mark.parametrize("flags", [0x00, 0xFF])
@pytest.mark.parametrize("n", [0, 1, 255, 256])
def test_packed_sums_equal_plain_sums(n, flags, log):
    assert lib().ev_valu_flush_bound() == 256       # a lane's instances between two flushes
    out = np.zeros(9, np.uint32)
    lib().ev_valu_flag_sums(log, n, flags, C.c_void_p(out.ctypes.data))
    assert [int(x) for x in out[:7]] == plain_sums([flags] * n, log)
    assert int(out[7]) == n
    assert int(out[8]) == (3 if log else 2)          # words a lane carries


@pytest.mark.parametrize("log", [0, 1])
def test_packed_sums_of_mixed_flags(log):
    """Each field counts its own flag only: 256 instances with every
    combination of the eight flag bits, once each."""
    fl = np.arange(256, dtype=np.uint32)
    out = np.zeros(7, np.uint32)
    lib().ev_valu_flag_sums_list(log, C.c_void_p(fl.ctypes.data), len(fl), C.c_void_p(out.ctypes.data))
    assert [int(x) for x in out] == plain_sums([int(f) for f in fl], log)
    # and one flag at a time, 256 times: its field alone reaches the bound
    for k in range(1, 7):
        one = np.full(256, FLAG_OF_SUM[k], np.uint32)
        lib().ev_valu_flag_sums_list(log, C.c_void_p(one.ctypes.data), len(one), C.c_void_p(out.ctypes.data))
        assert [int(x) for x in out] == plain_sums([FLAG_OF_SUM[k]] * 256, log), k
