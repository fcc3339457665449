"""The per-lane state machine's packed per-proposer state (csrc/paxos_ev.h):
for up to two proposers the broadcast counters (copies finished: the request
links' Philox seq; broadcasts queued: the ring index) are 16-bit fields of one
word each, and the pending-broadcast queue takes both entries of a handler's
two broadcasts in one shifted insert.

The host build of EvLane (tests/native/ev_packed_host.cpp) runs against the CPU
oracle instance by instance, as tests/test_ev_host.py does, while the driver
watches the queue and the counters from outside: every step's queue must be
what its inserts and pops make it, an ended instance's two counters must agree,
and the inputs below reach the fields' edges (a counter past 8 bits, a ring
index that wraps many times, the two-entry insert at every queue length)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_c
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ev_packed_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libev_packed_host.so")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")] + [
                    os.path.join(HERE, "..", "include", "paxos_batch.h")]
(ST_INS2_LEN0, ST_INS2_LEN1, ST_INS2_LEN2, ST_MAX_BCAST, ST_OVER_256, ST_BAD_QUEUE, ST_BAD_COUNT, ST_PACKED,
 ST_RING_SLOTS, ST_N) = range(10)
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
    return _lib


def packed_run(cfg, layout, pm, first, n):
    N = cfg.n_acceptors
    res = np.zeros((n, 4), np.uint32)
    dig = np.zeros((n, N), np.uint32)
    acc = np.zeros((n, N, 4), np.uint32)
    tot = (C.c_int64 * 16)()
    bail = np.zeros(max(n, 1), np.uint32)
    st = np.zeros(ST_N, np.uint64)
    nb = C.c_uint32(0)
    c = cfg.to_c(first, n)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib().ev_packed_run(C.byref(c), layout, pm, p(res), p(dig), p(acc), tot, p(bail), C.byref(nb), p(st))
    assert rc == 0, "ev_packed_run rc=%d" % rc
    return res, dig, acc, pxb.counters_dict(list(tot)), bail[:nb.value].copy(), [int(x) for x in st]


def check(cfg, layout, pm, first, n, max_bail_frac):
    """Exact against the oracle for every instance the shape keeps (results,
    digests, acceptor records, totals), the queue and the counters consistent
    at every step; returns the driver's statistics."""
    res, dig, acc, cnt, bails, st = packed_run(cfg, layout, pm, first, n)
    eres, edig, eacc, ecnt = oracle_c.run_cpu(cfg, first, n, threads=8, want_acceptors=True)
    ok = np.ones(n, bool)
    ok[bails] = False
    bad = np.nonzero(((res != eres).any(1) | (dig != edig).any(1) | (acc != eacc).any((1, 2))) & ok)[0]
    assert bad.size == 0, "instance %d: ev %s oracle %s" % (first + bad[0], res[bad[0]], eres[bad[0]])
    for b in bails:                                      # totals: the oracle's minus the bailed instances' own
        _, _, _, bc = oracle_c.run_cpu(cfg, first + int(b), 1)
        for k in ecnt:
            ecnt[k] -= bc[k]
    assert cnt == ecnt
    assert len(bails) <= max_bail_frac * n + 1, "%d of %d instances bailed" % (len(bails), n)
    assert st[ST_BAD_QUEUE] == 0 and st[ST_BAD_COUNT] == 0
    return st, bails


# the shapes the issue names: layout, proposer capacity, config
TIGHT = (7, 2, pxb.CONFIGS[4])
LAYOUT6 = (6, 2, pxb.CONFIGS[4])
SLIM_P2 = (5, 2, pxb.CONFIGS[5])
SLIM_P3 = (5, 3, pxb.CONFIGS[5])
LOG_CFG = pxb.Config(seed=0x1065, n_proposers=2, n_acceptors=5, loss_ppm=100000, delay_max=4, skew_max=3,
                     crash_ppm=200000, crash_len_max=12, crash_start_max=30, step_cap=1024, n_ticks=16, tick_period=4)
LOG_MODE = (4, 2, LOG_CFG)
LOG_SLIM = (9, 2, LOG_CFG)


@pytest.mark.parametrize("layout,pm,cfg,frac", [
    TIGHT + (0.015,), LAYOUT6 + (0.001,), SLIM_P2 + (0.45,), LOG_MODE + (0.05,), LOG_SLIM + (0.05,)],
    ids=["tight", "layout6", "slim_p2", "log", "log_slim"])
@pytest.mark.parametrize("first", [0, (1 << 32) - 700])
def test_packed_shapes_match_the_oracle(layout, pm, cfg, frac, first):
    """Every shape of up to two proposers that build() instantiates for the
    bench workloads, from instance 0 and across 2^32."""
    st, _ = check(cfg, layout, pm, first, 1500, frac)
    assert st[ST_PACKED] == 1 and st[ST_RING_SLOTS] == 4


def test_one_proposer_counters_are_plain_words():
    cfg = pxb.Config(seed=0x51, n_proposers=1, n_acceptors=7, delay_max=4, crash_ppm=250000, crash_len_max=12,
                     crash_start_max=10, step_cap=300)
    st, bails = check(cfg, 6, 1, 99, 1200, 0.0)
    assert st[ST_PACKED] == 1 and len(bails) == 0


@pytest.mark.parametrize("layout,pm", [(5, 3), (0, 3)], ids=["slim_p3", "wide_p3"])
def test_three_proposers_keep_a_word_each(layout, pm):
    """The unpacked path: three proposers' counters stay one word per proposer."""
    cfg = pxb.CONFIGS[5] if layout == 5 else pxb.Config(
        seed=0x3A5, n_proposers=3, n_acceptors=5, loss_ppm=150000, delay_max=5, skew_max=2, crash_ppm=150000,
        crash_len_max=8, crash_start_max=6, step_cap=200)
    st, _ = check(cfg, layout, pm, 9000, 1500, 0.03)
    assert st[ST_PACKED] == 0
    assert st[ST_INS2_LEN0] + st[ST_INS2_LEN1] + st[ST_INS2_LEN2] > 0


# Two proposers that duel for 1,024 steps: delays of 1 or 2 steps, no loss, no
# skew, so most instances run to the step cap with both proposers restarting
# every few steps (the oracle: up to 492 rounds per instance).  Layout 0 is
# what the routing gives a 1,024-step run; the simple layouts serve it too.
DUEL = pxb.Config(seed=0xD0E1, n_proposers=2, n_acceptors=7, delay_max=2, crash_ppm=200000, crash_len_max=16,
                  crash_start_max=8, step_cap=1024)


@pytest.mark.parametrize("layout", [0, 6, 7], ids=["wide", "layout6", "tight"])
def test_broadcast_counter_carries_past_8_bits(layout):
    """Instances whose proposers make more than 256 broadcasts each: a counter
    field carries past its low byte and stays clear of its neighbour (it is the
    request links' Philox seq, so any slip changes every later delay draw),
    and the ring index wraps more than 50 times."""
    st, bails = check(DUEL, layout, 2, 0, 300, 0.0)
    assert st[ST_PACKED] == 1 and len(bails) == 0
    assert st[ST_OVER_256] > 100 and st[ST_MAX_BCAST] > 400
    assert st[ST_MAX_BCAST] // st[ST_RING_SLOTS] > 50


# A two-entry insert behind two queued broadcasts needs the other proposer's
# Execute and restart (or two restarts) still unsent when this one's Round 2
# succeeds: about one instance in 2,000 of this duel (delays to 3, 256 steps;
# found with this driver), one in 3,000 of config 5's two-proposer share.
DUEL3 = pxb.Config(seed=0xD0E1, n_proposers=2, n_acceptors=7, delay_max=3, crash_ppm=200000, crash_len_max=16,
                   crash_start_max=8, step_cap=256)


@pytest.mark.parametrize("layout,pm,cfg,first,n", [
    (7, 2, DUEL3, 20000, 12000), (6, 2, DUEL3, 20000, 12000), SLIM_P2 + (5000, 3000)],
    ids=["tight", "layout6", "slim_p2"])
def test_two_broadcast_insert_at_every_queue_length(layout, pm, cfg, first, n):
    """Execute plus the restart's AskForTicket, queued by one handler, into a
    pending queue of 0, 1 and 2 entries (the proposer op runs only with room
    for two, so 2 is the most): seen at each length, and every one of them
    left the queue as checked step by step."""
    st, _ = check(cfg, layout, pm, first, n, 0.45)
    assert st[ST_INS2_LEN0] > 0 and st[ST_INS2_LEN1] > 0 and st[ST_INS2_LEN2] > 0, st[:3]
