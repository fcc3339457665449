"""The per-lane kernels' lane-masked LDS stores on the device (LdsMem::st_if
and its halfword forms, csrc/paxos_ev_kernel.h; the sites: csrc/paxos_ev.h),
through the C ABI against the CPU oracle, bit for bit: results, digests and all
16 run totals, and the totals again from a call that passes no per-instance
buffer.

A masked store narrows the wave's exec mask for one instruction.  It must AND
the mask, not replace it: the iteration runs with the wave's idle lanes
masked off, so config 4 (the tight layout and its second stage) runs at 1, 63,
64, 65 and 2^14 instances -- one lane, a wave with one idle lane, a full wave,
a second wave of one lane, and enough for refills, draining waves and both
hand-off stages -- and with a step cap of 16, where finishing and refilling
lanes are dense.  Configs 3, 5 and 7 cover the compact, the split
three-proposer and the log-mode shapes, which share the header.  The
instances the device hands on are those the host lane hands on
(tests/native/ev_masked_store_host.cpp)."""
import dataclasses

import numpy as np
import pytest

import oracle_c
import pxb
from test_ev_masked_store import bailed_ids

N_INST = 1 << 14
C4 = pxb.CONFIGS[4]
BATCHES = {
    "c4": C4,
    "c4_cap16": dataclasses.replace(C4, step_cap=16),
    "c3": pxb.CONFIGS[3],
    "c5": pxb.CONFIGS[5],
    "c7": pxb.CONFIGS[7],
}
_want = {}


def want(name, n):
    """The oracle's outputs, computed once per (batch, count) and left unchanged."""
    if (name, n) not in _want:
        res, dig, _, cnt = oracle_c.run_cpu(BATCHES[name], 0, n, threads=16)
        res.setflags(write=False)
        dig.setflags(write=False)
        _want[(name, n)] = (res, dig, cnt)
    return _want[(name, n)]


def same(name, n):
    cfg = BATCHES[name]
    eres, edig, ecnt = want(name, n)
    res, dig, _, cnt = pxb.run(cfg, 0, n)
    assert np.array_equal(res, eres), "%s, %d instances: results differ from the oracle" % (name, n)
    assert np.array_equal(dig, edig), "%s, %d instances: digests differ from the oracle" % (name, n)
    assert len(ecnt) == 16 and cnt == ecnt, "%s, %d instances: totals %s, oracle %s" % (name, n, cnt, ecnt)
    # totals only: no result, digest or acceptor buffer
    _, _, _, cnt2 = pxb.run(cfg, 0, n, want_results=False, want_digests=False)
    assert cnt2 == ecnt, "%s, %d instances, totals only: %s, oracle %s" % (name, n, cnt2, ecnt)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, N_INST])
def test_config4_lane_counts(gpu_lib, n):
    same("c4", n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4_cap16", "c3", "c5", "c7"])
def test_batches_match_the_oracle(gpu_lib, name):
    same(name, N_INST)


@pytest.mark.gpu
def test_hand_offs_equal_the_host_lanes(gpu_lib):
    """pxb_handoff_counts of one config-4 call: the tight layout's hand-offs
    and its second stage's are the host lane's over the same instances."""
    first = bailed_ids(C4, 7, 2, N_INST)
    # (the second stage runs the ids the first handed on)
    from test_ev_masked_store import run_ids, RW_BAILED
    second = [g for g, r in run_ids(C4, 6, 2, first).items() if r[RW_BAILED]] if first else []
    assert len(first) > 0
    pxb.handoff_counts(reset=True)
    pxb.run(C4, 0, N_INST)
    assert tuple(pxb.handoff_counts()) == (len(first), len(second))
