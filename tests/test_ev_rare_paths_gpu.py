"""The rarely-needed regions of the per-lane kernels' iteration on the device
(the Execute branches, the step end, the bail flag: csrc/paxos_ev.h,
csrc/paxos_ev_kernel.h), through the C ABI against the CPU oracle, word for
word: results, digests and all 16 run totals, and the totals again from a
call that passes no per-instance buffer.

Config 4 (the tight layout and its second stage) at 1, 63, 64, 65 and 2^14
instances: one lane, a wave with one idle lane, a full wave, a second wave of
one lane, and enough for refills and both hand-off stages; with a step cap of
16, so that finishing and refilling lanes are dense; and without crash windows
at delays of one step, so that every instance decides at once.  That last
batch is fault-free, which the routing gives to the fault-free kernel, so it
is run beside the same batch at delays of up to two steps, which stays on the
tight layout.  Configs 3, 5 and 7 cover the compact, the split three-proposer
and the log-mode shapes that share the header."""
import dataclasses

import numpy as np
import pytest

import oracle_c
import pxb

N_INST = 1 << 14
C4 = pxb.CONFIGS[4]
BATCHES = {
    "c4": C4,
    "c4_cap16": dataclasses.replace(C4, step_cap=16),
    "c4_dense_exec": dataclasses.replace(C4, crash_ppm=0, delay_max=1),
    "c4_dense_exec_d2": dataclasses.replace(C4, crash_ppm=0, delay_max=2),
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
def test_config4_two_stages_ran(gpu_lib):
    """2^14 instances reach both hand-off stages: the tight layout hands
    instances on to layout 6 (the host model: 0.76 %)."""
    pxb.handoff_counts(reset=True)
    same("c4", N_INST)
    assert pxb.handoff_counts()[0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4_cap16", "c4_dense_exec", "c4_dense_exec_d2", "c3", "c5", "c7"])
def test_batches_match_the_oracle(gpu_lib, name):
    same(name, N_INST)


def test_dense_batches_are_what_they_are_for():
    """(No GPU.)  With a step cap of 16 every instance ends within 16 steps;
    without crash windows every instance decides, so each makes at least one
    Execute broadcast."""
    n = 2048
    res, _, _, cnt = oracle_c.run_cpu(BATCHES["c4_cap16"], 0, n, threads=16)
    assert int((res[:, 3] >> 16).max()) <= 16 and cnt["step_cap"] > n // 2
    for name in ("c4_dense_exec", "c4_dense_exec_d2"):
        _, _, _, cnt = oracle_c.run_cpu(BATCHES[name], 0, n, threads=16)
        assert cnt["decided"] == n and cnt["executes"] >= n
