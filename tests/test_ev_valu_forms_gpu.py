"""Round 10's rewrites of the per-lane kernels on the device (the acceptor
selects with their lane masks kept, the shift-and-combine forms of lane masks,
the packed 0 / 1 run totals, the instance index from the counter word:
csrc/paxos_ev.h, csrc/paxos_ev_kernel.h), through the C ABI.

Against the CPU oracle, word for word (results, digests, all 16 run totals,
and the totals again from a call that passes no per-instance buffer): config 4
(the tight layout and its second stage) at 1, 63, 64, 65 and 2^14 instances,
and configs 3, 5 and 7 (the compact, the split three-proposer and the log-mode
shapes, which share the header) at 2^14.

The packed totals across a flush: config 4 with a step cap of 16 at 2^23
instances with one block per CU, 256 waves of 64 lanes, so that every lane
finishes about 512 instances and passes the flush bound of 256 several times;
the totals must equal those of the same batch at the default residency and
those of the same batch without the tight layout."""
import dataclasses

import numpy as np
import pytest

import oracle_c
import pxb

N_INST = 1 << 14
N_FLUSH = 1 << 23
C4 = pxb.CONFIGS[4]
C4_CAP16 = dataclasses.replace(C4, step_cap=16)
BATCHES = {"c4": C4, "c3": pxb.CONFIGS[3], "c5": pxb.CONFIGS[5], "c7": pxb.CONFIGS[7]}
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
def test_config4_sizes(gpu_lib, n):
    same("c4", n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3", "c5", "c7"])
def test_other_configs(gpu_lib, name):
    same(name, N_INST)


@pytest.mark.gpu
def test_packed_totals_across_flushes(gpu_lib):
    def totals(**env):
        with pxb.hooks(**env):
            _, _, _, cnt = pxb.run(C4_CAP16, 0, N_FLUSH, want_results=False, want_digests=False)
        return cnt

    one_block = totals(PXB_BLOCKS_PER_CU="1")
    default = totals()
    no_tight = totals(PXB_NO_TIGHT="1")
    assert one_block["instances"] == N_FLUSH
    assert one_block["decided"] + one_block["undecided"] == N_FLUSH
    assert one_block["step_cap"] > N_FLUSH // 2          # (most instances end at the cap: dense finishing lanes)
    assert one_block == default, "one block per CU: %s, default residency: %s" % (one_block, default)
    assert one_block == no_tight, "one block per CU: %s, without the tight layout: %s" % (one_block, no_tight)


def test_the_flush_batch_is_what_it_is_for():
    """(No GPU.)  With a step cap of 16 most instances end at the cap, and some
    decide before it, so the instance, step-cap, undecided and decided sums
    all move; 2^23 instances over 256 waves of 64 lanes are 512 a lane."""
    n = 4096
    res, _, _, cnt = oracle_c.run_cpu(C4_CAP16, 0, n, threads=16)
    assert int((res[:, 3] >> 16).max()) <= 16
    assert cnt["step_cap"] > n // 2 and cnt["decided"] > 0 and cnt["undecided"] > 0
    assert N_FLUSH // (256 * 64) >= 2 * 256
