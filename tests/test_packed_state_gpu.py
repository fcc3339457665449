"""The per-lane kernels' packed per-proposer state on the device: 2^14
contiguous instances of each bench workload that runs a per-lane shape
(configs 3, 4, 5 and 7) through the C ABI, against the CPU oracle word for
word -- results, digests and all 16 run totals.  Config 4, whose tight kernel
the packing was priced on, also with the in-kernel window draws
(PXB_NO_WIN_PREPASS=1) and from a first id whose low word wraps."""
import numpy as np
import pytest

import oracle_c
import pxb

N_INST = 1 << 14
CROSS = (1 << 32) - (N_INST // 2)            # (ids on both sides of 2^32)
_want = {}


def want(c, first):
    """The oracle's outputs, computed once per (config, first id) and left unchanged."""
    if (c, first) not in _want:
        res, dig, _, cnt = oracle_c.run_cpu(pxb.CONFIGS[c], first, N_INST, threads=16)
        res.setflags(write=False)
        dig.setflags(write=False)
        _want[(c, first)] = (res, dig, cnt)
    return _want[(c, first)]


def same(c, first):
    res, dig, _, cnt = pxb.run(pxb.CONFIGS[c], first, N_INST)
    eres, edig, ecnt = want(c, first)
    assert np.array_equal(res, eres), "config %d: results differ from the oracle" % c
    assert np.array_equal(dig, edig), "config %d: digests differ from the oracle" % c
    assert len(ecnt) == 16 and cnt == ecnt, "config %d: totals %s, oracle %s" % (c, cnt, ecnt)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 4, 5, 7])
def test_bench_configs_match_the_oracle(gpu_lib, c):
    same(c, 0)


@pytest.mark.gpu
def test_config4_with_in_kernel_window_draws(gpu_lib):
    with pxb.hooks(PXB_NO_WIN_PREPASS="1"):
        same(4, 0)


@pytest.mark.gpu
def test_config4_first_id_crosses_32_bits(gpu_lib):
    same(4, CROSS)
