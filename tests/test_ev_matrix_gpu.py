"""The per-lane kernel's matrix (tests/ev_matrix.py) on the GPU: every routed
layout at every topology it is routed for, through pxb.run.  Per cell: results,
digests, acceptor records and totals equal the oracle's bit for bit, and the
device's hand-off counts equal the host lane's (tests/test_ev_matrix.py), so a
shape that handed its instances on instead of running them -- exact either
way, the next stage recomputes them -- does not pass."""
import os

import numpy as np
import pytest

import ev_matrix as M
import oracle_c
import pxb
from test_ev_matrix import expected_handoffs

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("cell", M.CELLS, ids=M.IDS)
def test_cell(gpu_lib, cell):
    cfg, first, n = cell.cfg, cell.first, M.N_INST
    pxb.handoff_counts(0, reset=True)
    res, dig, acc, cnt = pxb.run(cfg, first, n, want_acceptors=True)
    h1, h2 = pxb.handoff_counts(0, reset=True)
    eres, edig, eacc, ecnt = oracle_c.run_cpu(cfg, first, n, threads=THREADS, want_acceptors=True)
    bad = np.nonzero((res != eres).any(axis=1))[0]
    assert bad.size == 0, "first mismatching instance %d: gpu %s oracle %s" % (
        first + bad[0], res[bad[0]], eres[bad[0]])
    assert np.array_equal(dig, edig)
    assert np.array_equal(acc, eacc)
    assert cnt == ecnt
    want1, want2 = expected_handoffs(cell)
    print("%s: hand-offs %d, %d (host lane %d, %d)" % (M.cell_id(cell), h1, h2, len(want1), len(want2)))
    assert h1 <= n // 8, (h1, h2)
    assert (h1, h2) == (len(want1), len(want2))
