"""The per-lane kernels at the limits of their packed fields, on the GPU: the
cells of tests/ev_limits.py through pxb.run.  Per cell, as
tests/test_ev_matrix_gpu.py does but without its bound on the hand-offs
(A512 hands nearly every instance on): results, digests, acceptor records and
totals equal the oracle's bit for bit, and the device's hand-off counts equal
the host lane's (ev_limits.HANDOFFS, which tests/test_ev_limits.py holds to the
host lane).  The counts are the check that
bites: a field that wraps on the device before the hand-off fires, or a
hand-off that fires one event late, moves them even where the next stage's
re-run hides the damage.

Then config 4 at step_cap = 512 on the tight routing (the largest cap the
compact layouts are routed for) from id 0 and across 2^32, and the lane-kernel
families, which have no next stage: cell D's hand-offs end PXB_TRACE_BAILED
there, exactly where the host build of the families' shape bails."""
import os

import numpy as np
import pytest

import ev_limits as EL
import oracle_c
import pxb
from test_ev_limits import lane_d_host

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
_CELLS = EL.CELLS + EL.TIGHT


@pytest.mark.parametrize("cell", _CELLS, ids=[EL.cell_id(c) for c in _CELLS])
def test_cell(gpu_lib, cell):
    cfg, first, n = cell.cfg, cell.first, EL.N_INST
    pxb.handoff_counts(0, reset=True)
    res, dig, acc, cnt = pxb.run(cfg, first, n, want_acceptors=True)
    h1, h2 = pxb.handoff_counts(0, reset=True)
    eres, edig, eacc, ecnt = oracle_c.run_cpu(cfg, first, n, threads=THREADS, want_acceptors=True)
    want = EL.HANDOFFS[EL.cell_id(cell)]                    # (the host lane's: tests/test_ev_limits.py)
    print("%s: hand-offs %d, %d (host lane %d, %d)" % (EL.cell_id(cell), h1, h2, *want))
    bad = np.nonzero((res != eres).any(axis=1))[0]
    assert bad.size == 0, "first mismatching instance %d: gpu %s oracle %s" % (
        first + bad[0], res[bad[0]], eres[bad[0]])
    assert np.array_equal(dig, edig)
    assert np.array_equal(acc, eacc)
    assert cnt == ecnt
    assert (h1, h2) == want


def test_lane_families_at_the_log_limit(gpu_lib):
    """128 ids of cell D, every hand-off of its first 1,000 among them, through
    the batched trace and, as rows extracted at depth 64, through the scripted
    lane: PXB_TRACE_BAILED exactly where the host build of that family's
    shape bails, and every PXB_TRACE_OK result is the oracle's.  (A link of
    these rows consumes up to some 1,500 entries; past the depth an entry reads
    the row's own Philox stream, script_core.h, so depth 64 carries the run.)"""
    d = lane_d_host()
    cfg, ids = EL.BY_ID["D"].cfg, d["ids"]
    rec, offs, status, res = pxb.trace_batch(cfg, ids, tail=1)
    ok = status == pxb.TRACE_OK
    print("trace_batch: %d of %d bailed" % (int((~ok).sum()), len(ok)))
    assert np.array_equal(status, d["tstatus"]) and int((status == pxb.TRACE_BAILED).sum()) == len(EL.LANE_D_HANDED_ON)
    assert np.array_equal(res[ok], d["eres"][ok])
    assert offs[-1] == len(rec) and (np.diff(offs.astype(np.int64))[ok] == 1).all()
    assert np.array_equal(rec[offs[:-1][ok].astype(np.int64), 0], (d["eres"][ok][:, 3] >> 16) - 1)

    rows = pxb.extract_schedule(cfg, ids, EL.LANE_DEPTH)
    assert np.array_equal(rows, d["rows"])
    res, dig, acc, status, sent = pxb.run_scripted(cfg, rows, EL.LANE_DEPTH, want_acceptors=True)
    ok = status == pxb.TRACE_OK
    print("run_scripted: %d of %d bailed" % (int((~ok).sum()), len(ok)))
    h = d["h"]
    assert np.array_equal(status, h["status"]) and int((status == pxb.TRACE_BAILED).sum()) == len(EL.LANE_D_HANDED_ON)
    assert np.array_equal(sent, h["sent"])
    assert np.array_equal(res[ok], d["eres"][ok]) and np.array_equal(dig[ok], d["edig"][ok])
    assert np.array_equal(acc[ok], d["eacc"][ok])
