"""The per-lane kernel's matrix (tests/ev_matrix.py) on the CPU.  For every
cell: (a) the routing names the layouts the table claims, (b) the host build
of the lane on those layouts equals the oracle on every instance it keeps,
which also records the cell's expected hand-offs, and (c) the first stage
hands on at most an eighth of the cell, so the layout under test runs the rest.

tests/test_ev_matrix_gpu.py runs the same cells on the device and holds its
hand-off counts to the host lane's (expected_handoffs).

Hand-offs out of 4096, host build (first = 1000):
  L3    0, but (3, 5): 1
  L6    (2, 5) 5, (2, 8) 7, (3, 3) 1, (3, 5) 31, else 0; layout 7: N = 6: 7, N = 7: 33
        (of which layout 6 hands on 0 and 1)
  L5    <= 27 (2, 9)
  L0    0 for P <= 2; P = 3 up to 153 (3, 9)
  L1    <= 191 (3, 9)
  LG4   <= 303 (3, 8); (3, 9) on its eased schedule (4 Ticks): see ev_matrix.py
  LG9   (2, 5) 128, (3, 3) 3, else 0
"""
import contextlib
import os

import numpy as np
import pytest

import ev_matrix as M
import pxb
import script_oracle as SO
from test_ev_host import check, ev_run
from test_route_plan import plan

_TWO = {(7, 6): "TIGHT", (4, 8): "LG2", (9, 8): "LG2"}
_handoffs = {}


@contextlib.contextmanager
def _forced_layout(layout):
    old = os.environ.get("EV_LAYOUT")
    os.environ["EV_LAYOUT"] = str(layout)
    try:
        yield
    finally:
        if old is None:
            del os.environ["EV_LAYOUT"]
        else:
            os.environ["EV_LAYOUT"] = old


def _bails(cell, layout, verify):
    """The ids (offsets from cell.first) the host lane on `layout` hands on;
    verify: and it equals the oracle (results, digests, acceptor records,
    totals) on every other instance."""
    with _forced_layout(layout):
        if verify:
            return check(cell.cfg, cell.first, M.N_INST, max_bail_frac=1.0)[2]
        return ev_run(cell.cfg, cell.first, M.N_INST)[4]


def expected_handoffs(cell, verify=False):
    """(first hand-offs, second hand-offs) of a cell, as sorted id arrays: what
    the host lane on the cell's first-stage layout bails, and, of those, what
    the second-stage layout bails too (none for a single-stage cell).  The bail
    decision is a function of the instance and the layout alone, so these are
    the device's hand-offs as well."""
    key = M.cell_id(cell)
    if key not in _handoffs or (verify and not _handoffs[key][2]):
        b1 = np.sort(_bails(cell, cell.layout1, verify))
        b2 = np.zeros(0, b1.dtype)
        if cell.layout2 is not None:
            b2 = np.intersect1d(b1, _bails(cell, cell.layout2, verify))
        for a in (b1, b2):
            a.setflags(write=False)
        _handoffs[key] = (b1, b2, verify)
    return _handoffs[key][:2]


def test_the_table_is_the_issue_s():
    fams = {f: [c for c in M.CELLS if c.family == f] for f in M.FAMILIES}
    assert {f: len({(c.P, c.N) for c in v}) for f, v in fams.items()} == {
        "L3": 19, "L6": 19, "L5": 24, "L0": 24, "L1": 24, "LG4": 24, "LG9": 14}
    for f, v in fams.items():                          # one cell per family across 2^32 as well
        hi = [c for c in v if c.first != M.FIRST]
        assert len(hi) == 1 and hi[0].first < (1 << 32) < hi[0].first + M.N_INST, f
    assert len(set(M.IDS)) == len(M.CELLS) == 148 + 7
    assert all(c.cfg.seed == 0x5EED0200 + 16 * c.P + c.N for c in M.CELLS)
    # every routed layout is some cell's first stage (layout 2 is never routed to,
    # layout 8 only as a second stage)
    assert {c.layout1 for c in M.CELLS} == {0, 1, 3, 4, 5, 6, 7, 9}
    assert {c.layout2 for c in M.CELLS} == {None, 6, 8}


def lane_host(P, N, mode):
    """A lane-family shape's LANE_IDS as all-keep rows through the host build of
    the scripted lane (tests/native/script_host.cpp): the rows and its outputs
    (computed once, read-only)."""
    key = (P, N, mode)
    if key not in _lane_host:
        cfg =M.lane_cfg(P, N, mode)
        rows = pxb.scripts_empty(cfg, M.LANE_IDS, M.LANE_DEPTH)
        h = SO.host_run(cfg, rows, M.LANE_DEPTH)
        for a in (rows, *h.values()):
            a.setflags(write=False)
        _lane_host[key] = (rows, h)
    return _lane_host[key]


_lane_host = {}


@pytest.mark.parametrize("P,N,mode", M.LANE_SHAPES, ids=M.LANE_SHAPE_IDS)
def test_lane_family_shape(P, N, mode):
    """The condition of the GPU sweeps of the lane-kernel families: at most an
    eighth of a shape's rows end with a status other than OK on the host build
    of the lane, and the others equal the oracle."""
    rows, h = lane_host(P, N, mode)
    eres, edig, eacc = M.lane_oracle(P, N, mode)
    ok = h["status"] == pxb.TRACE_OK
    print("p%dn%d-%s: %d of %d rows not OK" % (P, N, mode, int((~ok).sum()), len(ok)))
    assert int((~ok).sum()) <= M.LANE_CAP
    assert np.array_equal(h["res"][ok], eres[ok]) and np.array_equal(h["dig"][ok], edig[ok])
    assert np.array_equal(h["acc"][ok], eacc[ok])
    # (what the batched trace's sweep relies on: with tail = 1 an OK row keeps one
    # record, that of its last step)
    t = SO.host_run(M.lane_cfg(P, N, mode), rows, M.LANE_DEPTH, sel=(0, 0xFFFFFFFF, 1), capacity=1)
    assert (t["n_kept"][ok] == 1).all() and np.array_equal(t["rec"][ok, 0, 0], (eres[ok][:, 3] >> 16) - 1)


@pytest.mark.parametrize("cell", M.CELLS, ids=M.IDS)
def test_cell(cell):
    # (a) the plan is the intended one
    p = plan(cell.cfg)
    assert p["kind"] == "EV"
    if cell.layout2 is None:
        assert (p["two"], p["second"], "first" in p) == ("NONE", (cell.P, cell.N, cell.layout1), False), p
    else:
        assert (p["two"], p["first"], p["second"]) == (
            _TWO[cell.layout1, cell.layout2], (cell.P, cell.N, cell.layout1), (cell.P, cell.N, cell.layout2)), p
    # (b) the host lane equals the oracle on every instance it keeps
    h1, h2 = expected_handoffs(cell, verify=True)
    print("%s: %d first hand-offs, %d second" % (M.cell_id(cell), len(h1), len(h2)))
    # (c) the cap
    assert len(h1) <= M.HANDOFF_CAP, "%d of %d instances leave the layout under test" % (len(h1), M.N_INST)
