"""pxb_explore_win on the GPU (docs/SEMANTICS.md §17): pxb.explore_win and
pxb.explore_win_device against the yardstick, every candidate materialised by
pxb.explore_win_rows and pushed through pxb.run_scripted and pxb.cover, with the
predicate, the two-axis subset rule and pxb.explore_win_reach_of in Python
(explore_win_oracle.brute): ids, counts, reach records and status exactly
equal.  Then the ties to pxb.explore_cover, the device form's cursor and
guards, the host form's chunking and one pass over every kernel unit."""
import json

import numpy as np
import pytest

import cover_oracle as CO
import explore_cover_oracle as XC
import explore_oracle as X
import explore_win_oracle as XW
import pxb
from test_explore_gpu import UNIT_SHAPES

pytestmark = pytest.mark.gpu
GPU = dict(runner=pxb._run_scripted_runner, coverer=XC.gpu_coverer)
BIT = CO.BIT


def explore_win_both(cfg, parents, depth, sd, R, grid, query, mask):
    """pxb.explore_win in both listing modes against the yardstick; the minimal-mode outputs."""
    want = XW.brute(cfg, parents, depth, sd, R, grid, query, mask, **GPU)
    out = None
    for minimal in (False, True):
        out = pxb.explore_win(cfg, parents, depth, sd, R, grid, query, mask, minimal=minimal)
        XW.check(*out, want, minimal)
    return out, want


# ---- 1. the pinned shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_pinned_shapes(gpu_lib, name):
    """(a): T_w = 469 x 289 = 135,541, two windows, the parent's end inside a
    wave and all 12 cells populated; (b): T_w = 73 x 1,153 = 84,169, the recorded
    findings; (d): log mode, N = 2, two windows.  What the yardstick gives is
    asserted, two-window candidates that do not run OK included."""
    cfg, row, depth, sd, R, grid, Tw = XW.shape(name)
    assert pxb.explore_win_total(cfg, sd, R, grid) == Tw and Tw % 64 != 0
    for q, mask in XC.QUERIES.values():
        (ids, n, counts, reach, status), want = explore_win_both(cfg, row, depth, sd, R, grid, q, mask)
    if name == "a":
        assert (counts[0, :, :3, 0] > 0).all() and not counts[0, :, 3].any()      # 3 x 3 cells of this space
    kat = json.load(open(XW.KAT_PATH))["shapes"][name]
    assert XW.findings(name, **GPU) == kat
    r = pxb.explore_win(cfg, row, depth, sd, R, grid)[3][0]
    dist = pxb.reach_distance_win(r)
    assert pxb.cover_names(r.parent_mask) == kat["parent"]
    assert {n_: {"distance": dist[pxb.COVER_BIT[n_]], "cells": {"%d,%d" % k: {"first": f, "count": c} for k, (f, c) in cells.items()}}
            for n_, cells in r.by_name().items()} == kat["classes"]


def test_all_twelve_cells(gpu_lib):
    """Shape (a)'s config at link radius 3 with one start and two windows: every
    one of the 3 x 4 cells has candidates that ran OK."""
    cfg, row, depth, sd, _, _, _ = XW.shape("a")
    grid = pxb.WinGrid(2, 1, 1, open=True, radius=2)
    assert pxb.explore_win_total(cfg, sd, 3, grid) == 19 * 2049
    (ids, n, counts, reach, status), want = explore_win_both(cfg, row, depth, sd, 3, grid, *XC.QUERIES["cover"])
    assert (counts[0, :, :, 0] > 0).all() and n > 0


# ---- 2. the ties to pxb.explore_cover ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_no_window_radius_is_explore_cover(gpu_lib, name):
    """win_radius = 0: ids, counts[0], reach[0] and status are pxb.explore_cover's exactly."""
    cfg, row, depth, sd, R, T = X.shape(name)
    grid = pxb.WinGrid(0, 6, 3, open=True, radius=0)
    assert pxb.explore_win_total(cfg, sd, R, grid) == T
    for q, mask in XC.QUERIES.values():
        for minimal in (False, True):
            w = pxb.explore_win(cfg, row, depth, sd, R, grid, q, mask, minimal=minimal)
            c = pxb.explore_cover(cfg, row, depth, sd, R, q, mask, minimal=minimal)
            assert w[1] == c[1] and np.array_equal(w[0], c[0]) and np.array_equal(w[4], c[4])
            assert np.array_equal(w[2][:, 0], c[2]) and not w[2][:, 1:].any()
            rw, rc = XW.reach_records(w[3])[0], XC.reach_records(c[3])[0]
            assert np.array_equal(rw["count"][0], rc["count"]) and not rw["count"][1:].any()
            assert np.array_equal(rw["first"][0].min(axis=0), rc["first"]) and (rw["first"][1:] == pxb.REACH_NONE).all()
            assert rw["parent_mask"] == rc["parent_mask"] and rw["union_mask"] == rc["union_mask"]


def test_block_h_is_explore_cover_on_the_written_parent(gpu_lib):
    """Block h of a parent equals pxb.explore_cover on that parent with the
    windows written into the row: the held lists and the {ran OK, held} counts.
    Minimal differs by design (the joint rule also looks at fewer windows): the
    joint minimal set of the block is a subset of the per-parent one."""
    cfg, row, depth, sd, R, grid, Tw = XW.shape("b")
    T = pxb.explore_total(cfg, sd, R)
    q, mask = XC.QUERIES["both"]
    held = pxb.explore_win(cfg, row, depth, sd, R, grid, q, mask, minimal=False)
    mini = pxb.explore_win(cfg, row, depth, sd, R, grid, q, mask, minimal=True)
    smaller = 0
    for h in (0, 1, 10, 28, 49, 72):
        written = pxb.explore_win_rows(cfg, row, depth, sd, R, grid, [h * T])[0]
        c_held = pxb.explore_cover(cfg, written, depth, sd, R, q, mask, minimal=False)
        c_mini = pxb.explore_cover(cfg, written, depth, sd, R, q, mask, minimal=True)
        block = lambda ids: ids[(ids // np.uint64(T)) == h] - np.uint64(h * T)  # noqa: E731
        assert np.array_equal(block(held[0]), c_held[0]) and len(c_held[0]) > 0
        if h == 0:                                       # the cells of r_w = 0 are this one block
            assert np.array_equal(held[2][0, 0, :, :2], c_held[2][0, :, :2])
        assert set(block(mini[0]).tolist()) <= set(c_mini[0].tolist())
        smaller += len(block(mini[0])) < len(c_mini[0])
    assert smaller > 0                                   # (the joint rule does drop what a window variant lists again)
    # the {ran OK, held} counts of r_w = 1 are the sums over the 72 one-window parents
    written = pxb.explore_win_rows(cfg, row, depth, sd, R, grid, np.arange(1, 73) * T)
    sums = pxb.explore_cover(cfg, written, depth, sd, R, q, mask, minimal=False)[2][:, :, :2].sum(axis=0)
    assert np.array_equal(held[2][0, 1, :, :2], sums)


# ---- 3. five parents in one call -----------------------------------------------------------------------
def test_five_parents(gpu_lib):
    """The benign row, a malformed row, an extracted row with explicit windows,
    a row with keep windows, the benign row again: parent boundaries inside
    waves; the bad parent's neighbours are unaffected and the repeated parent
    gives an equal record."""
    cfg, parents, depth, sd, R, grid, Tw = XW.five_parents()
    assert Tw % 64 != 0
    q, mask = XC.QUERIES["cover"]
    (ids, n, counts, reach, status), want = explore_win_both(cfg, parents, depth, sd, R, grid, q, mask)
    assert list(status) == [0, pxb.SCRIPT_BAD, 0, 0, 0] and not counts[1].any()
    bad = XW.reach_records(reach)[1]
    assert not bad["count"].any() and (bad["first"] == pxb.REACH_NONE).all() and bad["parent_mask"] == 0 == bad["union_mask"]
    assert reach[0] == reach[4] and reach[0] != reach[2] and (counts[0] == counts[4]).all()
    alone = pxb.explore_win(cfg, parents[0], depth, sd, R, grid, q, mask)
    assert alone[3][0] == reach[0] and (alone[2][0] == counts[0]).all()
    per = [ids[ids // np.uint64(Tw) == i] - np.uint64(i * Tw) for i in range(5)]
    assert len(per[0]) and np.array_equal(per[0], per[4]) and np.array_equal(per[0], alone[0]) and len(per[1]) == 0
    assert (np.diff(ids.astype(np.int64)) > 0).all()


# ---- 4. the device form ------------------------------------------------------------------------------------
def device_call(cfg, parents, depth, sd, R, grid, query, mask, minimal, capacity, first_parent=0, d_ids=None, d_n=None,
                stream=None, want_reach=True):
    import torch
    dev = torch.device("cuda:0")
    rows = pxb._script_rows(cfg, parents, depth)
    n = len(rows)
    d_rows = torch.from_numpy(rows.reshape(-1).copy()).to(dev)
    if d_n is None:
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    if d_ids is None and capacity:
        d_ids = torch.full((capacity + 8,), -7, dtype=torch.int64, device=dev)
    # (guard words behind every output: nothing past the call's share is touched)
    d_counts = torch.full((n * 36 + 8,), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    d_reach = torch.full((n * pxb.EXPLORE_WIN_REACH_BYTES + 64,), 0x5A, dtype=torch.uint8, device=dev) if want_reach else None
    pxb.explore_win_device(cfg, d_rows, n, depth, sd, R, grid, d_n, query=query, flag_mask=mask, d_ids=d_ids,
                           capacity=capacity, d_counts=d_counts[:n * 36], d_reach=d_reach[:n * pxb.EXPLORE_WIN_REACH_BYTES]
                           if want_reach else None, d_status=d_status[:n], first_parent=first_parent, minimal=minimal,
                           stream=stream)
    return d_rows, d_ids, d_n, d_counts, d_reach, d_status


def outputs(d_counts, d_reach, d_status, n):
    c, s = d_counts.cpu().numpy(), d_status.cpu().numpy()
    assert (c[n * 36:] == -7).all() and (s[n:] == -7).all()
    rec = None
    if d_reach is not None:
        raw = d_reach.cpu().numpy()
        assert (raw[n * pxb.EXPLORE_WIN_REACH_BYTES:] == 0x5A).all()
        rec = raw[:n * pxb.EXPLORE_WIN_REACH_BYTES].view(pxb.win_reach_dtype())
    return c[:n * 36].view(np.uint32).reshape(n, 3, 4, 3), rec, s[:n].view(np.uint32)


def test_capacity_and_cursor(gpu_lib):
    import torch
    cfg, parents, depth, sd, R, grid, Tw = XW.five_parents()
    q, mask = XC.QUERIES["cover"]
    want = XW.brute(cfg, parents, depth, sd, R, grid, q, mask, **GPU)
    held = want["held"].astype(np.int64)
    k = len(held)
    assert k > 100
    # capacity 0: sizes only
    _, d_ids, d_n, d_counts, d_reach, d_status = device_call(cfg, parents, depth, sd, R, grid, q, mask, False, 0)
    torch.cuda.synchronize()
    counts, rec, status = outputs(d_counts, d_reach, d_status, 5)
    assert d_ids is None and int(d_n.item()) == k
    assert np.array_equal(counts, want["counts"]) and np.array_equal(status, want["status"])
    assert rec.tobytes() == want["reach"].tobytes()
    # a capacity below the matches: the first 100, the guard values past them untouched; a null d_reach
    _, d_ids, d_n, d_counts, _, d_status = device_call(cfg, parents, depth, sd, R, grid, q, mask, False, 100, want_reach=False)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == k and np.array_equal(got[:100], held[:100]) and (got[100:] == -7).all()
    counts, _, status = outputs(d_counts, None, d_status, 5)
    assert np.array_equal(counts, want["counts"]) and np.array_equal(status, want["status"])
    # two calls, first_parent 0 and 5, append to one list through the cursor
    d_ids = torch.full((2 * k + 16,), -7, dtype=torch.int64, device="cuda:0")
    _, _, d_n, _, _, _ = device_call(cfg, parents, depth, sd, R, grid, q, mask, False, 2 * k + 16, d_ids=d_ids)
    device_call(cfg, parents, depth, sd, R, grid, q, mask, False, 2 * k + 16, first_parent=5, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == 2 * k and np.array_equal(got[:2 * k], np.concatenate([held, held + 5 * Tw])) and (got[2 * k:] == -7).all()
    # a cursor already past the capacity: counted, nothing written
    d_ids.fill_(-7)
    d_n.fill_(5)
    m = len(want["minimal"])
    device_call(cfg, parents, depth, sd, R, grid, q, mask, True, 4, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == 5 + m and (d_ids.cpu().numpy() == -7).all()
    # ids past 2^32: the records' `first` stay c' < T_w
    fp = (1 << 32) // Tw + 7
    _, d_ids, d_n, _, d_reach, _ = device_call(cfg, parents[0], depth, sd, R, grid, q, mask, True, 4, first_parent=fp)
    torch.cuda.synchronize()
    one = XW.brute(cfg, parents[0], depth, sd, R, grid, q, mask, **GPU)
    assert int(d_n.item()) == len(one["minimal"]) >= 4
    assert list(d_ids.cpu().numpy()[:5]) == [fp * Tw + int(c) for c in one["minimal"][:4]] + [-7]
    assert d_reach.cpu().numpy()[:pxb.EXPLORE_WIN_REACH_BYTES].tobytes() == one["reach"].tobytes()
    # count == 0
    d_rows = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    before = int(d_n.item())
    pxb.explore_win_device(cfg, d_rows, 0, depth, sd, R, grid, d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == before
    assert pxb.explore_win(cfg, np.zeros((0, parents.shape[1]), np.uint8), depth, sd, R, grid)[1] == 0


# ---- 5. host-form chunking ----------------------------------------------------------------------------------
def test_host_form_chunks(gpu_lib):
    """PXB_EXPLORE_CHUNK = 15,000 with the five parents (T_w = 6,775): two
    parents a chunk, three chunks; 1: a parent a chunk.  Every output equals the
    one-chunk call's."""
    cfg, parents, depth, sd, R, grid, Tw = XW.five_parents()
    q, mask = XC.QUERIES["both"]
    whole = pxb.explore_win(cfg, parents, depth, sd, R, grid, q, mask, minimal=False)
    assert whole[1] > 50 and whole[0][-1] >= 4 * Tw
    for chunk in (15000, 1):
        with pxb.hooks(PXB_EXPLORE_CHUNK=chunk):
            got = pxb.explore_win(cfg, parents, depth, sd, R, grid, q, mask, minimal=False)
            part = pxb.explore_win(cfg, parents, depth, sd, R, grid, q, mask, minimal=False, capacity=50)
        assert got[1] == whole[1] and got[3] == whole[3]
        assert all(np.array_equal(a, b) for a, b in zip((got[0], got[2], got[4]), (whole[0], whole[2], whole[4])))
        assert part[1] == whole[1] and np.array_equal(part[0], whole[0][:50]) and part[3] == whole[3]


# ---- 6. every kernel unit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,delay_max", UNIT_SHAPES)
def test_every_kernel_unit(gpu_lib, P, N, delay_max):
    """test_explore_gpu's shapes (every proposer-count unit with the smallest and
    the largest acceptor count, and the 16-step wheel) at radius 1, win_radius
    1, grid (0, 2, 1), for the wiring: ids in both modes, counts, reach and
    status equal the host build's (tests/native/explore_win_host.cpp) exactly."""
    cfg, parents, depth, sd, R = XC.unit_case(P, N, delay_max)
    grid = pxb.WinGrid(0, 2, 1, radius=1)
    q = pxb.CoverQuery(any_mask=BIT["PROPOSE_NACK"] | BIT["HAVE_BELOW"] | BIT["DISCARD_DEAD"] | BIT["R1OK_STALE"] |
                       BIT["ASK_NACK"] | BIT["DISCARD_ISOLATED"])
    for minimal in (False, True):
        h = XW.host_explore_win(cfg, parents, depth, sd, R, grid, q, 0, minimal=minimal)
        ids, n, counts, reach, status = pxb.explore_win(cfg, parents, depth, sd, R, grid, q, 0, minimal=minimal)
        assert n == h["n"] and np.array_equal(ids, h["ids"])
        assert np.array_equal(counts, h["counts"]) and np.array_equal(status, h["status"])
        assert XW.reach_records(reach).tobytes() == h["reach"].tobytes()
    assert (status == pxb.TRACE_OK).all() and reach[0].union != 0 and reach[1].union != 0 and n > 0
    assert counts[:, 1, :2, 0].all()                      # one-window candidates ran OK at both link radii
