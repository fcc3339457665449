"""pxb_explore_win (docs/SEMANTICS.md §17) without a GPU.

The logic the kernels share (csrc/explore_win_core.h: the window space, its
unrank and rank, the overwrite of a started lane's windows, the two-axis
minimality test) is compiled for the HOST (tests/native/explore_win_host.cpp)
and checked: the index is a bijection, exhaustively; the C++ unrank, total and
row equal the Python mirror's; the host build equals brute force (every
non-skipped candidate materialised by pxb.explore_win_rows and run by the host
builds of the scripted lane and of the coverage lane; predicate, subset rule and
reach in numpy).  Then the pinned findings, the C-ABI boundary of the new entry
points, and one stand-alone AddressSanitizer + UBSan program (its own main;
nothing sanitized is loaded into Python)."""
import ctypes as C
import dataclasses
import itertools
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import explore_cover_oracle as XC
import explore_oracle as X
import explore_win_oracle as XW
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "explore_win_host_san")


def cfg_of(P, N, A=2):
    return pxb.Config(seed=1, n_proposers=P, n_acceptors=N, delay_max=A, step_cap=64)


# grids with W = 1, 2 and 12 alternatives per acceptor
GRIDS = {1: dict(first=3, starts=1, lens=1, open=False), 2: dict(first=0, starts=1, lens=1, open=True),
         12: dict(first=5, starts=4, lens=2, open=True)}


# ---- 1. the index ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 9])
@pytest.mark.parametrize("W", [1, 2, 12])
def test_index_is_a_bijection(N, W):
    """rank(unrank(c')) == c' for every c' of the space, window radius 0..2, over
    small link spaces (one proposer, site_depth 1, link radius 0..2), checked in
    C++; the totals equal Python's and the library's."""
    cfg = cfg_of(1, N)
    fn = pxb._win_fn("pxb_explore_win_total")
    for wr, R in itertools.product(range(3), range(3)):
        grid = pxb.WinGrid(radius=wr, **GRIDS[W])
        assert grid.W == W
        sp = XW.space_c(1, R, grid)
        Tw = pxb.explore_win_total(cfg, 1, R, grid)
        import math
        assert Tw == sum(math.comb(N, q) * W ** q for q in range(wr + 1)) * pxb.explore_total(cfg, 1, R) > 0
        args = (1, N, cfg.delay_max, C.addressof(sp))
        assert XW.lib().explore_win_host_total(*args) == Tw == fn(*args)
        assert XW.lib().explore_win_host_check(*args) == 0


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_unrank_equals_pythons(name):
    """The C++ unrank of every candidate of the pinned host shapes equals
    pxb.explore_win_unrank (spot rows) and the vectorised mirror (all rows)."""
    cfg, row, depth, sd, R, grid, Tw = XW.shape(name, XW.HOST_SHAPES)
    assert pxb.explore_win_total(cfg, sd, R, grid) == Tw
    T = pxb.explore_total(cfg, sd, R)
    cs = np.arange(Tw)
    got = XW.host_unrank(cfg, sd, R, grid, cs)
    r_w, acc, dig = pxb._win_unrank_many(cfg.n_acceptors, grid, cs // T)
    r_l, sites, digits = pxb._explore_unrank_many(2 * cfg.n_proposers * cfg.n_acceptors * sd, cfg.delay_max, R, cs % T)
    want = np.concatenate([r_w[:, None], acc, dig, r_l[:, None], sites, digits], axis=1)
    assert np.array_equal(got, want.astype(np.uint32))
    rw, rl = XW.radii(cfg, sd, R, grid)
    assert np.array_equal(rw, r_w) and np.array_equal(rl, r_l)
    for c in list(range(0, Tw, max(1, Tw // 97))) + [Tw - 1]:
        (a, d), (s, j) = pxb.explore_win_unrank(cfg, sd, R, grid, c)
        g = got[c]
        assert (a, d) == (list(g[1:1 + g[0]]), list(g[3:3 + g[0]])) and (s, j) == (list(g[6:6 + g[5]]), list(g[9:9 + g[5]]))
        wins, links = pxb.explore_win_changes(cfg, sd, R, grid, c)
        assert [w[0] for w in wins] == a and all(0 <= c0 < c1 <= 4096 for _, c0, c1 in wins)
        assert links == pxb.explore_changes(cfg, sd, R, c % T)
    assert pxb.explore_win_changes(cfg, sd, R, grid, T)[0] == [(0, 0, 1)] and pxb.explore_win_changes(cfg, sd, R, grid, 0) == ([], [])
    with pytest.raises(ValueError):
        pxb.explore_win_unrank(cfg, sd, R, grid, Tw)


def test_totals():
    """pxb_explore_win_total equals Python's, including the invalid spaces and
    more than 2^30 candidates (0)."""
    fn = pxb._win_fn("pxb_explore_win_total")
    cfg = X.CFG_B

    def both(sd, R, grid, cfg_=cfg):
        sp = XW.space_c(sd, R, grid)
        t = fn(cfg_.n_proposers, cfg_.n_acceptors, cfg_.delay_max, C.addressof(sp))
        assert t == pxb.explore_win_total(cfg_, sd, R, grid) == XW.lib().explore_win_host_total(
            cfg_.n_proposers, cfg_.n_acceptors, cfg_.delay_max, C.addressof(sp))
        return t
    assert both(2, 2, XW.GRID_B) == 73 * 1153 and both(2, 2, XW.GRID_A, X.CFG_A) == 469 * 289
    assert both(2, 2, pxb.WinGrid(0, 1, 1, radius=0)) == 1153                 # no window changes: T
    assert both(2, 3, pxb.WinGrid(0, 256, 255, open=True, radius=1)) == 0     # (1 + 3 x 65,536) x 17,345 > 2^30
    assert both(2, 1, pxb.WinGrid(0, 256, 255, open=True, radius=1)) == 196609 * 49
    assert both(2, 0, pxb.WinGrid(0, 2048, 15, open=True, radius=2)) == 0     # H alone: 3 x 32,768^2 > 2^30
    assert both(2, 0, pxb.WinGrid(0, 4096, 0, open=True, radius=2)) == 1 + 3 * 4096 + 3 * 4096 ** 2
    assert both(2, 1, pxb.WinGrid(0, 0, 1)) == 0                              # W = 0: no start
    assert both(2, 1, pxb.WinGrid(0, 2, 0)) == 0                              # W = 0: no length
    assert both(2, 1, pxb.WinGrid(0, 2, 0, open=True)) == 7 * 49
    assert both(2, 1, pxb.WinGrid(0, 2, 1, radius=3)) == 0                    # win_radius > 2
    assert both(2, 1, pxb.WinGrid(4000, 90, 8)) == 0 and both(2, 1, pxb.WinGrid(4000, 90, 7)) == (1 + 3 * 630) * 49   # the 4096 bound
    assert both(0, 1, XW.GRID_B) == 0 and both(2, 4, XW.GRID_B) == 0          # the link part's own rules
    assert fn(2, 3, 2, None) == 0


def test_row_equals_pythons():
    """pxb_explore_win_row equals pxb.explore_win_rows byte for byte: every
    candidate of host shape (b) over an extracted parent with explicit and keep
    windows; in place; c >= T_w, a changed keep site and a null row refused."""
    cfg, _, depth, sd, R, grid, Tw = XW.shape("b", XW.HOST_SHAPES)
    fn = pxb._win_fn("pxb_explore_win_row")
    parent = X.benign_row(cfg, depth).copy()
    win = pxb.script_windows(cfg, parent[None, :])
    win[0, 0], win[0, 1] = (3, 9), (0xFFFF, 0xFFFF)
    pxb.script_links(cfg, parent[None, :], depth)[0, 1, 1, 2, 0] = 0xFF      # one keep site
    c_ = cfg.to_c(0, 1)
    sp = XW.space_c(sd, R, grid)
    ids = np.arange(Tw, dtype=np.uint64)
    skipped = pxb.explore_win_skipped(cfg, parent, depth, sd, R, grid, ids)
    assert 0 < skipped.sum() < Tw
    want = pxb.explore_win_rows(cfg, parent, depth, sd, R, grid, ids[~skipped])
    out = np.zeros(len(parent), np.uint8)
    k = 0
    for c in range(Tw):
        out[:] = 0x5A
        rc = fn(C.byref(c_), depth, C.byref(sp), parent.ctypes.data, c, out.ctypes.data)
        if skipped[c]:
            assert rc == pxb.PXB_E_INVAL and (out == 0x5A).all()
        else:
            assert rc == 0 and out.tobytes() == want[k].tobytes(), c
            k += 1
    assert k == len(want)
    with pytest.raises(ValueError):
        pxb.explore_win_rows(cfg, parent, depth, sd, R, grid, ids[skipped][:1])
    T = pxb.explore_total(cfg, sd, R)
    h = 1 + 24 + 5                                                              # acceptor 1, digit 5: start 1, length 2
    row = pxb.explore_win_rows(cfg, parent, depth, sd, R, grid, [h * T])[0]
    assert pxb.script_windows(cfg, row[None, :])[0].tolist() == [[3, 9], [1, 3], [0, 0]]   # the keep pair is replaced
    row = pxb.explore_win_rows(cfg, parent, depth, sd, R, grid, [(1 + 3) * T])[0]
    assert pxb.script_windows(cfg, row[None, :])[0].tolist() == [[0, 4096], [0xFFFF, 0xFFFF], [0, 0]]   # the open one
    inplace = parent.copy()
    assert fn(C.byref(c_), depth, C.byref(sp), inplace.ctypes.data, h * T + 1, inplace.ctypes.data) == 0
    assert inplace.tobytes() == pxb.explore_win_rows(cfg, parent, depth, sd, R, grid, [h * T + 1])[0].tobytes()
    assert fn(C.byref(c_), depth, C.byref(sp), parent.ctypes.data, Tw, out.ctypes.data) == pxb.PXB_E_INVAL
    assert fn(C.byref(c_), depth, C.byref(sp), None, 0, out.ctypes.data) == pxb.PXB_E_INVAL
    assert fn(C.byref(c_), depth, None, parent.ctypes.data, 0, out.ctypes.data) == pxb.PXB_E_INVAL


# ---- 2. the host build against the brute ------------------------------------------------------------
def host_against_brute(cfg, parents, depth, sd, R, grid, query, flag_mask, **kw):
    """The host build in both listing modes against the yardstick, exactly:
    bytes, masks, ids, n, counts, reach, status.  Returns the minimal-mode dict."""
    want = XW.brute(cfg, parents, depth, sd, R, grid, query, flag_mask)
    out = None
    Tw = pxb.explore_win_total(cfg, sd, R, grid)
    for minimal in (False, True):
        o = XW.host_explore_win(cfg, parents, depth, sd, R, grid, query, flag_mask, minimal=minimal, **kw)
        assert np.array_equal(o["bytes"], want["bytes"]) and np.array_equal(o["masks"], want["masks"])
        XW.check(o["ids"], o["n"], o["counts"], o["reach"], o["status"], want, minimal, kw.get("first_parent", 0), Tw)
        out = o
    return out


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_host_build_equals_brute(name):
    """The host shapes ((a) with two windows, (b) with one, (d) in log mode with
    two) with a cover-only query, a flag-only predicate and both.  XW.run_all
    asserts that every candidate but the skipped ones was compared."""
    cfg, row, depth, sd, R, grid, Tw = XW.shape(name, XW.HOST_SHAPES)
    held = {}
    for key, (q, mask) in XC.QUERIES.items():
        o = host_against_brute(cfg, row, depth, sd, R, grid, q, mask)
        held[key] = int(o["counts"][0, :, :, 1].sum())
        print(name, key, "held", held[key], "minimal", int(o["counts"][0, :, :, 2].sum()), "n", o["n"])
        assert o["counts"][0, :, :, 2].sum() <= held[key]
    assert held["both"] > 0 and held["cover"] > 0 and (held["flag"] > 0 or name == "d")   # (the queries are not vacuous)


def test_minimal_is_joint():
    """A failure that needs no window is listed once, not once per window
    variant; one that needs only a window is not listed again under link changes."""
    cfg, row, depth, sd, R, grid, Tw = XW.shape("b", XW.HOST_SHAPES)
    T = pxb.explore_total(cfg, sd, R)
    q = pxb.CoverQuery(all_mask=XC.BIT["Q1_FOREIGN_ACCEPT"])
    o = XW.host_explore_win(cfg, row, depth, sd, R, grid, q, 0, minimal=True)
    link_only = XC.host_explore_cover(cfg, row, depth, sd, R, q, 0, minimal=True)
    assert link_only["n"] > 0
    assert np.array_equal(o["ids"][o["ids"] < T], link_only["ids"])           # block h = 0: the link-only minimal ones
    held = (o["bytes"][0].reshape(-1, T) & XW.HELD) != 0
    for g in o["ids"]:
        h, c = divmod(int(g), T)
        assert not (h and held[0, c]) and not (c and held[h, 0]) and not held[0, 0]
    per_variant = sum(int(XC.host_explore_cover(cfg, pxb.explore_win_rows(cfg, row, depth, sd, R, grid, [h * T])[0], depth, sd,
                                                R, q, 0)["n"]) for h in range(0, 73, 8))
    assert per_variant > link_only["n"]                                       # what the composed search lists again


@pytest.mark.parametrize("all_mask", [0, XC.BIT["Q1_FOREIGN_ACCEPT"]])
def test_no_window_radius_is_the_cover_build(all_mask):
    """The link-only space is the joint space with one window choice: over a
    grid of radius 0 (H = 1, r_w = 0) the host win build equals the host cover
    build, on shape (b) at link radius 2 (T = 1,153), with the all-zero query and
    with all = Q1_FOREIGN_ACCEPT."""
    cfg, row, depth, sd, R, _, _ = XW.shape("b")
    grid = pxb.WinGrid(0, 1, 1, radius=0)
    assert pxb.explore_win_total(cfg, sd, R, grid) == pxb.explore_total(cfg, sd, R) == 1153
    q = pxb.CoverQuery(all_mask=all_mask) if all_mask else None
    w = XW.host_explore_win(cfg, row, depth, sd, R, grid, q, 0)
    c = XC.host_explore_cover(cfg, row, depth, sd, R, q, 0)
    assert np.array_equal(w["bytes"], c["bytes"]) and np.array_equal(w["ids"], c["ids"])
    assert w["n"] == c["n"] and np.array_equal(w["status"], c["status"])
    assert w["n"] > 0 and np.array_equal(w["masks"], c["masks"])
    assert np.array_equal(w["counts"][:, 0], c["counts"]) and not w["counts"][:, 1:].any()
    wr, cr = w["reach"], c["reach"]
    assert np.array_equal(wr["count"][:, 0], cr["count"]) and not wr["count"][:, 1:].any()
    assert np.array_equal(wr["first"][:, 0].min(axis=1), cr["first"]) and (wr["first"][:, 1:] == pxb.REACH_NONE).all()
    assert np.array_equal(wr["parent_mask"], cr["parent_mask"]) and np.array_equal(wr["union_mask"], cr["union_mask"])
    assert cr["union_mask"][0] != 0


def test_five_parents_on_the_host():
    """A malformed parent, a parent with explicit windows and one with keep
    windows among good ones; first_parent; a capacity below the matches."""
    cfg, parents, depth, sd, R, grid, Tw = XW.five_parents()
    assert Tw == 271 * 25
    q, mask = XC.QUERIES["cover"]
    o = host_against_brute(cfg, parents, depth, sd, R, grid, q, mask, first_parent=3)
    assert list(o["status"]) == [0, pxb.SCRIPT_BAD, 0, 0, 0]
    bad = o["reach"][1]
    assert not bad["count"].any() and (bad["first"] == pxb.REACH_NONE).all() and bad["parent_mask"] == 0 == bad["union_mask"]
    assert not o["counts"][1].any()
    assert o["reach"][0].tobytes() == o["reach"][4].tobytes() and o["reach"][0].tobytes() != o["reach"][2].tobytes()
    # where every acceptor's window is replaced nothing of the parent's windows is left: the keep
    # parent (base 5) differs from the benign one only there, and in its Philox base, which no explicit link reads
    o2 = XW.host_explore_win(cfg, parents, depth, sd, R, grid, q, mask, capacity=5, first_parent=3)
    assert o2["n"] == o["n"] > 5 and np.array_equal(o2["ids"], o["ids"][:5])


# ---- 3. the pinned findings ----------------------------------------------------------------------------
def test_pinned_findings():
    """tests/golden/kat_explore_win.json, shape (b) with grid (0, 6, 3, open):
    what one isolation window reaches with NO link change, against the host
    build at link radius 0 and 1 (the file's cells of link radius <= 1), and the
    link-only cells against kat_explore_cover.json."""
    kat = json.load(open(XW.KAT_PATH))["shapes"]
    b = kat["b"]["classes"]
    T2, grid = 1153, XW.GRID_B

    def window_only(c):                                  # c' of a window-only candidate -> (acceptor, c0, c1)
        assert c % T2 == 0
        return pxb.explore_win_changes(X.CFG_B, 2, 2, grid, c)[0]
    for name, win in (("EXEC_PANIC", (0, 2, 4)), ("DISCARD_DEAD", (0, 2, 4)), ("Q7_STALE_EXEC", (0, 4, 6)),
                      ("DISCARD_ISOLATED", (0, 0, 2))):
        assert b[name]["distance"] == 1 and "0,0" not in b[name]["cells"], name
        assert window_only(b[name]["cells"]["1,0"]["first"]) == [win], name
    assert "0,1" not in b["EXEC_PANIC"]["cells"] and "0,2" in b["EXEC_PANIC"]["cells"]        # links alone need two
    assert not any(k.startswith("0,") for k in b["Q7_STALE_EXEC"]["cells"])                  # links alone: not within 2
    assert not any(k.startswith("0,") for k in b["DISCARD_ISOLATED"]["cells"])
    assert kat["b"]["ran_ok"]["1,0"] == 72 and kat["b"]["ran_ok"]["0,0"] == 1                # all 73 window-only candidates ran
    # the link-only cells (r_w = 0) are kat_explore_cover.json's
    cover = json.load(open(XC.KAT_PATH))["shapes"]
    for s, R in (("a", 2), ("b", 2), ("d", 1)):
        for name, rec in cover[s]["classes"].items():
            cells = kat[s]["classes"].get(name, {"cells": {}})["cells"]
            assert [cells.get("0,%d" % r, {"count": 0})["count"] for r in range(R + 1)] == rec["count"][:R + 1], (s, name)
            if rec["distance"] <= R:
                assert cells["0,%d" % rec["distance"]]["first"] == rec["first"], (s, name)   # (T_w's block 0 is T's order)
        assert kat[s]["parent"] == cover[s]["parent"]
    # the host build gives the file's cells of link radius <= 1
    for s in ("a", "b", "d"):
        cfg, row, depth, sd, R, g, Tw = XW.shape(s, XW.HOST_SHAPES)
        T_file, T = pxb.explore_total(cfg, sd, XW.SHAPES[s][1]), pxb.explore_total(cfg, sd, R)
        r = pxb.ExploreWinReach.from_record(XW.host_explore_win(cfg, row, depth, sd, R, g)["reach"][0])
        got = {n: {"%d,%d" % k: {"first": f // T * T_file + f % T, "count": c} for k, (f, c) in cells.items()}
               for n, cells in r.by_name().items()}
        want = {n: {k: v for k, v in rec["cells"].items() if int(k[2]) <= R} for n, rec in kat[s]["classes"].items()}
        assert got == {n: v for n, v in want.items() if v}, s


# ---- 4. the C-ABI boundary ------------------------------------------------------------------------------
def test_validation_without_a_device_call():
    L = pxb.load()
    cfg, row, depth, sd, R, grid, Tw = XW.shape("a")
    rows = np.stack([row, row])
    buf = np.zeros(2048, np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    host, dev = pxb._win_fn("pxb_explore_win"), pxb._win_fn("pxb_explore_win_device")
    OPEN = pxb.EXPLORE_WIN_OPEN

    def calls(cfg_=cfg, cflags=0, rows_p=P(rows), count=2, depth_=depth, space=(sd, R, 0, 1 | OPEN), q=(0, 0, 0, 0),
              win=(2, 0, 4, 2), ids_p=P(buf), cap=8, nm_p=P(buf[16:]), counts_p=None, reach_p=None, status_p=None,
              which=(0, 1)):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= cflags
        cp = C.byref(c) if c is not None else None
        sp = pxb.pxb_explore_win_space(*space, pxb.pxb_cover_query(*q), *win) if space is not None else None
        spp = C.byref(sp) if sp is not None else None
        fns = (lambda: host(cp, rows_p, count, depth_, spp, ids_p, cap, nm_p, counts_p, reach_p, status_p),
               lambda: dev(cp, rows_p, count, depth_, spp, 0, ids_p, cap, nm_p, counts_p, reach_p, status_p, None))
        return [fns[i]() for i in which]

    def inval(**kw):
        got = calls(**kw)
        return len(got) > 0 and all(rc == pxb.PXB_E_INVAL for rc in got)
    # the window fields
    assert inval(win=(2, 0, 0, 2))                                        # W = 0: no start
    assert inval(win=(2, 0, 4, 0), space=(sd, R, 0, 1))                   # W = 0: no length without WIN_OPEN
    assert inval(win=(3, 0, 4, 2))                                        # win_radius > 2
    assert inval(win=(1, 4000, 90, 8)) and inval(win=(1, 4097, 1, 0)) and inval(win=(1, 0, 1, 4097))   # the 4096 bound
    assert inval(win=(1, 0xFFFFFFFF, 2, 1))                               # (no wrap-around)
    assert inval(win=(2, 0, 2048, 15))                                    # T_w > 2^30 (H alone)
    assert inval(win=(2, 0, 4096, 0))                                     # T_w > 2^30 (H T)
    assert inval(win=(2, 0, 64, 63), space=(sd, 3, 0, 1 | OPEN))          # T_w > 2^30 (H T)
    assert inval(space=(sd, R, 0, 4)) and inval(space=(sd, R, 0, 1 | OPEN | 8))   # unknown flags bits
    assert inval(count=(1 << 32) // Tw + 1, which=(1,))                   # count x T_w > 2^32
    # pxb_explore_cover_device's rules
    assert inval(cfg_=None) and inval(space=None)
    assert inval(rows_p=None) and inval(nm_p=None) and inval(ids_p=None)
    assert inval(depth_=4097, space=(4097, R, 0, 1))
    assert inval(space=(0, R, 0, 1)) and inval(space=(depth + 1, R, 0, 1)) and inval(space=(sd, 4, 0, 1))
    assert inval(space=(sd, R, 0x100, 1)) and inval(q=(0, 0, 0, 1)) and inval(cflags=pxb.CFG_TRACE_PRODUCTION)
    assert inval(count=(1 << 30) + 1)
    off = lambda k: C.c_void_p(buf.ctypes.data + k)  # noqa: E731
    assert inval(rows_p=C.c_void_p(rows.ctypes.data + 4), which=(1,))
    assert inval(ids_p=off(4), which=(1,)) and inval(nm_p=off(4), which=(1,))
    assert inval(counts_p=off(2), which=(1,)) and inval(status_p=off(2), which=(1,))
    assert inval(reach_p=off(512 + 4), which=(1,))                        # a misaligned d_reach
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0)):
        assert inval(cfg_=bad), bad
    hdr = open(os.path.join(X.ROOT, "include", "paxos_batch.h")).read()
    assert re.search(r"typedef struct pxb_explore_win_space \{\s+/\* 48 B", hdr)
    assert re.search(r"typedef struct pxb_explore_win_reach \{\s+/\* 3080 B", hdr)
    assert C.sizeof(pxb.pxb_explore_win_space) == 48 and C.sizeof(pxb.pxb_explore_win_reach) == 3080 == pxb.win_reach_dtype().itemsize
    assert L.pxb_abi_version() == 5 and pxb.ABI_VERSION == 5
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_explore_win", "pxb_explore_win_device", "pxb_explore_win_row", "pxb_explore_win_total"):
        assert " T %s\n" % name in out and hasattr(L, name)
    import torch
    if not torch.cuda.is_available():                                     # valid calls, no GPU
        assert calls(which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(space=(sd, R, X.PANIC, 0), q=(1, 2, 4, 0), win=(0, 7, 1, 1), reach_p=off(512), which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=0, rows_p=None, cap=0, ids_p=None, which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=(1 << 32) // Tw + 1, which=(0,)) == [pxb.PXB_E_NODEV]   # (the host form walks in chunks)
        with pytest.raises(pxb.PaxosError):
            pxb.explore_win(cfg, row, depth, sd, R, grid)


def test_struct_sizes_in_c(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "paxos_batch.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(pxb_explore_win_space), sizeof(pxb_explore_win_reach),
         offsetof(pxb_explore_win_space, q), offsetof(pxb_explore_win_space, win_radius),
         offsetof(pxb_explore_win_reach, first), offsetof(pxb_explore_win_reach, parent_mask),
         offsetof(pxb_explore_win_reach, union_mask));
  return 0;
}'''
    tmp = str(tmp_path / "pxb_exw_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(X.ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True).stdout.split()]
    assert got == [48, 3080, pxb.pxb_explore_win_space.q.offset, pxb.pxb_explore_win_space.win_radius.offset,
                   pxb.pxb_explore_win_reach.first.offset, pxb.pxb_explore_win_reach.parent_mask.offset,
                   pxb.pxb_explore_win_reach.union_mask.offset] == [48, 3080, 16, 32, 1536, 3072, 3076]


def test_python_argument_checks():
    cfg, row, depth, sd, R, grid, Tw = XW.shape("a")
    import torch
    n = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="required"):
        pxb.explore_win_device(cfg, None, 1, depth, sd, R, grid, None)
    with pytest.raises(ValueError, match="CUDA"):
        pxb.explore_win_device(cfg, torch.zeros(len(row), dtype=torch.uint8), 1, depth, sd, R, grid, n)
    with pytest.raises(ValueError, match="no such space"):
        pxb.explore_win_rows(cfg, row, depth, sd, R, pxb.WinGrid(0, 0, 1), [0])
    z = np.zeros(10, np.uint32)
    rec = pxb.explore_win_reach_of(z, np.ones(10, bool), z, z)
    assert pxb.reach_distance_win(rec) == [None] * 29 and (rec["first"] == pxb.REACH_NONE).all()
    m = np.array([1, 0, 3, 2, 2], np.uint32)
    rec = pxb.explore_win_reach_of(m, [1, 1, 1, 0, 1], [0, 0, 1, 1, 2], [0, 1, 0, 3, 1])
    assert pxb.reach_distance_win(rec)[:2] == [0, 1] and rec["count"][1, 0, 1] == 1 and rec["first"][2, 1, 1] == 4
    assert rec["count"][1, 3].sum() == 0 and rec["union_mask"] == 3 and rec["parent_mask"] == 1
    assert pxb.WinGrid(0, 6, 3, open=True).window(3) == (0, 4096) and pxb.WinGrid(0, 6, 3, open=True).window(5) == (1, 3)


# ---- 5. one stand-alone sanitizer program ------------------------------------------------------------------
SAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAIN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_EXPLORE_WIN_HOST_MAIN",
              "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_explore_win_core_sanitized():
    """explore_win_host.cpp with its own main (one shape: P = 1, N = 3, W = 8)
    under AddressSanitizer + UBSan, as a subprocess over the five parents, every
    buffer sized exactly: exit status 0, the bijection check passes there, and
    the output equals the library build's."""
    if XW.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([SO.HIPCC, *MAIN_FLAGS, *SAN_FLAGS, "-o", tmp, XW.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    cfg, parents, depth, sd, R, grid, Tw = XW.five_parents()
    q, mask = XC.QUERIES["both"]
    sp = XW.space_c(sd, R, grid, q, mask, True)
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
        with open(inp, "wb") as f:
            f.write(bytes(cfg.to_c(0, 1)) + bytes(sp) + np.array([depth], np.uint32).tobytes() +
                    np.array([len(parents)], np.uint64).tobytes() + parents.tobytes())
        e = dict(os.environ)
        e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
        p = subprocess.run([EXE, inp, out], capture_output=True, text=True, env=e, timeout=600)
        assert p.returncode == 0, "%s failed (rc %d): %s" % (EXE, p.returncode, p.stderr[-4000:])
        got = np.fromfile(out, dtype=np.uint8)
    o = XW.host_explore_win(cfg, parents, depth, sd, R, grid, q, mask, minimal=True)
    want = np.concatenate([np.zeros(8, np.uint8), o["bytes"].reshape(-1), o["masks"].reshape(-1).view(np.uint8),
                           o["counts"].reshape(-1).view(np.uint8), o["reach"].view(np.uint8), o["status"].view(np.uint8),
                           np.array([o["n"]], np.uint64).view(np.uint8), o["ids"].view(np.uint8)])
    assert len(want) == len(got) and (want == got).all()
    assert o["n"] > 0
