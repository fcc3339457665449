"""Test-side helpers for pxb_explore_win (docs/SEMANTICS.md §17).

* ``brute``: the yardstick.  Every non-skipped candidate of every parent
  materialised by pxb.explore_win_rows; status, flags and send counts from a
  scripted runner (script_oracle.host_runner, or pxb.run_scripted on the GPU);
  masks from a cover function (cover_oracle.host_cover, or pxb.cover); then the
  predicate, the two-axis subset rule (``subset_table``) and
  pxb.explore_win_reach_of in Python.  ``run_all`` asserts that it compared
  every candidate but the skipped ones, and is computed once per key.
* ``host_explore_win``: the host build of the shared logic
  (tests/native/explore_win_host.cpp).
* ``check``: an implementation's outputs against the yardstick, exactly.
* the shapes and parents the tests share.  No tests here."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np

import explore_cover_oracle as XC
import explore_oracle as X
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "explore_win_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libexplore_win_host.so")
DEPS = sorted(set([d for d in XC.DEPS if not d.endswith("explore_cover_host.cpp")] + [
    SRC, os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", "explore_win_core.h")]))
KAT_PATH = os.path.join(HERE, "golden", "kat_explore_win.json")
RAN, HELD, MINIMAL = X.RAN, X.HELD, X.MINIMAL
_lib = None
_brutes = {}


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def lib():
    global _lib
    if _lib is None:
        if stale(OUT):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run([SO.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", tmp, SRC],
                           check=True, timeout=900)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _lib.explore_win_host_total.argtypes = [u32, u32, u32, vp]
        _lib.explore_win_host_total.restype = u64
        _lib.explore_win_host_check.argtypes = [u32, u32, u32, vp]
        _lib.explore_win_host_check.restype = u64
        _lib.explore_win_host_unrank.argtypes = [u32, u32, u32, vp, vp, u64, vp]
        _lib.explore_win_host_run.argtypes = [vp, vp, u64, u32, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    return _lib


def space_c(sd, R, grid, query=None, flag_mask=0, minimal=True):
    return pxb._explore_win_space(sd, R, grid, query, flag_mask, minimal)


def host_unrank(cfg, sd, R, grid, c):
    """(n, 12) uint32: r_w, acc[2], wdigit[2], r_l, site[3], digit[3] of the candidates c."""
    c = np.ascontiguousarray(c, dtype=np.uint64)
    out = np.zeros((len(c), 12), dtype=np.uint32)
    sp = space_c(sd, R, grid)
    assert lib().explore_win_host_unrank(cfg.n_proposers, cfg.n_acceptors, cfg.delay_max, C.addressof(sp), c.ctypes.data,
                                         len(c), out.ctypes.data) == 0
    return out


def host_explore_win(cfg, parents, depth, sd, R, grid, query=None, flag_mask=0, minimal=True, capacity=None,
                     first_parent=0):
    """explore_win_host_run: a dict of ids, n, counts (n, 3, 4, 3), reach (n,)
    records, status, bytes (n, T_w), masks (n, T_w)."""
    rows = pxb._script_rows(cfg, parents, depth)
    n, T = len(rows), pxb.explore_win_total(cfg, sd, R, grid)
    o = {"counts": np.full((n, 3, 4, 3), 99, np.uint32), "status": np.full(n, 99, np.uint32),
         "bytes": np.full((n, T), 0xA5, np.uint8), "masks": np.full((n, T), 0xA5A5A5A5, np.uint32),
         "reach": np.zeros(n, pxb.win_reach_dtype())}
    o["reach"].view(np.uint8)[:] = 0xA5
    c = cfg.to_c(0, 1)
    sp = space_c(sd, R, grid, query, flag_mask, minimal)
    nm = C.c_uint64(0)

    def call(ids, cap):
        nm.value = 0
        rc = lib().explore_win_host_run(C.addressof(c), rows.ctypes.data, n, depth, C.addressof(sp), first_parent,
                                        ids.ctypes.data if cap else None, cap, C.addressof(nm),
                                        o["counts"].ctypes.data, o["reach"].ctypes.data, o["status"].ctypes.data,
                                        o["bytes"].ctypes.data, o["masks"].ctypes.data)
        assert rc == 0, "explore_win_host_run rc=%d" % rc
    if capacity is None:
        call(None, 0)
        capacity = nm.value
    ids = np.zeros(capacity, np.uint64)
    call(ids, capacity)
    o["ids"], o["n"] = ids[:min(nm.value, capacity)], nm.value
    return o


def radii(cfg, sd, R, grid):
    """(r_w (T_w,), r_l (T_w,)) of every candidate c'."""
    T = pxb.explore_total(cfg, sd, R)
    H = pxb.explore_win_total(cfg, sd, R, grid) // T
    S, A = 2 * cfg.n_proposers * cfg.n_acceptors * sd, cfg.delay_max
    r_l = pxb._explore_unrank_many(S, A, R, np.arange(T))[0]
    r_w = pxb._win_unrank_many(cfg.n_acceptors, grid, np.arange(H))[0]
    return np.repeat(r_w, T), np.tile(r_l, H)


def win_subset_table(N, grid):
    """(rank (4, H), valid (4, H)): for every window choice and every `sub` in
    0..3, the choice made of the changed acceptors whose bit is set in `sub` (with
    their digits); valid where `sub` is a subset of the choice's changes.  Written
    out with numpy, independent of the C++ code."""
    W = grid.W
    base = pxb._win_bases(N, W, grid.radius) + [0, 0]
    H = base[grid.radius + 1]
    r, acc, dig = pxb._win_unrank_many(N, grid, np.arange(H))
    rank, valid = np.zeros((4, H), np.int64), np.zeros((4, H), bool)
    for sub in range(4):
        pick = [i for i in range(2) if sub >> i & 1]
        valid[sub] = sub < (1 << r)
        if len(pick) == 0:
            continue
        if len(pick) == 1:
            rank[sub] = base[1] + acc[:, pick[0]] * W + dig[:, pick[0]]
        else:
            rank[sub] = base[2] + (acc[:, 0] + acc[:, 1] * (acc[:, 1] - 1) // 2) * W * W + dig[:, 0] + dig[:, 1] * W
        rank[sub] = np.where(valid[sub], rank[sub], 0)
    return r, rank, valid


def run_all(cfg, parents, depth, sd, R, grid, runner=SO.host_runner, coverer=XC.host_coverer, chunk=1 << 15):
    """(ran (n, T_w) bool, flags, masks, status (n,)): every candidate of every
    parent run as a materialised row; the mask of a candidate that did not run OK
    is 0.  No sampling: the number of rows run equals n T_w minus the skipped
    candidates and the bad parents' ones."""
    rows = pxb._script_rows(cfg, parents, depth)
    key = ("run", repr(cfg), rows.tobytes(), depth, sd, R, grid, runner, coverer)
    if key in _brutes:
        return _brutes[key]
    n, T = len(rows), pxb.explore_win_total(cfg, sd, R, grid)
    status = np.array([pxb.SCRIPT_BAD if (r[8] > cfg.n_proposers or r[9]) else pxb.TRACE_OK for r in rows], np.uint32)
    g = np.arange(n * T, dtype=np.uint64)
    skipped = pxb.explore_win_skipped(cfg, rows, depth, sd, R, grid, g)
    run = ~skipped & (status[g // np.uint64(T)] == pxb.TRACE_OK)
    ran, flags, masks = np.zeros(n * T, bool), np.zeros(n * T, np.uint32), np.zeros(n * T, np.uint32)
    todo, compared = g[run], 0
    for a in range(0, len(todo), chunk):
        w = todo[a:a + chunk]
        cand = pxb.explore_win_rows(cfg, rows, depth, sd, R, grid, w)
        res, st, sent = runner(cfg, cand, depth)
        ok = (np.asarray(st) == pxb.TRACE_OK) & (np.asarray(sent).reshape(len(w), -1).max(axis=1) <= depth)
        m, mst = coverer(cfg, cand, depth)
        assert np.array_equal(np.asarray(mst), np.asarray(st))
        wi = w.astype(np.int64)
        ran[wi], flags[wi], masks[wi] = ok, np.asarray(res)[:, 3] & 0xFF, np.where(ok, m, 0)
        compared += len(w)
    good = int((status == pxb.TRACE_OK).sum())
    assert compared == good * T - int(skipped.reshape(n, T)[status == pxb.TRACE_OK].sum())
    _brutes[key] = (ran.reshape(n, T), flags.reshape(n, T), masks.reshape(n, T), status)
    return _brutes[key]


def brute(cfg, parents, depth, sd, R, grid, query=None, flag_mask=0, runner=SO.host_runner, coverer=XC.host_coverer):
    """The yardstick: a dict of bytes (n, T_w) with the ran / held / minimal bits,
    masks, counts (n, 3, 4, 3), reach (n,) records, status (n,), held and minimal
    (ascending global ids)."""
    q = query or pxb.CoverQuery()
    ran, flags, masks, status = run_all(cfg, parents, depth, sd, R, grid, runner, coverer)
    n, Tw = ran.shape
    T = pxb.explore_total(cfg, sd, R)
    H = Tw // T
    S, A = 2 * cfg.n_proposers * cfg.n_acceptors * sd, cfg.delay_max
    match = ((masks & q.all_mask) == q.all_mask) & ((masks & q.none_mask) == 0)
    if q.any_mask:
        match &= (masks & q.any_mask) != 0
    held = ran & match
    if flag_mask:
        held &= (flags & flag_mask) != 0
    by = (ran * RAN + held * HELD).astype(np.uint8)
    _, lrank, lvalid = X.subset_table(S, A, R)          # (7, T): the proper subsets of the link changes
    rw_of, wrank, wvalid = win_subset_table(cfg.n_acceptors, grid)   # (4, H): the subsets of the window changes
    r_w, r_l = radii(cfg, sd, R, grid)
    for i in range(n):
        hd = held[i].reshape(H, T)
        smaller = np.zeros((H, T), bool)                 # another candidate made of subsets holds
        for sw in range(4):
            sub_w = hd[wrank[sw]]                        # (H, T): held of (subset sw of h's windows, c)
            for sl in range(7):                          # fewer link changes, any subset of the windows
                smaller |= wvalid[sw][:, None] & lvalid[sl][None, :] & sub_w[:, lrank[sl]]
            proper_w = wvalid[sw] & (sw < (1 << rw_of) - 1)
            smaller |= proper_w[:, None] & sub_w         # all the link changes, fewer windows
        by[i, held[i] & ~smaller.reshape(-1)] |= MINIMAL
    counts = np.zeros((n, 3, 4, 3), np.uint32)
    for a in range(3):
        for l in range(4):
            cell = (r_w == a) & (r_l == l)
            for b in range(3):
                counts[:, a, l, b] = ((by[:, cell] >> b) & 1).sum(axis=1)
    reach = np.zeros(n, pxb.win_reach_dtype())
    for i in range(n):
        reach[i] = pxb.explore_win_reach_of(masks[i], ran[i], r_w, r_l)
    flat = by.reshape(-1)
    return {"bytes": by, "masks": masks, "counts": counts, "reach": reach, "status": status,
            "held": np.nonzero(flat & HELD)[0].astype(np.uint64), "minimal": np.nonzero(flat & MINIMAL)[0].astype(np.uint64)}


def reach_records(reach):
    """A list of pxb.ExploreWinReach, or an array of records, as an array of records."""
    if isinstance(reach, np.ndarray):
        return reach
    out = np.zeros(len(reach), pxb.win_reach_dtype())
    out["first"][:] = pxb.REACH_NONE
    for i, r in enumerate(reach):
        out["count"][i, :, :, :29], out["first"][i, :, :, :29] = r.counts, r.first
        out["parent_mask"][i], out["union_mask"][i] = r.parent_mask, r.union
        assert r.tail_ok
    return out


def check(got_ids, got_n, counts, reach, status, want, minimal, first_parent=0, T=0):
    """ids, n_matches, counts, reach and status against the yardstick, exactly."""
    X.check(got_ids, got_n, counts, status, want, minimal, first_parent, T)
    reach = reach_records(reach)
    assert reach.tobytes() == want["reach"].tobytes(), [
        (i, k) for i in range(len(reach)) for k in reach.dtype.names if not np.array_equal(reach[i][k], want["reach"][i][k])]


# ---- what the tests share -----------------------------------------------------------------------
GRID_A = pxb.WinGrid(0, 4, 2, open=True, radius=2)
GRID_B = pxb.WinGrid(0, 6, 3, open=True, radius=1)
# name: (explore_oracle's shape, link radius, grid, T_w); the GPU tests' pinned shapes
SHAPES = {"a": ("a", 2, GRID_A, 469 * 289), "b": ("b", 2, GRID_B, 73 * 1153), "d": ("d", 1, GRID_A, 169 * 49)}
# the same at link radius 1 for the host lane, which runs a candidate at a time
HOST_SHAPES = {"a": ("a", 1, GRID_A, 469 * 25), "b": ("b", 1, GRID_B, 73 * 49), "d": ("d", 1, GRID_A, 169 * 49)}


def shape(name, table=SHAPES):
    """(cfg, benign parent row, depth, site_depth, radius, grid, T_w)."""
    base, R, grid, Tw = table[name]
    cfg, row, depth, sd, _, _ = X.shape(base)
    return cfg, row, depth, sd, R, grid, Tw


CRASH_CFG = dataclasses.replace(X.CFG_A, seed=0x5EED0171, crash_ppm=600000, crash_len_max=6, crash_start_max=6)


def five_parents(R=1, grid=pxb.WinGrid(0, 3, 2, open=True, radius=2)):
    """(cfg, parents, depth, site_depth, radius, grid, T_w) over shape (a)'s
    config with a crash rate: the benign row, a malformed row (reserved byte
    set), an extracted row that carries explicit windows (which the candidates
    replace), the benign row with keep windows (the instance's own draws), and
    the benign row again.  T_w = 271 x 25 = 6,775."""
    cfg, depth, sd = CRASH_CFG, 16, 2
    row = X.benign_row(cfg, depth)
    bad = row.copy()
    bad[9] = 1
    ex = SO.host_extract(cfg, np.arange(32), depth)
    has = [r for r in ex if (pxb.script_windows(cfg, r[None, :])[0, :, 1] > pxb.script_windows(cfg, r[None, :])[0, :, 0]).any()]
    assert has, "no extracted row of CRASH_CFG carries a window"
    keep = row.copy()
    pxb.script_base(keep[None, :])[0] = 5
    pxb.script_windows(cfg, keep[None, :])[:] = 0xFFFF
    return cfg, np.stack([row, bad, has[0], keep, row]), depth, sd, R, grid, pxb.explore_win_total(cfg, sd, R, grid)


# ---- the pinned findings (tests/golden/kat_explore_win.json) ---------------------------------------
def findings(name, **kw):
    """Of a pinned shape's benign parent, from the yardstick: per reached class
    its reach distance and per populated cell "r_w,r_l" the first c' and the
    count; the parent's classes; the cells' ran-OK counts."""
    cfg, row, depth, sd, R, grid, Tw = shape(name)
    w = brute(cfg, row, depth, sd, R, grid, **kw)
    r = pxb.ExploreWinReach.from_record(w["reach"][0])
    dist = pxb.reach_distance_win(r)
    return {"T_w": Tw, "parent": pxb.cover_names(r.parent_mask),
            "ran_ok": {"%d,%d" % (a, l): int(w["counts"][0, a, l, 0]) for a in range(3) for l in range(4)
                       if w["counts"][0, a, l, 0]},
            "classes": {n: {"distance": dist[pxb.COVER_BIT[n]],
                            "cells": {"%d,%d" % k: {"first": f, "count": c} for k, (f, c) in cells.items()}}
                        for n, cells in r.by_name().items()}}


if __name__ == "__main__":                           # python tests/explore_win_oracle.py: rewrite the recorded results
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    with open(KAT_PATH, "w") as f:
        json.dump({"about": "pxb_explore_win: per pinned shape of tests/explore_win_oracle.py (benign parent), the reach "
                            "record of the brute-force yardstick: per reached class its reach distance and, per "
                            "populated (r_w, r_l) cell, the first candidate c' and the count",
                   "shapes": {n: findings(n) for n in ("a", "b", "d")}}, f, indent=1)
        f.write("\n")
