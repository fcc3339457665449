"""Test-side helpers for the explorer (docs/SEMANTICS.md §12).

* ``host_explore``: the host build of the explorer's shared logic
  (tests/native/explore_host.cpp), pxb_explore_device's arguments and outputs
  plus the candidates' flag bytes.
* ``brute``: the yardstick.  Every candidate of every parent materialised by
  pxb.explore_rows and run by a scripted runner (the host lane, or
  pxb.run_scripted on the GPU), the predicate and the subset rule in Python;
  computed once per (config, parents, space, mask, runner) and shared.
* ``check``: an explorer's outputs against the yardstick, exactly.
* the shapes (a) to (d) the tests pin numbers for.
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np

import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "explore_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libexplore_host.so")
DEPS = [SRC, os.path.join(HERE, "native", "host_lane.h"), os.path.join(HERE, "native", "explore_host.h")] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "paxos_trace_core.h", "ev_layouts.h",
              "lane_shapes.h", "script_core.h", "script_lane.h", "shrink_core.h", "explore_core.h",
              "explore_cover_core.h", "cover_core.h", "events_core.h")] + [     # (explore_host.h includes the last three)
                  os.path.join(ROOT, "include", "paxos_batch.h")]
RAN, HELD, MINIMAL = 1, 2, 4
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
        vp = C.c_void_p
        _lib.explore_host_total.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        _lib.explore_host_total.restype = C.c_uint64
        _lib.explore_host_check.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        _lib.explore_host_check.restype = C.c_uint64
        _lib.explore_host_unrank.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp]
        _lib.explore_host_run.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]
    return _lib


def host_unrank(S, A, R, c):
    """(n, 7) uint32: r, site[3], digit[3] of the candidates c."""
    c = np.ascontiguousarray(c, dtype=np.uint64)
    out = np.zeros((len(c), 7), dtype=np.uint32)
    assert lib().explore_host_unrank(S, A, R, c.ctypes.data, len(c), out.ctypes.data) == 0
    return out


def host_explore(cfg, parents, depth, site_depth, radius, flag_mask, minimal=True, capacity=None, first_parent=0):
    """explore_host_run: a dict of ids, n, counts (n, 4, 3), status, bytes (n, T)."""
    rows = pxb._script_rows(cfg, parents, depth)
    n, T = len(rows), pxb.explore_total(cfg, site_depth, radius)
    o = {"counts": np.full((n, 4, 3), 99, np.uint32), "status": np.full(n, 99, np.uint32),
         "bytes": np.full((n, T), 0xA5, np.uint8)}
    c = cfg.to_c(0, 1)
    sp = pxb.pxb_explore_space(site_depth, radius, flag_mask, pxb.EXPLORE_MINIMAL if minimal else 0)
    nm = C.c_uint64(0)

    def call(ids, cap):
        nm.value = 0
        rc = lib().explore_host_run(C.addressof(c), rows.ctypes.data, n, depth, C.addressof(sp), first_parent,
                                    ids.ctypes.data if cap else None, cap, C.addressof(nm), o["counts"].ctypes.data,
                                    o["status"].ctypes.data, o["bytes"].ctypes.data)
        assert rc == 0, "explore_host_run rc=%d" % rc
    if capacity is None:
        call(None, 0)
        capacity = nm.value
    ids = np.zeros(capacity, np.uint64)
    call(ids, capacity)
    o["ids"], o["n"] = ids[:min(nm.value, capacity)], nm.value
    return o


def benign_row(cfg, depth, base=0):
    """The explicit all-benign row: n_proposers = P, skews 0, no windows, every link byte 1."""
    row = pxb.scripts_empty(cfg, [base], depth)
    pxb.script_n_proposers(row)[0] = cfg.n_proposers
    pxb.script_skews(row)[:] = 0
    pxb.script_windows(cfg, row)[:] = 0
    pxb.script_links(cfg, row, depth)[:] = 1
    return row[0]


def subset_table(S, A, radius):
    """(r (T,), rank (7, T), valid (7, T)): for every candidate and every
    `sub` in 0..6, the candidate made of the changes whose bit is set in `sub`
    (with their digits), valid where that is a proper subset (sub < 2^r - 1; the
    empty one, candidate 0, included).  The combinatorial number system written
    out with numpy, independent of the C++ code."""
    base = pxb._explore_bases(S, A, radius)
    T = base[-1]
    r, sites, digits = pxb._explore_unrank_many(S, A, radius, np.arange(T))
    comb = [None, lambda s: s, lambda s: s * (s - 1) // 2, lambda s: s * (s - 1) * (s - 2) // 6]
    rank, valid = np.zeros((7, T), np.int64), np.zeros((7, T), bool)
    for sub in range(7):
        pick = [i for i in range(3) if sub >> i & 1]
        valid[sub] = sub < (1 << r) - 1
        if len(pick) > radius:
            continue
        m = sum((comb[q + 1](sites[:, i]) for q, i in enumerate(pick)), np.zeros(T, np.int64))
        v = sum((digits[:, i] * A ** q for q, i in enumerate(pick)), np.zeros(T, np.int64))
        rank[sub] = np.where(valid[sub], base[len(pick)] + m * A ** len(pick) + v, 0)
    return r, rank, valid


def brute(cfg, parents, depth, site_depth, radius, flag_mask, runner=SO.host_runner, chunk=1 << 15):
    """The yardstick: a dict of bytes (n, T) with the ran / held / minimal bits,
    counts (n, 4, 3), status (n,), held and minimal (ascending global ids)."""
    rows = pxb._script_rows(cfg, parents, depth)
    key = (repr(cfg), rows.tobytes(), depth, site_depth, radius, flag_mask, runner)
    if key in _brutes:
        return _brutes[key]
    n, T = len(rows), pxb.explore_total(cfg, site_depth, radius)
    S, A = 2 * cfg.n_proposers * cfg.n_acceptors * site_depth, cfg.delay_max
    status = np.array([pxb.SCRIPT_BAD if (r[8] > cfg.n_proposers or r[9]) else pxb.TRACE_OK for r in rows], np.uint32)
    g = np.arange(n * T, dtype=np.uint64)
    run = ~pxb.explore_skipped(cfg, rows, depth, site_depth, radius, g) & (status[g // np.uint64(T)] == pxb.TRACE_OK)
    by = np.zeros(n * T, np.uint8)
    todo = g[run]
    for a in range(0, len(todo), chunk):
        w = todo[a:a + chunk]
        res, st, sent = runner(cfg, pxb.explore_rows(cfg, rows, depth, site_depth, radius, w), depth)
        ok = (np.asarray(st) == pxb.TRACE_OK) & (np.asarray(sent).reshape(len(w), -1).max(axis=1) <= depth)
        held = ok & ((np.asarray(res)[:, 3] & 0xFF & flag_mask) != 0)
        by[w.astype(np.int64)] = ok * RAN + held * HELD
    by = by.reshape(n, T)
    r_of, rank, valid = subset_table(S, A, radius)
    for i in range(n):
        held = (by[i] & HELD) != 0
        smaller = np.zeros(T, bool)                    # a proper subset of the changes holds
        for sub in range(7):
            smaller |= valid[sub] & held[rank[sub]]
        by[i, held & ~smaller] |= MINIMAL
    counts = np.zeros((n, 4, 3), np.uint32)
    for r in range(radius + 1):
        for b in range(3):
            counts[:, r, b] = ((by[:, r_of == r] >> b) & 1).sum(axis=1)
    flat = by.reshape(-1)
    _brutes[key] = {"bytes": by, "counts": counts, "status": status, "held": np.nonzero(flat & HELD)[0].astype(np.uint64),
                    "minimal": np.nonzero(flat & MINIMAL)[0].astype(np.uint64)}
    return _brutes[key]


def check(got_ids, got_n, counts, status, want, minimal, first_parent=0, T=0):
    """ids, n_matches, counts and status of an explorer against the yardstick."""
    ids = want["minimal" if minimal else "held"] + np.uint64(first_parent * T)
    assert got_n == len(ids), (got_n, len(ids))
    assert np.array_equal(np.asarray(got_ids, dtype=np.uint64), ids)
    assert np.array_equal(counts, want["counts"]), (counts, want["counts"])
    assert np.array_equal(status, want["status"])


# ---- the pinned shapes -----------------------------------------------------------------------
CFG_A = pxb.Config(seed=0xE1, n_proposers=1, n_acceptors=3, delay_max=2, step_cap=256)
CFG_B = dataclasses.replace(CFG_A, n_proposers=2)
CFG_D = pxb.Config(seed=0xE4, n_proposers=2, n_acceptors=2, delay_max=2, step_cap=256, n_ticks=3, tick_period=8)
# name: (cfg, depth, site_depth, radius, T)
SHAPES = {"a": (CFG_A, 16, 2, 3, 2049), "b": (CFG_B, 16, 2, 3, 17345), "d": (CFG_D, 32, 3, 2, 1153)}
STUCK, PANIC, LOG_DIV = 0x2, 0x4, 0x8
_id10 = {}


def shape(name):
    """(cfg, parent row, depth, site_depth, radius, T)."""
    if name == "c":
        cfg = pxb.CONFIGS[3]
        if "row" not in _id10:
            _id10["row"] = pxb.shrink(cfg, SO.host_extract(cfg, [10], 64)[0], pxb.F_PANIC, runner=SO.host_runner,
                                      depth=64)[0]
        return cfg, _id10["row"], 64, 2, 2, 12641
    cfg, depth, sd, R, T = SHAPES[name]
    return cfg, benign_row(cfg, depth), depth, sd, R, T
