"""The explorer (docs/SEMANTICS.md §12) without a GPU.

The logic the explore kernels share (csrc/explore_core.h: the candidate space,
unrank and rank, ExploreByte and ExploreDraws over the per-lane state machine,
the keep-site test, minimality) is compiled for the HOST
(tests/native/explore_host.cpp) and checked against the pure Python functions of
pxb and against brute force: every candidate materialised by pxb.explore_rows
and run by the host build of the scripted lane, the subset rule in Python.  Then
the C-ABI boundary of the new entry points, and one stand-alone AddressSanitizer
+ UBSan program (its own main; nothing is loaded into Python)."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import explore_oracle as X
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "explore_host_san")


# ---- 1. the index is a bijection --------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 5, 12, 24])
def test_index_is_a_bijection(S):
    """Exhaustively in C++: rank(unrank(c)) == c, ascending sites below S, digits
    below A, the radius of c's interval.  The C++ unrank equals the vectorised
    Python one on every candidate of the spaces up to 2^16 (a fixed sample and
    the interval ends beyond), and pxb.explore_unrank, the scalar specification,
    on a sample of those."""
    rng = np.random.default_rng(S)
    for A in (1, 2, 4, 15):
        for R in range(4):
            T = pxb._explore_bases(S, A, R)[-1]
            assert X.lib().explore_host_total(S, A, R) == T
            assert X.lib().explore_host_check(S, A, R) == 0, (S, A, R)
            base = pxb._explore_bases(S, A, R)
            ends = [c for b in base for c in (b - 1, b) if 0 <= c < T]
            c = np.arange(T) if T <= 1 << 16 else np.unique(np.concatenate([rng.integers(0, T, 1 << 14), ends]))
            got = X.host_unrank(S, A, R, c)
            r, sites, digits = pxb._explore_unrank_many(S, A, R, c)
            assert np.array_equal(got[:, 0], r) and np.array_equal(got[:, 1:4], sites) and np.array_equal(got[:, 4:], digits)
            for j in np.unique(np.concatenate([rng.integers(0, len(c), 64), [0, len(c) - 1]])):
                s, d = pxb.explore_unrank(S, A, R, int(c[j]))
                assert (list(got[j, 1:1 + got[j, 0]]), list(got[j, 4:4 + got[j, 0]])) == (s, d), (S, A, R, c[j])
                assert s == sorted(set(s)) and all(x < A for x in d)


def test_index_of_a_large_space():
    """S = 432 (P = 3, N = 9, site_depth 8), A = 2, R = 3: the first and the last
    candidate of every radius, against pxb.explore_changes; and the totals."""
    cfg = pxb.Config(seed=1, n_proposers=3, n_acceptors=9, delay_max=2)
    S, A, R = 432, 2, 3
    base = pxb._explore_bases(S, A, R)
    assert pxb.explore_total(cfg, 8, R) == base[-1] == X.lib().explore_host_total(S, A, R)
    c = [x for r in range(R + 1) for x in (base[r], base[r + 1] - 1)]
    got = X.host_unrank(S, A, R, c)
    for j, cc in enumerate(c):
        r = j // 2
        ch = pxb.explore_changes(cfg, 8, R, cc)
        assert got[j, 0] == r == len(ch)
        sites = [((dirn * 3 + p) * 9 + a) * 8 + k for dirn, p, a, k, _ in ch]
        assert sites == list(got[j, 1:1 + r]) and [x[4] for x in ch] == list(got[j, 4:4 + r])
        # the first of a radius: sites 0..r-1, digits 0; the last: the top r sites, digits A - 1
        assert sites == (list(range(r)) if j % 2 == 0 else list(range(S - r, S)))
        assert [x[4] for x in ch] == [0 if j % 2 == 0 else A - 1] * r
    assert pxb.explore_changes(cfg, 8, R, 0) == []
    L = pxb.load()
    assert L.pxb_explore_total(3, 9, 2, 8, 3) == base[-1]
    # T beyond 2^30: S = 3456, A = 15, R = 3
    big = pxb.Config(seed=1, n_proposers=3, n_acceptors=9, delay_max=15)
    assert pxb._explore_bases(3456, 15, 3)[-1] > 1 << 30
    assert L.pxb_explore_total(3, 9, 15, 64, 3) == 0 == pxb.explore_total(big, 64, 3) == X.lib().explore_host_total(3456, 15, 3)
    assert L.pxb_explore_total(3, 9, 15, 64, 1) == 1 + 3456 * 15
    for bad in ((0, 3, 2, 2, 1), (4, 3, 2, 2, 1), (1, 10, 2, 2, 1), (1, 3, 0, 2, 1), (1, 3, 16, 2, 1), (1, 3, 2, 0, 1),
                (1, 3, 2, 4097, 1), (1, 3, 2, 2, 4)):
        assert L.pxb_explore_total(*bad) == 0, bad


# ---- 2. pxb_explore_row equals pxb.explore_rows ---------------------------------------------------
def _explore_row(cfg, depth, site_depth, radius, parent, c):
    out = np.full(len(parent), 0xA5, np.uint8)
    cc = cfg.to_c(0, 1)
    sp = pxb.pxb_explore_space(site_depth, radius, 0, 0)
    rc = pxb.load().pxb_explore_row(C.byref(cc), depth, C.byref(sp), parent.ctypes.data, c, out.ctypes.data)
    return rc, out


def test_explore_row_equals_explore_rows():
    cfg, row, depth, sd, R, T = X.shape("a")
    row = row.copy()
    pxb.script_links(cfg, row[None, :], depth)[0, 1, 0, 2, 1] = 7      # (a byte above delay_max: min(b, A) applies)
    pxb.script_links(cfg, row[None, :], depth)[0, 0, 0, 1, 0] = 0
    want = pxb.explore_rows(cfg, row, depth, sd, R, np.arange(T))
    assert want.shape == (T, len(row)) and (want[0] == row).all()
    for c in range(T):
        rc, out = _explore_row(cfg, depth, sd, R, row, c)
        assert rc == 0 and (out == want[c]).all(), c
    # every value in 0..A but the parent's own, at the changed sites only
    off = pxb.script_links_off(cfg)
    assert [int(x) for x in want[1:5, off]] == [2, 0, 1, 1]            # site 0 (byte 1): digits 0 and 1; then site 1
    assert [int(x) for x in want[5:7, off + depth]] == [1, 2]          # site 2 (byte 0: lost)
    assert [int(x) for x in want[23:25, off + 5 * depth + 1]] == [0, 1]   # site 11 (byte 7: as delay_max)
    assert _explore_row(cfg, depth, sd, R, row, T)[0] == pxb.PXB_E_INVAL
    # a changed keep site: PXB_E_INVAL, nothing written; the candidates beside it are fine
    row[pxb.script_links_off(cfg) + 1] = 0xFF                          # site 1: link 0, seq 1
    skipped = pxb.explore_skipped(cfg, row, depth, sd, R, np.arange(T))
    assert skipped[3] and skipped[4] and not skipped[1] and not skipped[0] and skipped.sum() == 2 + 11 * 4 + 55 * 8
    for c in (3, 4, int(np.nonzero(skipped)[0][-1])):
        rc, out = _explore_row(cfg, depth, sd, R, row, c)
        assert rc == pxb.PXB_E_INVAL and (out == 0xA5).all()
        with pytest.raises(ValueError):
            pxb.explore_rows(cfg, row, depth, sd, R, [c])
    assert _explore_row(cfg, depth, sd, R, row, 1)[0] == 0


# ---- 3. host explore agrees with brute force -------------------------------------------------------
def held_by_radius(o):
    return [int(x) for x in o["counts"][0, :, 1]]


def minimal_by_radius(o):
    return [int(x) for x in o["counts"][0, :, 2]]


def both_modes(name, mask):
    """Host explore of a pinned shape in both listing modes, checked against
    brute force: bytes, counts, status and ids.  Returns the minimal-mode dict."""
    cfg, row, depth, sd, R, T = X.shape(name)
    assert pxb.explore_total(cfg, sd, R) == T
    want = X.brute(cfg, row, depth, sd, R, mask)
    out = None
    for minimal in (False, True):
        o = X.host_explore(cfg, row, depth, sd, R, mask, minimal=minimal)
        assert np.array_equal(o["bytes"], want["bytes"]), (name, mask)
        X.check(o["ids"], o["n"], o["counts"], o["status"], want, minimal)
        out = o
    print(name, hex(mask), "T", T, "ran", int(out["counts"][0, :, 0].sum()), "held", held_by_radius(out), "minimal",
          minimal_by_radius(out), "first", list(out["ids"][:3]))
    return out


def test_shape_a():
    """P1, N3, delay_max 2, depth 16, site_depth 2, R 3: T = 2,049, none past depth."""
    o = both_modes("a", X.PANIC)
    assert int(o["counts"][0, :, 0].sum()) == 2049
    assert held_by_radius(o) == [0, 3, 45, 294] and list(o["ids"]) == [4, 8, 12]
    assert pxb.explore_changes(X.CFG_A, 2, 3, 4) == [(0, 0, 0, 1, 1)]      # link 0, seq 1, digit 1: lost
    assert [pxb.explore_changes(X.CFG_A, 2, 3, c)[0][:4] for c in (8, 12)] == [(0, 0, 1, 1), (0, 0, 2, 1)]
    o = both_modes("a", X.STUCK)
    assert sum(held_by_radius(o)) == 598 and minimal_by_radius(o) == [0, 0, 36, 0] and list(o["ids"][:3]) == [32, 36, 40]
    o = both_modes("a", 0xFE)
    assert sum(held_by_radius(o)) == 940 and minimal_by_radius(o) == [0, 3, 21, 0]


def test_shape_b():
    """P2, N3, otherwise (a): T = 17,345, of which 2,445 run past depth."""
    o = both_modes("b", X.PANIC)
    assert 17345 - int(o["counts"][0, :, 0].sum()) == 2445
    assert held_by_radius(o) == [0, 0, 3, 105] and list(o["ids"]) == [140, 208, 292]
    o = both_modes("b", X.STUCK)
    assert sum(held_by_radius(o)) == 1526 and minimal_by_radius(o) == [0, 0, 36, 68]
    o = both_modes("b", X.LOG_DIV)
    assert held_by_radius(o) == [0, 0, 0, 36] and minimal_by_radius(o) == [0, 0, 0, 36] and o["ids"][0] == 1472
    o = both_modes("b", 0xFE)
    assert sum(held_by_radius(o)) == 1625 and sum(minimal_by_radius(o)) == 110


def test_shape_c():
    """Config 3, the row pxb.shrink gives id 10 at depth 64, site_depth 2, R 2: T =
    12,641; candidate 0 holds, so it is the only minimal one."""
    o = both_modes("c", X.PANIC)
    assert held_by_radius(o) == [1, 152, 11285, 0] and list(o["ids"]) == [0]
    assert 12641 - int(o["counts"][0, :, 0].sum()) == 1203


def test_shape_d():
    """Log mode: P2, N2, delay_max 2, 3 Ticks 8 steps apart, depth 32, site_depth
    3, R 2: T = 1,153."""
    o = both_modes("d", X.LOG_DIV)
    assert sum(held_by_radius(o)) == 74 and minimal_by_radius(o) == [0, 2, 12, 0] and list(o["ids"][:2]) == [16, 22]
    o = both_modes("d", X.PANIC)
    assert sum(held_by_radius(o)) == 0 and o["n"] == 0


def test_parents_cursor_and_capacity():
    """Several parents (one malformed, one with keep sites), first_parent, and a
    capacity below the matches: the host build follows pxb_explore_device's rules."""
    cfg, row, depth, sd, R, T = X.shape("a")
    bad = row.copy()
    bad[9] = 1
    keep = row.copy()
    pxb.script_links(cfg, keep[None, :], depth)[0, :, :, 1, :] = 0xFF
    parents = np.stack([row, bad, keep, row])
    want = X.brute(cfg, parents, depth, sd, R, X.PANIC)
    assert list(want["status"]) == [0, pxb.SCRIPT_BAD, 0, 0] and not want["counts"][1].any()
    sk = pxb.explore_skipped(cfg, keep, depth, sd, R, np.arange(T))
    assert (~sk).sum() == 1 + 8 * 2 + 28 * 4 + 56 * 8                        # the 8 sites of the other two acceptors
    assert not want["bytes"][2][sk].any() and want["counts"][2, :, 0].sum() <= (~sk).sum()
    o = X.host_explore(cfg, parents, depth, sd, R, X.PANIC, first_parent=5)
    assert np.array_equal(o["bytes"], want["bytes"])
    X.check(o["ids"], o["n"], o["counts"], o["status"], want, True, first_parent=5, T=T)
    assert list(o["ids"][:3]) == [5 * T + 4, 5 * T + 8, 5 * T + 12] and list(o["ids"][-3:]) == [8 * T + 4, 8 * T + 8, 8 * T + 12]
    o2 = X.host_explore(cfg, parents, depth, sd, R, X.PANIC, capacity=4, first_parent=5)
    assert o2["n"] == o["n"] and np.array_equal(o2["ids"], o["ids"][:4])


# ---- 4. every minimal candidate of (b), shrunk -------------------------------------------------------
@pytest.mark.parametrize("mask, n", [(X.PANIC, 3), (X.STUCK, 104), (X.LOG_DIV, 36)])
def test_minimal_candidates_are_shrunk_already(mask, n):
    """pxb.shrink on each minimal candidate of (b) takes nothing away: as many
    faults as the candidate has changes, in 2 launches (the row, then the singles
    that prove it 1-minimal)."""
    cfg, row, depth, sd, R, T = X.shape("b")
    ids = X.brute(cfg, row, depth, sd, R, mask)["minimal"]
    assert len(ids) == n
    rows = pxb.explore_rows(cfg, row, depth, sd, R, ids)
    for c, r in zip(ids, rows):
        _, faults, launches = pxb.shrink(cfg, r, mask, runner=SO.host_runner, depth=depth)
        assert len(faults) == len(pxb.explore_changes(cfg, sd, R, int(c))) and launches == 2, int(c)


# ---- 5. the C-ABI boundary ----------------------------------------------------------------------------
def test_explore_validation_without_a_device_call():
    L = pxb.load()
    cfg, row, depth, sd, R, T = X.shape("a")
    rows = np.stack([row, row])
    buf = np.zeros(64, np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def calls(cfg_=cfg, rows_p=P(rows), count=2, depth_=depth, space=(sd, R, X.PANIC, 1), ids_p=P(buf), cap=8,
              nm_p=P(buf[16:]), counts_p=None, status_p=None, which=(0, 1)):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        cp = C.byref(c) if c is not None else None
        sp = pxb.pxb_explore_space(*space) if space is not None else None
        spp = C.byref(sp) if sp is not None else None
        fns = (lambda: L.pxb_explore(cp, rows_p, count, depth_, spp, ids_p, cap, nm_p, counts_p, status_p),
               lambda: L.pxb_explore_device(cp, rows_p, count, depth_, spp, 0, ids_p, cap, nm_p, counts_p, status_p, None))
        return [fns[i]() for i in which]

    def inval(**kw):
        got = calls(**kw)
        return len(got) > 0 and all(rc == pxb.PXB_E_INVAL for rc in got)
    assert inval(cfg_=None) and inval(space=None)                         # null cfg, null space
    assert inval(rows_p=None)                                             # null rows, count > 0
    assert inval(nm_p=None)                                               # no cursor
    assert inval(depth_=4097, space=(4097, R, X.PANIC, 1))                # depth > 4096
    assert inval(space=(0, R, X.PANIC, 1)) and inval(space=(depth + 1, R, X.PANIC, 1))   # site_depth 0, > depth
    assert inval(space=(sd, 4, X.PANIC, 1))                               # radius > 3
    assert inval(space=(sd, R, 0, 1)) and inval(space=(sd, R, 0x100, 1))  # no flag of the low byte
    assert inval(space=(sd, R, X.PANIC, 2))                               # unknown flags bit
    assert inval(ids_p=None)                                              # capacity > 0 without ids
    big = dataclasses.replace(cfg, n_proposers=3, n_acceptors=9, delay_max=15)
    assert inval(cfg_=big, depth_=64, space=(64, 3, X.PANIC, 1), rows_p=P(np.zeros(1 << 16, np.uint8)), count=1)   # T == 0
    assert inval(count=(1 << 32) // T + 1, which=(1,))                    # count x T > 2^32
    assert inval(count=(1 << 30) + 1)
    assert inval(rows_p=C.c_void_p(rows.ctypes.data + 4), which=(1,))     # misaligned rows
    assert inval(ids_p=C.c_void_p(buf.ctypes.data + 4), which=(1,)) and inval(nm_p=C.c_void_p(buf.ctypes.data + 4), which=(1,))
    assert inval(counts_p=C.c_void_p(buf.ctypes.data + 2), which=(1,)) and inval(status_p=C.c_void_p(buf.ctypes.data + 2), which=(1,))
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0),
                dataclasses.replace(cfg, step_cap=4096), dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, tick_period=0)):
        assert inval(cfg_=bad), bad
    hdr = open(os.path.join(X.ROOT, "include", "paxos_batch.h")).read()
    assert re.search(r"#define PXB_EXPLORE_MAX_RADIUS\s+3u\s", hdr) and re.search(r"#define PXB_EXPLORE_MINIMAL\s+1u\s", hdr)
    assert (pxb.EXPLORE_MAX_RADIUS, pxb.EXPLORE_MINIMAL) == (3, 1) and C.sizeof(pxb.pxb_explore_space) == 16
    assert L.pxb_abi_version() == 5 and pxb.ABI_VERSION == 5
    import torch
    if not torch.cuda.is_available():                                     # valid calls, no GPU
        assert calls(which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=0, rows_p=None, cap=0, ids_p=None, which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=(1 << 32) // T + 1, which=(0,)) == [pxb.PXB_E_NODEV]   # (the host form walks in chunks)


def test_python_argument_checks():
    cfg, row, depth, sd, R, T = X.shape("a")
    with pytest.raises(ValueError):
        pxb.explore_rows(cfg, row, depth, sd, R, [T])                     # beyond the last parent
    with pytest.raises(ValueError):
        pxb.explore_rows(cfg, row, depth, depth + 1, R, [0])
    with pytest.raises(ValueError):
        pxb.explore_rows(cfg, row[:-8], depth, sd, R, [0])
    with pytest.raises(ValueError):
        pxb.explore_unrank(12, 2, 3, T)
    with pytest.raises(ValueError):
        pxb.explore_changes(dataclasses.replace(cfg, n_proposers=3, n_acceptors=9, delay_max=15), 64, 3, 0)
    assert pxb.explore_total(cfg, sd, R) == T == 1 + 12 * 2 + 66 * 4 + 220 * 8
    assert pxb.explore_total(cfg, sd, 4) == 0 and pxb.explore_total(cfg, 0, 1) == 0


# ---- 6. one stand-alone sanitizer program ----------------------------------------------------------------
SAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAIN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_EXPLORE_HOST_MAIN",
              "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_explore_core_sanitized():
    """explore_host.cpp with its own main (one shape: P = 1, N = 3, W = 8) under
    AddressSanitizer + UBSan, as a subprocess over shape (a), every buffer sized
    exactly: exit status 0, and the output equals the library build's."""
    if X.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([SO.HIPCC, *MAIN_FLAGS, *SAN_FLAGS, "-o", tmp, X.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    cfg, row, depth, sd, R, T = X.shape("a")
    for mask, minimal in ((X.PANIC, True), (0xFE, False)):
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "o.bin")
            e = dict(os.environ)
            e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
            p = subprocess.run([EXE, out, hex(cfg.seed), str(cfg.step_cap), str(mask), str(int(minimal))],
                               capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode == 0, "%s failed (rc %d): %s" % (EXE, p.returncode, p.stderr[-4000:])
            got = np.fromfile(out, dtype=np.uint8)
        o = X.host_explore(cfg, row, depth, sd, R, mask, minimal=minimal)
        want = np.concatenate([o["bytes"].reshape(-1), o["counts"].reshape(-1).view(np.uint8), o["status"].view(np.uint8),
                               np.array([o["n"]], np.uint64).view(np.uint8), o["ids"].view(np.uint8)])
        assert len(want) == len(got) and (want == got).all()
        assert o["n"] > 0
