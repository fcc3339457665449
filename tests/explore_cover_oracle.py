"""Test-side helpers for pxb_explore_cover (docs/SEMANTICS.md §15).

* ``brute``: the yardstick.  Every non-skipped candidate of every parent
  materialised by pxb.explore_rows; status, flags and send counts from a
  scripted runner (script_oracle.host_runner, or pxb.run_scripted on the GPU);
  masks from a cover function (cover_oracle.host_cover, or pxb.cover); then the
  predicate, the subset rule (explore_oracle.subset_table) and
  pxb.explore_reach_of in Python.  Computed once per key and shared.
* ``host_explore_cover``: the host build of the shared logic
  (tests/native/explore_cover_host.cpp): pxb_explore_cover_device's arguments
  and outputs plus the candidates' flag bytes and masks.
* ``check``: an implementation's outputs against the yardstick, exactly.
* the parents and queries the tests share.  No tests here."""
import ctypes as C
import os
import subprocess

import numpy as np

import cover_oracle as CO
import explore_oracle as X
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "explore_cover_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libexplore_cover_host.so")
DEPS = sorted(set(X.DEPS[1:] + CO.DEPS[:-2] + [SRC] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("cover_core.h", "events_core.h", "explore_cover_core.h")]))
KAT_PATH = os.path.join(HERE, "golden", "kat_explore_cover.json")
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
        vp = C.c_void_p
        _lib.explore_cover_host_run.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp,
                                                vp, vp, vp, vp]
    return _lib


def host_explore_cover(cfg, parents, depth, site_depth, radius, query=None, flag_mask=0, minimal=True, capacity=None,
                       first_parent=0):
    """explore_cover_host_run: a dict of ids, n, counts (n, 4, 3), reach (n,)
    records, status, bytes (n, T), masks (n, T)."""
    rows = pxb._script_rows(cfg, parents, depth)
    n, T = len(rows), pxb.explore_total(cfg, site_depth, radius)
    o = {"counts": np.full((n, 4, 3), 99, np.uint32), "status": np.full(n, 99, np.uint32),
         "bytes": np.full((n, T), 0xA5, np.uint8), "masks": np.full((n, T), 0xA5A5A5A5, np.uint32),
         "reach": np.zeros(n, pxb.reach_dtype())}
    o["reach"].view(np.uint8)[:] = 0xA5
    c = cfg.to_c(0, 1)
    sp = pxb._explore_cover_space(site_depth, radius, query, flag_mask, minimal)
    nm = C.c_uint64(0)

    def call(ids, cap):
        nm.value = 0
        rc = lib().explore_cover_host_run(C.addressof(c), rows.ctypes.data, n, depth, C.addressof(sp), first_parent,
                                          ids.ctypes.data if cap else None, cap, C.addressof(nm),
                                          o["counts"].ctypes.data, o["reach"].ctypes.data, o["status"].ctypes.data,
                                          o["bytes"].ctypes.data, o["masks"].ctypes.data)
        assert rc == 0, "explore_cover_host_run rc=%d" % rc
    if capacity is None:
        call(None, 0)
        capacity = nm.value
    ids = np.zeros(capacity, np.uint64)
    call(ids, capacity)
    o["ids"], o["n"] = ids[:min(nm.value, capacity)], nm.value
    return o


def host_coverer(cfg, rows, depth):
    """The masks of well-formed rows through the host build of the coverage lane."""
    rc, masks, status, _, _ = CO.host_cover(cfg, rows, depth)
    assert rc == 0
    return masks, status


def gpu_coverer(cfg, rows, depth):
    masks, status, _, _ = pxb.cover(cfg, rows, depth)
    return masks, status


def run_all(cfg, parents, depth, site_depth, radius, runner=SO.host_runner, coverer=host_coverer, chunk=1 << 15):
    """(ran (n, T) bool, flags (n, T) uint32, masks (n, T) uint32, status (n,)):
    every candidate of every parent run as a materialised row; the mask of a
    candidate that did not run OK is 0.  Does not depend on a predicate: shared
    by every query over the same space."""
    rows = pxb._script_rows(cfg, parents, depth)
    key = ("run", repr(cfg), rows.tobytes(), depth, site_depth, radius, runner, coverer)
    if key in _brutes:
        return _brutes[key]
    n, T = len(rows), pxb.explore_total(cfg, site_depth, radius)
    status = np.array([pxb.SCRIPT_BAD if (r[8] > cfg.n_proposers or r[9]) else pxb.TRACE_OK for r in rows], np.uint32)
    g = np.arange(n * T, dtype=np.uint64)
    run = ~pxb.explore_skipped(cfg, rows, depth, site_depth, radius, g) & (status[g // np.uint64(T)] == pxb.TRACE_OK)
    ran, flags, masks = np.zeros(n * T, bool), np.zeros(n * T, np.uint32), np.zeros(n * T, np.uint32)
    todo = g[run]
    for a in range(0, len(todo), chunk):
        w = todo[a:a + chunk]
        cand = pxb.explore_rows(cfg, rows, depth, site_depth, radius, w)
        res, st, sent = runner(cfg, cand, depth)
        ok = (np.asarray(st) == pxb.TRACE_OK) & (np.asarray(sent).reshape(len(w), -1).max(axis=1) <= depth)
        m, mst = coverer(cfg, cand, depth)
        assert np.array_equal(np.asarray(mst), np.asarray(st))
        wi = w.astype(np.int64)
        ran[wi], flags[wi], masks[wi] = ok, np.asarray(res)[:, 3] & 0xFF, np.where(ok, m, 0)
    _brutes[key] = (ran.reshape(n, T), flags.reshape(n, T), masks.reshape(n, T), status)
    return _brutes[key]


def brute(cfg, parents, depth, site_depth, radius, query=None, flag_mask=0, runner=SO.host_runner, coverer=host_coverer):
    """The yardstick: a dict of bytes (n, T) with the ran / held / minimal bits,
    masks (n, T), counts (n, 4, 3), reach (n,) records, status (n,), held and
    minimal (ascending global ids)."""
    q = query or pxb.CoverQuery()
    ran, flags, masks, status = run_all(cfg, parents, depth, site_depth, radius, runner, coverer)
    n, T = ran.shape
    S, A = 2 * cfg.n_proposers * cfg.n_acceptors * site_depth, cfg.delay_max
    match = ((masks & q.all_mask) == q.all_mask) & ((masks & q.none_mask) == 0)
    if q.any_mask:
        match &= (masks & q.any_mask) != 0
    held = ran & match
    if flag_mask:
        held &= (flags & flag_mask) != 0
    by = (ran * RAN + held * HELD).astype(np.uint8)
    r_of, rank, valid = X.subset_table(S, A, radius)
    for i in range(n):
        smaller = np.zeros(T, bool)                    # a proper subset of the changes holds
        for sub in range(7):
            smaller |= valid[sub] & held[i][rank[sub]]
        by[i, held[i] & ~smaller] |= MINIMAL
    counts = np.zeros((n, 4, 3), np.uint32)
    for r in range(radius + 1):
        for b in range(3):
            counts[:, r, b] = ((by[:, r_of == r] >> b) & 1).sum(axis=1)
    reach = np.zeros(n, pxb.reach_dtype())
    for i in range(n):
        reach[i] = pxb.explore_reach_of(masks[i], ran[i], S, A, radius)
    flat = by.reshape(-1)
    return {"bytes": by, "masks": masks, "counts": counts, "reach": reach, "status": status,
            "held": np.nonzero(flat & HELD)[0].astype(np.uint64), "minimal": np.nonzero(flat & MINIMAL)[0].astype(np.uint64)}


def reach_records(reach):
    """A list of pxb.ExploreReach, or an array of records, as an array of records."""
    if isinstance(reach, np.ndarray):
        return reach
    out = np.zeros(len(reach), pxb.reach_dtype())
    out["first"][:] = pxb.REACH_NONE
    for i, r in enumerate(reach):
        out["count"][i, :, :29], out["first"][i, :29] = r.counts, r.first
        out["parent_mask"][i], out["union_mask"][i] = r.parent_mask, r.union
        assert r.tail == [[0, 0, 0, 0, pxb.REACH_NONE]] * 3, r.tail
    return out


def check(got_ids, got_n, counts, reach, status, want, minimal, first_parent=0, T=0):
    """ids, n_matches, counts, reach and status against the yardstick, exactly."""
    X.check(got_ids, got_n, counts, status, want, minimal, first_parent, T)
    reach = reach_records(reach)
    assert reach.tobytes() == want["reach"].tobytes(), [
        (i, k) for i in range(len(reach)) for k in reach.dtype.names if not np.array_equal(reach[i][k], want["reach"][i][k])]


# ---- what the tests share -----------------------------------------------------------------------
BIT = CO.BIT
QUERIES = {"cover": (pxb.CoverQuery(any_mask=BIT["PROPOSE_NACK"] | BIT["HAVE_ABORT_R2"], none_mask=BIT["EXEC_PANIC"]), 0),
           "flag": (None, X.PANIC), "both": (pxb.CoverQuery(all_mask=BIT["R1OK_STALE"]), 0xFE)}


def five_parents():
    """(cfg, parents, depth, site_depth, radius, T) of shape (a): the benign row, a
    malformed row (reserved byte set), two rows extracted from the config (ids 1
    and 2) with keep sites, and the benign row again.  Shape (a) has one
    proposer, so no extracted row of it has an absent proposer's links: the keep
    sites are put on one acceptor's links and on every reply link instead
    (keep_parents has rows whose keep sites are absent proposers')."""
    cfg, row, depth, sd, R, T = X.shape("a")
    bad = row.copy()
    bad[9] = 1
    k1, k2 = SO.host_extract(cfg, [1, 2], depth)
    pxb.script_links(cfg, k1[None, :], depth)[0, :, :, 1, :] = 0xFF
    pxb.script_links(cfg, k2[None, :], depth)[0, 1, :, :, :] = 0xFF
    return cfg, np.stack([row, bad, k1, k2, row]), depth, sd, R, T


KEEP_CFG = pxb.Config(seed=0x5EED0155, n_proposers=2, n_acceptors=3, loss_ppm=100000, delay_max=2, skew_max=3,
                      randomize=True, step_cap=256)


def keep_parents():
    """(cfg, parents, depth, site_depth, radius, T): a RANDOMIZE config of up to
    two proposers; five parents at depth 8, site_depth 1, radius 2 (T = 289): two
    extracted rows whose drawn P is 1 (the links of proposer 1 are keep sites), a
    malformed row, an extracted row with both proposers, and the first again."""
    cfg, depth, sd, R = KEEP_CFG, 8, 1, 2
    rows = SO.host_extract(cfg, np.arange(64), depth)
    drawn = pxb.script_n_proposers(rows)
    one, two = np.nonzero(drawn == 1)[0], np.nonzero(drawn == 2)[0]
    bad = rows[two[0]].copy()
    bad[9] = 1
    return cfg, np.stack([rows[one[0]], rows[one[1]], bad, rows[two[0]], rows[one[0]]]), depth, sd, R, 289


# ---- the pinned findings (tests/golden/kat_explore_cover.json) ------------------------------------
def findings(name):
    """{class name: {"first", "count", "distance"}} of a pinned shape's reached
    classes, and the parent's classes, from the yardstick."""
    cfg, row, depth, sd, R, T = X.shape(name)
    r = pxb.ExploreReach.from_record(brute(cfg, row, depth, sd, R)["reach"][0])
    dist = pxb.reach_distance(r)
    return {"T": T, "parent": pxb.cover_names(r.parent_mask),
            "classes": {n: {"first": f, "count": c[:R + 1], "distance": dist[pxb.COVER_BIT[n]]}
                        for n, (f, c) in r.by_name().items()}}


if __name__ == "__main__":                           # python tests/explore_cover_oracle.py: rewrite the recorded results
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    with open(KAT_PATH, "w") as f:
        json.dump({"about": "pxb_explore_cover: per pinned shape of tests/explore_oracle.py (benign parent), the reach "
                            "record of the brute-force yardstick: first candidate, count per radius and reach distance "
                            "of every reached class", "shapes": {n: findings(n) for n in ("a", "b", "d")}}, f, indent=1)
        f.write("\n")


def unit_case(P, N, delay_max):
    """test_explore_gpu.unit_case's config and parents (the benign row and an
    extracted row of a faulty config) at depth 64 with a step cap of 64, so that
    the duelling proposers of the largest shapes still run OK within the depth: (cfg, parents, depth, site_depth 1, radius 1)."""
    cfg = pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                     delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                     step_cap=64)
    depth = 64
    return cfg, np.stack([X.benign_row(cfg, depth), SO.host_extract(cfg, [1], depth)[0]]), depth, 1, 1
