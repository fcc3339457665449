"""pxb_explore_cover (docs/SEMANTICS.md §15) without a GPU.

The logic the kernels share (csrc/explore_cover_core.h: ExploreEventDraws under
CoverLane, the flag byte; explore_core.h: the space and the minimality test) is
compiled for the HOST (tests/native/explore_cover_host.cpp) and checked against
brute force: every candidate materialised by pxb.explore_rows, run by the host
build of the scripted lane and of the coverage lane, the predicate, the subset
rule and pxb.explore_reach_of in Python.  Then the ties to the reference model's
fold and to pxb_explore, the pinned findings, the C-ABI boundary of the new entry
points, and one stand-alone AddressSanitizer + UBSan program (its own main;
nothing is loaded into Python)."""
import ctypes as C
import dataclasses
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cover_oracle as CO
import explore_cover_oracle as XC
import explore_oracle as X
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "explore_cover_host_san")
BIT = CO.BIT


def host_against_brute(cfg, parents, depth, sd, R, query, flag_mask, **kw):
    """The host build in both listing modes against the yardstick, exactly:
    bytes, masks, ids, n, counts, reach, status.  Returns the minimal-mode dict."""
    want = XC.brute(cfg, parents, depth, sd, R, query, flag_mask)
    out = None
    for minimal in (False, True):
        o = XC.host_explore_cover(cfg, parents, depth, sd, R, query, flag_mask, minimal=minimal, **kw)
        assert np.array_equal(o["bytes"], want["bytes"]) and np.array_equal(o["masks"], want["masks"])
        T = pxb.explore_total(cfg, sd, R)
        XC.check(o["ids"], o["n"], o["counts"], o["reach"], o["status"], want, minimal, kw.get("first_parent", 0), T)
        out = o
    return out


# ---- 1. the host build against the brute ------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_host_build_equals_brute(name):
    """Shapes (a), (b), (d) and (c) (the shrunk config-3 id 10 row), with a
    cover-only query, a flag-only predicate and both."""
    cfg, row, depth, sd, R, T = X.shape(name)
    assert pxb.explore_total(cfg, sd, R) == T
    held = {}
    for key, (q, mask) in XC.QUERIES.items():
        o = host_against_brute(cfg, row, depth, sd, R, q, mask)
        held[key] = int(o["counts"][0, :, 1].sum())
        print(name, key, "held", held[key], "minimal", int(o["counts"][0, :, 2].sum()), "n", o["n"])
    assert held["both"] > 0 and (held["cover"] > 0 or name == "c")       # (the queries are not vacuous)


def test_five_parents_on_the_host():
    """Shape (a), T = 2,049: a malformed parent and parents with keep sites among
    good ones, first_parent, and a capacity below the matches."""
    cfg, parents, depth, sd, R, T = XC.five_parents()
    q, mask = XC.QUERIES["cover"]
    o = host_against_brute(cfg, parents, depth, sd, R, q, mask, first_parent=3)
    assert list(o["status"]) == [0, pxb.SCRIPT_BAD, 0, 0, 0]
    bad = o["reach"][1]
    assert not bad["count"].any() and (bad["first"] == pxb.REACH_NONE).all() and bad["parent_mask"] == 0 == bad["union_mask"]
    assert o["reach"][0].tobytes() == o["reach"][4].tobytes() and o["reach"][0].tobytes() != o["reach"][2].tobytes()
    o2 = XC.host_explore_cover(cfg, parents, depth, sd, R, q, mask, capacity=5, first_parent=3)
    assert o2["n"] == o["n"] > 5 and np.array_equal(o2["ids"], o["ids"][:5])
    cfg, parents, depth, sd, R, T = XC.keep_parents()
    assert pxb.explore_total(cfg, sd, R) == T
    sk = pxb.explore_skipped(cfg, parents, depth, sd, R, np.arange(5 * T)).reshape(5, T)
    assert sk[0].any() and sk[1].any() and not sk[3].any()               # absent proposers' links are keep sites
    o = host_against_brute(cfg, parents, depth, sd, R, None, 0)
    assert list(o["status"]) == [0, 0, pxb.SCRIPT_BAD, 0, 0] and not o["bytes"][sk].any()


# ---- 2. ties to the reference model ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_masks_equal_the_reference_models(name):
    """The first[b] candidate of every reached class and 64 candidates drawn with
    a fixed seed: cover_oracle.oracle_row (the Python reference-model fold, and
    pxb.cover_of_events beside it) gives the mask the host lane gave."""
    cfg, row, depth, sd, R, T = X.shape(name)
    o = XC.host_explore_cover(cfg, row, depth, sd, R)
    rec = pxb.ExploreReach.from_record(o["reach"][0])
    firsts = [f for f in rec.first if f != pxb.REACH_NONE]
    assert firsts
    cs = np.unique(np.concatenate([firsts, np.random.default_rng(0xC0FE + T).integers(0, T, 64)])).astype(np.uint64)
    rows = pxb.explore_rows(cfg, row, depth, sd, R, cs)
    for c, r in zip(cs, rows):
        m = CO.oracle_row(cfg, r, depth)[0]
        if o["bytes"][0, int(c)] & XC.RAN:
            assert m == int(o["masks"][0, int(c)]), (int(c), pxb.cover_names(m), pxb.cover_names(o["masks"][0, int(c)]))
        else:
            assert o["masks"][0, int(c)] == 0
    for b, f in enumerate(rec.first):                                    # the witness has its class
        assert f == pxb.REACH_NONE or (o["masks"][0, f] >> b) & 1


# ---- 3. ties to pxb_explore ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("mask", [X.PANIC, X.LOG_DIV])
def test_flag_only_predicate_is_pxb_explores(name, mask):
    cfg, row, depth, sd, R, T = X.shape(name)
    for minimal in (False, True):
        h = X.host_explore(cfg, row, depth, sd, R, mask, minimal=minimal)
        o = XC.host_explore_cover(cfg, row, depth, sd, R, None, mask, minimal=minimal)
        assert np.array_equal(o["bytes"], h["bytes"]) and np.array_equal(o["ids"], h["ids"]) and o["n"] == h["n"]
        assert np.array_equal(o["counts"], h["counts"]) and np.array_equal(o["status"], h["status"])


# ---- 4. the pinned findings ------------------------------------------------------------------------------
def test_pinned_findings():
    """tests/golden/kat_explore_cover.json against the yardstick, and the numbers
    of the feature's README paragraph.  (Where a candidate consumes more than
    `depth` entries of a link it did not run OK and has no mask: without that
    rule Q1_FOREIGN_ACCEPT of (b) would read first 1, [0, 6, 215, 3809],
    R2S_REPEAT first 1442, [0, 0, 0, 23], and R2S_DROPPED of (d) first 199,
    [0, 0, 7].)"""
    kat = json.load(open(XC.KAT_PATH))["shapes"]
    for name in ("a", "b", "d"):
        assert XC.findings(name) == kat[name], name
    a, b, d = (kat[n]["classes"] for n in "abd")
    assert (a["EXEC_PANIC"]["first"], a["EXEC_PANIC"]["count"]) == (4, [0, 3, 45, 294])
    for n in ("PROPOSE_NACK", "EXEC_IGNORED", "EXEC_PANIC", "HAVE_IDLE", "HAVE_BELOW"):
        assert a[n]["distance"] == 1
    assert [a[n]["first"] for n in ("PROPOSE_NACK", "EXEC_IGNORED", "EXEC_PANIC", "HAVE_IDLE", "HAVE_BELOW")] == [2, 2, 4, 10, 2]
    assert (b["Q1_FOREIGN_ACCEPT"]["first"], b["Q1_FOREIGN_ACCEPT"]["count"]) == (2, [0, 3, 110, 2015])
    assert (b["EXEC_PANIC"]["first"], b["EXEC_PANIC"]["count"]) == (140, [0, 0, 3, 105])
    assert (b["DISCARD_DEAD"]["first"], b["DISCARD_DEAD"]["count"][:3]) == (140, [0, 0, 3])
    assert (b["R2S_REPEAT"]["first"], b["R2S_REPEAT"]["count"], b["R2S_REPEAT"]["distance"]) == (1444, [0, 0, 0, 2], 3)
    for n in ("Q7_STALE_EXEC", "TICK_BUSY", "DISCARD_ISOLATED"):
        assert n not in b
    assert d["TICK_BUSY"]["first"] == 0 and "TICK_BUSY" in kat["d"]["parent"]
    assert (d["R2S_DROPPED"]["first"], d["R2S_DROPPED"]["count"]) == (354, [0, 0, 2])
    assert "EXEC_PANIC" not in d
    # every minimal candidate with a repeated Round2Success near (b) changes three sites
    cfg, row, depth, sd, R, T = X.shape("b")
    o = XC.host_explore_cover(cfg, row, depth, sd, R, pxb.CoverQuery(all_mask=BIT["R2S_REPEAT"]))
    base = pxb._explore_bases(2 * 2 * 3 * sd, cfg.delay_max, R)
    assert o["n"] == len(o["ids"]) > 0 and (o["ids"] >= base[3]).all() and o["ids"][0] == 1444


# ---- 5. properties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_properties_of_a_record(name):
    cfg, row, depth, sd, R, T = X.shape(name)
    o = XC.host_explore_cover(cfg, row, depth, sd, R)
    rec = o["reach"][0]
    r = pxb.ExploreReach.from_record(rec)
    S, A = 2 * cfg.n_proposers * cfg.n_acceptors * sd, cfg.delay_max
    assert pxb.explore_reach_of(o["masks"][0], (o["bytes"][0] & XC.RAN) != 0, S, A, R).tobytes() == rec.tobytes()
    dist = pxb.reach_distance(r)
    assert dist == pxb.reach_distance(rec) and len(dist) == pxb.COVER_CLASSES
    base = pxb._explore_bases(S, A, R)
    union = 0
    for b in range(pxb.COVER_CLASSES):
        col = [r.counts[q][b] for q in range(4)]
        if any(col):
            union |= 1 << b
            first_r = next(q for q in range(4) if col[q])
            assert dist[b] == first_r and base[first_r] <= r.first[b] < base[first_r + 1]
        else:
            assert dist[b] is None and r.first[b] == pxb.REACH_NONE
        assert all(col[q] <= int(o["counts"][0, q, 0]) for q in range(4)) and not any(col[R + 1:])
    assert r.union == union and (union >> pxb.COVER_CLASSES) == 0
    ev = pxb.event_dtype()
    events = CO.oracle_row(cfg, row, depth)[2]
    assert events.dtype == ev and r.parent_mask == pxb.cover_of_events(events, cfg.n_acceptors)
    with pytest.raises(ValueError):
        pxb.explore_reach_of(o["masks"][0][:-1], np.ones(T - 1, bool), S, A, R)


# ---- 6. the C-ABI boundary ------------------------------------------------------------------------------------
def test_validation_without_a_device_call():
    L = pxb.load()
    cfg, row, depth, sd, R, T = X.shape("a")
    rows = np.stack([row, row])
    buf = np.zeros(64 + 2 * 81, np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def calls(cfg_=cfg, cflags=0, rows_p=P(rows), count=2, depth_=depth, space=(sd, R, 0, 1), q=(0, 0, 0, 0), ids_p=P(buf),
              cap=8, nm_p=P(buf[16:]), counts_p=None, reach_p=None, status_p=None, which=(0, 1)):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= cflags
        cp = C.byref(c) if c is not None else None
        sp = pxb.pxb_explore_cover_space(*space, pxb.pxb_cover_query(*q)) if space is not None else None
        spp = C.byref(sp) if sp is not None else None
        fns = (lambda: L.pxb_explore_cover(cp, rows_p, count, depth_, spp, ids_p, cap, nm_p, counts_p, reach_p, status_p),
               lambda: L.pxb_explore_cover_device(cp, rows_p, count, depth_, spp, 0, ids_p, cap, nm_p, counts_p, reach_p,
                                                  status_p, None))
        return [fns[i]() for i in which]

    def inval(**kw):
        got = calls(**kw)
        return len(got) > 0 and all(rc == pxb.PXB_E_INVAL for rc in got)
    assert inval(cfg_=None) and inval(space=None)                         # null cfg, null space
    assert inval(rows_p=None)                                             # null rows, count > 0
    assert inval(nm_p=None)                                               # no cursor
    assert inval(depth_=4097, space=(4097, R, 0, 1))                      # depth > 4096
    assert inval(space=(0, R, 0, 1)) and inval(space=(depth + 1, R, 0, 1))   # site_depth 0, > depth
    assert inval(space=(sd, 4, 0, 1))                                     # radius > 3
    assert inval(space=(sd, R, 0x100, 1))                                 # a flag mask with nothing in the low byte
    assert inval(space=(sd, R, 0, 2))                                     # unknown flags bit
    assert inval(q=(0, 0, 0, 1))                                          # q.reserved
    assert inval(cflags=pxb.CFG_TRACE_PRODUCTION)
    assert inval(ids_p=None)                                              # capacity > 0 without ids
    big = dataclasses.replace(cfg, n_proposers=3, n_acceptors=9, delay_max=15)
    assert inval(cfg_=big, depth_=64, space=(64, 3, 0, 1), rows_p=P(np.zeros(1 << 16, np.uint8)), count=1)   # T == 0
    assert inval(count=(1 << 32) // T + 1, which=(1,))                    # count x T > 2^32
    assert inval(count=(1 << 30) + 1)
    off = lambda k: C.c_void_p(buf.ctypes.data + k)  # noqa: E731
    assert inval(rows_p=C.c_void_p(rows.ctypes.data + 4), which=(1,))     # misaligned rows
    assert inval(ids_p=off(4), which=(1,)) and inval(nm_p=off(4), which=(1,))
    assert inval(counts_p=off(2), which=(1,)) and inval(status_p=off(2), which=(1,))
    assert inval(reach_p=off(512 + 4), which=(1,))                        # a misaligned d_reach
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0),
                dataclasses.replace(cfg, step_cap=4096), dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, tick_period=0)):
        assert inval(cfg_=bad), bad
    hdr = open(os.path.join(X.ROOT, "include", "paxos_batch.h")).read()
    assert re.search(r"typedef struct pxb_explore_reach \{\s+/\* 648 B", hdr)
    assert re.search(r"typedef struct pxb_explore_cover_space \{\s+/\* 32 B", hdr)
    assert C.sizeof(pxb.pxb_explore_cover_space) == 32 and C.sizeof(pxb.pxb_explore_reach) == 648 == pxb.reach_dtype().itemsize
    assert L.pxb_abi_version() == 5 and pxb.ABI_VERSION == 5
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_explore_cover", "pxb_explore_cover_device"):
        assert " T %s\n" % name in out and hasattr(L, name)
    import torch
    if not torch.cuda.is_available():                                     # valid calls, no GPU
        assert calls(which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(space=(sd, R, X.PANIC, 0), q=(1, 2, 4, 0), reach_p=off(512), which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=0, rows_p=None, cap=0, ids_p=None, which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(count=(1 << 32) // T + 1, which=(0,)) == [pxb.PXB_E_NODEV]   # (the host form walks in chunks)
        with pytest.raises(pxb.PaxosError):
            pxb.explore_cover(cfg, row, depth, sd, R)


def test_struct_sizes_in_c(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "paxos_batch.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(pxb_explore_cover_space), sizeof(pxb_explore_reach),
         offsetof(pxb_explore_cover_space, q), offsetof(pxb_explore_reach, first),
         offsetof(pxb_explore_reach, parent_mask), offsetof(pxb_explore_reach, union_mask));
  return 0;
}'''
    tmp = str(tmp_path / "pxb_exc_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(X.ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True).stdout.split()]
    assert got == [32, 648, pxb.pxb_explore_cover_space.q.offset, pxb.pxb_explore_reach.first.offset,
                   pxb.pxb_explore_reach.parent_mask.offset, pxb.pxb_explore_reach.union_mask.offset] == [32, 648, 16, 512, 640, 644]


def test_python_argument_checks():
    cfg, row, depth, sd, R, T = X.shape("a")
    import torch
    n = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="required"):
        pxb.explore_cover_device(cfg, None, 1, depth, sd, R, None)
    with pytest.raises(ValueError, match="CUDA"):
        pxb.explore_cover_device(cfg, torch.zeros(len(row), dtype=torch.uint8), 1, depth, sd, R, n)
    assert pxb.reach_distance(pxb.explore_reach_of(np.zeros(T, np.uint32), np.ones(T, bool), 12, 2, 3)) == [None] * 29
    hs = open(os.path.join(X.ROOT, "cloud-haskell-paxos_amd", "hs", "PaxosBatch.hs")).read()
    assert "pxb_explore_cover" in hs and "exploreCover" in hs


# ---- 7. one stand-alone sanitizer program ------------------------------------------------------------------------
SAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAIN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_EXPLORE_COVER_HOST_MAIN",
              "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_explore_cover_core_sanitized():
    """explore_cover_host.cpp with its own main (one shape: P = 1, N = 3, W = 8)
    under AddressSanitizer + UBSan, as a subprocess over the five parents of
    shape (a), every buffer sized exactly: exit status 0, and the output equals
    the library build's."""
    if XC.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([SO.HIPCC, *MAIN_FLAGS, *SAN_FLAGS, "-o", tmp, XC.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    cfg, parents, depth, sd, R, T = XC.five_parents()
    q, mask = XC.QUERIES["both"]
    sp = pxb._explore_cover_space(sd, R, q, mask, True)
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
    o = XC.host_explore_cover(cfg, parents, depth, sd, R, q, mask, minimal=True)
    want = np.concatenate([o["bytes"].reshape(-1), o["masks"].reshape(-1).view(np.uint8), o["counts"].reshape(-1).view(np.uint8),
                           o["reach"].view(np.uint8), o["status"].view(np.uint8), np.array([o["n"]], np.uint64).view(np.uint8),
                           o["ids"].view(np.uint8)])
    assert len(want) == len(got) and (want == got).all()
    assert o["n"] > 0
