"""The batched shrinker (docs/SEMANTICS.md §11) without a GPU.

The logic the shrink kernels share (csrc/shrink_core.h: ShrinkDraws over the
per-lane state machine, the per-entry fault test, the rank tables, select and
settle, the signature) is compiled for the HOST (tests/native/shrink_host.cpp)
and checked, instance by instance and bit for bit, against pxb.shrink with the
host runner of the scripted lane; then the C-ABI boundary of the new entry
points, and one stand-alone AddressSanitizer + UBSan program (its own main;
nothing is loaded into Python)."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import pxb
import script_oracle as SO
import shrink_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "shrink_host_san")
EXE_PLAIN = os.path.join(HERE, "native", "_build", "shrink_host_plain")
C3_INPUTS = [0, 3, 6, 10, 12, 14, 17, 18, 20, 23, 24, 26, 28, 29, 31, 39, 41, 48, 49, 54, 56, 57, 58, 60]
SETS = {"c3": (3, 64, pxb.F_PANIC), "c5": (5, 32, 0x3E), "c7": (7, 16, pxb.F_PANIC)}
_batches = {}


def batch(name, depth=64):
    """(cfg, extracted rows, host-batch outputs) of a set at `depth`, run once."""
    if (name, depth) not in _batches:
        c, n, mask = SETS[name]
        cfg = pxb.CONFIGS[c]
        rows = SO.host_extract(cfg, range(n), depth)
        _batches[(name, depth)] = (cfg, rows, H.host_batch(cfg, np.arange(n), mask, depth=depth))
    return _batches[(name, depth)]


def refs(name, depth=64):
    c, n, mask = SETS[name]
    cfg, rows, _ = batch(name, depth)
    return [H.reference(cfg, rows[i], mask, depth=depth, runner=SO.host_runner) for i in range(n)]


def check_set(name, depth=64):
    cfg, rows, o = batch(name, depth)
    rr = refs(name, depth)
    for i, ref in enumerate(rr):
        H.check(cfg, o, i, ref, depth)
    return cfg, rows, o, rr


# ---- 1-3. the three configurations ------------------------------------------------------------
def test_config3_equals_shrink():
    """Config 3, ids 0..63, depth 64, F_PANIC: the 24 inputs the issue lists, with
    rows, faults and launches those of pxb.shrink; the others NOT_INPUT, untouched.
    (pxb.shrink's launches for the 24 span 6 to 50, id 56 taking the 50, not the 6
    to 24 the issue states; their first rounds have 43 to 665 candidates.)"""
    cfg, rows, o, rr = check_set("c3")
    inputs = [i for i, r in enumerate(rr) if r["status"] != pxb.SHRINK_NOT_INPUT]
    assert inputs == C3_INPUTS
    la = [rr[i]["launches"] for i in inputs]
    first = [len(pxb.script_faults(cfg, rows[i], 64, SO.host_run(cfg, rows[i], 64)["sent"][0])) for i in inputs]
    print("launches", la, "first-round candidates", first)
    # parents finish in different rounds, and their candidates straddle the 64-lane blocks
    assert min(la) == 6 and max(la) >= 24 and len(set(la)) > 4, la
    assert (min(first), max(first)) == (43, 665), first
    for i in range(64):
        if i not in inputs:
            assert o["status"][i] == pxb.SHRINK_NOT_INPUT and (o["rows"][i] == rows[i]).all()
            assert o["launches"][i] == 1 and o["n_faults"][i] == 0
    assert (o["status"][inputs] == pxb.SHRINK_MINIMAL).all()


def test_config5_randomized():
    """Config 5, ids 0..31, mask 0x3E: randomized P, N = 9, the 8-step wheel."""
    _, _, o, rr = check_set("c5")
    assert sum(r["status"] != pxb.SHRINK_NOT_INPUT for r in rr) == 22
    assert ((o["status"] == pxb.SHRINK_MINIMAL) | (o["status"] == pxb.SHRINK_NOT_INPUT)).all()


def test_config7_log_mode():
    _, _, o, rr = check_set("c7")
    assert any(r["status"] != pxb.SHRINK_NOT_INPUT for r in rr)


# ---- 4. a shallow table -----------------------------------------------------------------------
def test_depth8():
    """Depth 8 on config 3: ids 0, 6, 12 shrink as pxb.shrink(depth=8) does (id 6
    to 2 faults, against 15 at depth 64); a link that outran the table: NOT_INPUT."""
    _, _, o, rr = check_set("c3", depth=8)
    _, _, o64 = batch("c3")
    for i in (0, 6, 12):
        assert rr[i]["status"] == pxb.SHRINK_MINIMAL, i
    assert o["n_faults"][6] == 2 and o64["n_faults"][6] == 15
    for i in (3, 10, 14, 20):
        assert o["status"][i] == pxb.SHRINK_NOT_INPUT, i


# ---- 5. the budget ------------------------------------------------------------------------------
@pytest.mark.parametrize("max_launches, want", [(1, (1, 268)), (2, (1, 268)), (3, (3, 146)), (7, (7, 132)), (8, (7, 132))])
def test_budget(max_launches, want):
    cfg, rows, _ = batch("c3")
    o = H.host_batch(cfg, rows[24:25], pxb.F_PANIC, max_launches=max_launches)
    ref = H.reference(cfg, rows[24], pxb.F_PANIC, max_launches=max_launches, runner=SO.host_runner)
    assert (int(o["launches"][0]), int(o["n_faults"][0])) == want
    assert o["status"][0] == pxb.SHRINK_BUDGET
    H.check(cfg, o, 0, ref, 64)


# ---- 6. nothing to shrink -----------------------------------------------------------------------
def test_no_faults():
    cfg = pxb.Config(seed=1, n_proposers=3, n_acceptors=9, step_cap=32)
    rows = SO.host_extract(cfg, [0, 1], 64)
    o = H.host_batch(cfg, rows, pxb.F_STEP_CAP)
    for i in range(2):
        assert (o["status"][i], o["launches"][i], o["n_faults"][i]) == (pxb.SHRINK_MINIMAL, 1, 0)
        H.check(cfg, o, i, H.reference(cfg, rows[i], pxb.F_STEP_CAP, runner=SO.host_runner), 64)


# ---- 7. batch independence ----------------------------------------------------------------------
def test_batch_independence():
    """Test 1's ids shuffled, with repeats and non-inputs interleaved: every id's
    outputs are those it had in test 1."""
    cfg, rows, o = batch("c3")
    rng = np.random.default_rng(7)
    order = np.concatenate([rng.permutation(64), rng.integers(0, 64, 16), [10, 10, 1, 10]])
    s = H.host_batch(cfg, rows[order], pxb.F_PANIC)
    for k in ("rows", "status", "n_faults", "launches", "sent", "res", "sig"):
        assert (s[k] == o[k][order]).all(), k


# ---- 8. the signature ---------------------------------------------------------------------------
def test_signature_and_clusters():
    """H.check holds the signature to pxb.script_signature; here: equal signature
    iff equal fault list (with the proposer count) within each set, and the
    clusters' counts sum to the number of shrunk rows."""
    for name in SETS:
        cfg, _, o = batch(name)
        shrunk = [i for i in range(len(o["status"])) if o["status"][i] in (pxb.SHRINK_MINIMAL, pxb.SHRINK_BUDGET)]
        key = {i: (int(o["rows"][i][8]), tuple(pxb.script_faults(cfg, o["rows"][i], 64, o["sent"][i])),
                   fault_values(cfg, o["rows"][i], o["sent"][i])) for i in shrunk}
        for i in shrunk:
            for j in shrunk:
                assert (o["sig"][i] == o["sig"][j]) == (key[i] == key[j]), (name, i, j)
        sig, cnt = pxb.shrink_clusters(o["sig"], o["status"])
        assert cnt.sum() == len(shrunk) and len(sig) == len({key[i] for i in shrunk})
        assert list(cnt) == sorted(cnt, reverse=True)


def fault_values(cfg, row, sent):
    """What each fault of the row is set to (the signature covers the values too)."""
    r = row[None, :]
    out = []
    for f in pxb.script_faults(cfg, row, 64, sent):
        if f[0] == "skew":
            out.append(int(pxb.script_skews(r)[0, f[1]]))
        elif f[0] == "win":
            out.append(tuple(min(int(x), 4096) for x in pxb.script_windows(cfg, r)[0, f[1]]))
        else:
            out.append(int(pxb.script_links(cfg, r, 64)[(0,) + tuple(f[1:])]))
    return tuple(out)


# ---- 9. the C-ABI boundary ----------------------------------------------------------------------
def test_shrink_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call (so on every
    host); the status constants; the ABI version stays 5."""
    L = pxb.load()
    cfg = pxb.CONFIGS[3]
    depth = 4
    rows = pxb.scripts_empty(cfg, range(8), depth)
    out = np.zeros(8 * 64, np.uint64)                   # (stands in for any output buffer: 16-byte aligned or not)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    base = out.ctypes.data + (-out.ctypes.data % 16)

    def calls(cfg_, rows_p=P(rows), count=8, depth_=depth, mask=pxb.F_PANIC, ml=64, which=(0, 1), dev_out=None):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        cp = C.byref(c) if c is not None else None
        d = dev_out or [None] * 6
        fns = (lambda: L.pxb_shrink_batch(cp, None, rows_p, count, depth_, mask, ml, None, None, None, None, None, None),
               lambda: L.pxb_shrink_batch_device(cp, rows_p, count, depth_, mask, ml, *d, None))
        return [fns[i]() for i in which]

    def inval(*a, **kw):
        got = calls(*a, **kw)
        return len(got) > 0 and all(rc == pxb.PXB_E_INVAL for rc in got)
    assert inval(None)                                                    # null cfg
    assert inval(cfg, rows_p=None)                                        # null rows, count > 0
    assert inval(cfg, depth_=4097)                                        # depth > 4096
    assert inval(cfg, count=(1 << 30) + 1)                                # count > 2^30
    assert inval(cfg, mask=0) and inval(cfg, mask=0x100)                  # no flag of the low byte
    assert inval(cfg, ml=0)                                               # no launch at all
    assert inval(cfg, rows_p=C.c_void_p(rows.ctypes.data + 4), which=(1,))   # misaligned rows
    for slot, off in ((0, 2), (1, 2), (2, 2), (3, 1), (4, 8), (5, 4)):   # status, faults, launches, sent, results, signature
        d = [None] * 6
        d[slot] = C.c_void_p(base + off)
        assert inval(cfg, which=(1,), dev_out=d), slot
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0),
                dataclasses.replace(cfg, step_cap=4096),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, tick_period=0),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, n_ticks=4097)):
        assert inval(bad), bad
    assert (pxb.SHRINK_MINIMAL, pxb.SHRINK_BUDGET, pxb.SHRINK_NOT_INPUT, pxb.SHRINK_TOO_MANY,
            pxb.SHRINK_UNSTABLE) == (0, 1, 2, 3, 4)
    hdr = open(os.path.join(H.ROOT, "include", "paxos_batch.h")).read()
    for name, v in (("MINIMAL", 0), ("BUDGET", 1), ("NOT_INPUT", 2), ("TOO_MANY", 3), ("UNSTABLE", 4)):
        assert re.search(r"#define PXB_SHRINK_%s\s+%du\s" % (name, v), hdr), name
    assert L.pxb_abi_version() == 5 and pxb.ABI_VERSION == 5
    import torch
    if not torch.cuda.is_available():                                     # a valid call, no GPU
        assert calls(cfg, which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(cfg, count=0, rows_p=None, which=(0,)) == [pxb.PXB_E_NODEV]


def test_python_argument_checks():
    cfg = pxb.CONFIGS[3]
    with pytest.raises(ValueError):
        pxb.shrink_batch(cfg, [1, 2], pxb.F_PANIC, chunk=0)
    with pytest.raises(ValueError):
        pxb.shrink_batch(cfg, [1, 2], pxb.F_PANIC, depth=4097)
    with pytest.raises(ValueError):
        pxb.shrink_batch(cfg, np.zeros((2, 7), np.uint8), pxb.F_PANIC)
    sig, cnt = pxb.shrink_clusters(np.array([5, 9, 5, 7, 9, 5], np.uint64), np.array([0, 1, 0, 2, 0, 1]))
    assert list(sig) == [5, 9] and list(cnt) == [3, 2]
    # the hash of a row with no faults is FNV-1a-64 of its proposer-count byte
    row = pxb.scripts_empty(cfg, [0], 4)
    pxb.script_links(cfg, row, 4)[:] = 1
    pxb.script_skews(row)[:] = 0
    pxb.script_windows(cfg, row)[:] = 0
    pxb.script_n_proposers(row)[0] = 2
    assert pxb.script_signature(cfg, row[0], 4, np.full((2, 2, 5), 4)) == ((pxb.FNV64_BASIS ^ 2) * pxb.FNV64_PRIME) % 2**64


# ---- 10. one stand-alone sanitizer program ------------------------------------------------------
SAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAIN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_SHRINK_HOST_MAIN",
              "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_shrink_core_sanitized():
    """shrink_host.cpp with its own main (one shape: P = 2, N = 5, W = 8) under
    AddressSanitizer + UBSan, as a subprocess over config 3's ids 0..31 at depth
    12, every buffer sized exactly: exit status 0, and the output equals the
    unsanitized build's and the library build's."""
    for exe, extra in ((EXE, SAN_FLAGS), (EXE_PLAIN, [])):
        if H.stale(exe):
            os.makedirs(os.path.dirname(exe), exist_ok=True)
            tmp = "%s.%d" % (exe, os.getpid())
            subprocess.run([SO.HIPCC, *MAIN_FLAGS, *extra, "-o", tmp, H.SRC], check=True, timeout=900)
            os.replace(tmp, exe)
    cfg = pxb.CONFIGS[3]
    n, depth = 32, 12
    got = []
    with tempfile.TemporaryDirectory() as td:
        for exe in (EXE, EXE_PLAIN):
            out = os.path.join(td, "o.bin")
            e = dict(os.environ)
            e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
            p = subprocess.run([exe, out, hex(cfg.seed), "0", str(n), str(depth), str(cfg.loss_ppm), str(cfg.delay_max),
                                str(cfg.skew_max), str(cfg.step_cap), str(pxb.F_PANIC), "64"],
                               capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode == 0, "%s failed (rc %d): %s" % (exe, p.returncode, p.stderr[-4000:])
            got.append(np.fromfile(out, dtype=np.uint8))
    assert len(got[0]) == len(got[1]) and (got[0] == got[1]).all()
    o = H.host_batch(cfg, np.arange(n), pxb.F_PANIC, depth=depth)
    want = np.concatenate([o[k].reshape(-1).view(np.uint8) for k in
                           ("rows", "status", "n_faults", "launches", "sent", "res", "sig")])
    assert len(want) == len(got[0]) and (want == got[0]).all()
    assert (o["status"] != pxb.SHRINK_NOT_INPUT).any()
