"""Handler-path coverage (docs/SEMANTICS.md §14) without a GPU.

The coverage lane the kernels run (csrc/cover_core.h: CoverLane over the
scripted lane with the tapped draw source) is compiled for the HOST
(tests/native/cover_host.cpp) and checked against the fold of the reference
model's events (tests/cover_oracle.py), which is itself compared with the
specification ``pxb.cover_of_events`` on every row; against hand-derived rows
(tests/golden/kat_cover.json); at the C-ABI boundary of the new entry points;
and by one stand-alone AddressSanitizer + UBSan program (its own main; nothing
is loaded into Python)."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import cover_oracle as CO
import event_oracle as EO
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "cover_host_san")
NONE64 = (1 << 64) - 1


def check_call(cfg, rows, depth, want_masks, want_steps):
    """The host lane's masks, status, steps and summary of well-formed rows that do not bail."""
    rc, m, st, res, s = CO.host_cover(cfg, rows, depth)
    assert rc == 0 and (st == pxb.TRACE_OK).all()
    bad = np.nonzero(m != want_masks)[0]
    assert len(bad) == 0, "row %d: host %s, oracle %s" % (bad[0], pxb.cover_names(m[bad[0]]),
                                                         pxb.cover_names(want_masks[bad[0]]))
    assert ((res[:, 3] >> 16) == want_steps).all()
    steps4 = np.zeros((len(rows), 4), np.uint32)
    steps4[:, 3] = want_steps.astype(np.uint32) << 16
    assert CO.summary_dict(s) == CO.expected_summary(want_masks, np.zeros(len(rows), np.uint32), steps4)
    assert s.n_matches == 0
    return m, st, res, s


# ---- 1. the five cases ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CO.CASES))
def test_cases_equal_the_oracle_fold(name):
    cfg, ids, masks, steps = CO.case_oracle(name)
    check_call(cfg, pxb.scripts_empty(cfg, ids, 0), 0, masks, steps)


def test_extracted_rows_equal_the_oracle_fold():
    """The lossy case as rows extracted at depth 64: the oracle runs every extracted row itself."""
    cfg, ids, masks, steps = CO.case_oracle("lossy-p2n3")
    rows = SO.host_extract(cfg, ids, CO.EXTRACT_DEPTH)
    got = [CO.oracle_row(cfg, rows[i], CO.EXTRACT_DEPTH)[:2] for i in range(len(ids))]
    emasks = np.array([g[0] for g in got], dtype=np.uint32)
    esteps = np.array([g[1] for g in got], dtype=np.uint32)
    check_call(cfg, rows, CO.EXTRACT_DEPTH, emasks, esteps)
    assert (emasks == masks).all() and (esteps == steps).all()        # (the schedule Philox gives, spelled out)


def test_the_cases_reach_every_class():
    union = 0
    for name in CO.CASES:
        union |= int(np.bitwise_or.reduce(CO.case_oracle(name)[2]))
    assert union == (1 << 29) - 1, pxb.cover_names(CO.ALL & ~union)
    lossy = CO.case_oracle("lossy-p2n3")[2]
    assert int(((lossy >> pxb.COVER_BIT["R2S_REPEAT"]) & 1).sum()) == 5          # the rarest: 5 of 3,000


# ---- 2. counts off the wave size, count 0, bad and bailed rows -------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 65, 130])
def test_counts_that_are_no_multiple_of_64(n):
    cfg, ids, masks, steps = CO.case_oracle("lossy-p2n3")
    _, _, _, s = check_call(cfg, pxb.scripts_empty(cfg, ids[:n], 0), 0, masks[:n], steps[:n])
    if n == 0:
        assert s.counts == [0] * 29 and s.witness == [NONE64] * 29 and s.witness_steps == [0xFFFFFFFF] * 29
        assert (s.rows_ok, s.rows_bailed, s.rows_bad, s.union) == (0, 0, 0, 0)


def test_bad_and_bailed_rows_count_under_no_class():
    cfg, rows, i_bad, i_bail = CO.bad_and_bailed_rows()
    assert SO.host_run(cfg, rows[i_bail], 0)["status"][0] == pxb.TRACE_BAILED      # (the scripted run bails on it too)
    rc, m, st, res, s = CO.host_cover(cfg, rows, 0)
    assert rc == 0
    CO.check_bad_and_bailed(cfg, rows, i_bad, i_bail, m, st, res, s)


# ---- 3. the hand-derived rows ------------------------------------------------------------
KATS = CO.kat_cases()


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_hand_derived_rows(case):
    cfg, row, depth = CO.kat_row(case)
    want = sum(1 << pxb.COVER_BIT[n] for n in case["mask"])
    events, summary = EO.oracle_events(cfg, row, depth)
    packed = EO.pack(events)
    per_oracle = CO.fold(events, cfg.n_acceptors, per_event=True)
    per_spec = pxb.cover_of_events(packed, cfg.n_acceptors, per_event=True)
    assert per_oracle == per_spec and len(events) == case["n_events"]
    assert CO.fold(events, cfg.n_acceptors) == pxb.cover_of_events(packed, cfg.n_acceptors) == want
    rc, m, st, res, s = CO.host_cover(cfg, row, depth)
    assert rc == 0 and st[0] == pxb.TRACE_OK and m[0] == want and res[0, 3] >> 16 == case["steps"] == summary[4]
    assert pxb.cover_names(int(m[0])) == case["mask"]
    if "class" in case:
        bit = pxb.COVER_BIT[case["class"]]
        first = next(i for i, x in enumerate(per_spec) if (x >> bit) & 1)
        assert first == case["event_index"] and pxb.event_lines(packed[first:first + 1]) == [case["event_line"]]
        assert s.witness[bit] == 0 and s.witness_steps[bit] == case["steps"] and s.counts[bit] == 1


def test_the_benign_row_and_its_lost_propose():
    benign, lost = (set(c["mask"]) for c in KATS[:2])
    assert benign == {"ASK_GRANT_EMPTY", "PROPOSE_ACCEPT", "EXEC_APPLY", "TICK_START", "R1OK_ACK", "R1OK_PROPOSE_OWN",
                      "R1OK_STALE", "R2S_ACK", "R2S_DONE", "R2S_DROPPED"}
    assert lost - benign == {"EXEC_PANIC"} and benign - lost == {"R2S_DROPPED"}
    witnesses = {c["class"]: int(c["name"].rsplit("id", 1)[1]) for c in KATS[2:]}
    assert witnesses == {"Q1_FOREIGN_ACCEPT": 1661, "Q7_STALE_EXEC": 47, "HAVE_ABORT_R2": 302, "R2S_REPEAT": 1911}
    # the oracle's shortest of the lossy case, ties to the lowest id
    cfg, ids, masks, steps = CO.case_oracle("lossy-p2n3")
    for name, inst in witnesses.items():
        has = np.nonzero((masks >> pxb.COVER_BIT[name]) & 1)[0]
        assert inst == int(has[np.lexsort((has, steps[has]))[0]])


def test_names_and_constants_mirror_the_header(tmp_path):
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"paxos_batch.h\"\nint main(void) {\n"
    src += "".join('  printf("%%u\\n", PXB_COVER_%s);\n' % n for n in pxb.COVER_NAMES)
    src += ('  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(pxb_cover_summary), '
            'offsetof(pxb_cover_summary, rows_bailed), offsetof(pxb_cover_summary, n_matches), '
            'offsetof(pxb_cover_summary, count), offsetof(pxb_cover_summary, witness), '
            'offsetof(pxb_cover_summary, witness_steps), offsetof(pxb_cover_summary, union_mask), '
            'sizeof(pxb_cover_query), offsetof(pxb_cover_query, none_mask), PXB_COVER_CLASSES, PXB_ABI_VERSION);\n'
            '  return 0;\n}\n')
    tmp = str(tmp_path / "pxb_cover_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(EO.ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:29] == [1 << i for i in range(29)] == [getattr(pxb, "COVER_" + n) for n in pxb.COVER_NAMES]
    assert got[29:] == [680, 8, 24, 32, 288, 544, 672, 16, 8, 29, 5]
    S, Q = pxb.pxb_cover_summary, pxb.pxb_cover_query
    assert [C.sizeof(S), S.rows_bailed.offset, S.n_matches.offset, S.count.offset, S.witness.offset,
            S.witness_steps.offset, S.union_mask.offset, C.sizeof(Q), Q.none_mask.offset] == got[29:38]
    assert list(pxb.COVER_NAMES) == list(CO.BIT) and pxb.COVER_CLASSES == 29
    assert pxb.cover_names(pxb.COVER_Q1_FOREIGN_ACCEPT | pxb.COVER_R2S_REPEAT) == ["Q1_FOREIGN_ACCEPT", "R2S_REPEAT"]
    assert [pxb.COVER_NAMES[i] for i in (pxb.COVER_Q1, pxb.COVER_Q7, pxb.COVER_Q10, pxb.COVER_Q5, pxb.COVER_Q4,
                                         pxb.COVER_Q2)] == ["Q1_FOREIGN_ACCEPT", "Q7_STALE_EXEC", "HAVE_ABORT_R2",
                                                            "Q5_ADOPTED_OWN", "Q4_TIE", "R2S_REPEAT"]
    lib_ = pxb.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_cover", "pxb_cover_device", "pxb_cover_range"):
        assert " T %s\n" % name in out and hasattr(lib_, name)


# ---- 4. validation ------------------------------------------------------------------------
def test_cover_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call; a valid call is
    PXB_E_NODEV without a GPU.  The host build refuses the same configs."""
    import torch
    L = pxb.load()
    cfg = pxb.CONFIGS[3]
    depth = 4
    rows = pxb.scripts_empty(cfg, range(8), depth)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    summ = pxb.pxb_cover_summary()

    def calls(cfg_, rows_p=P(rows), count=8, depth_=depth, flags=0):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= flags
        cp = C.byref(c) if c is not None else None
        return [L.pxb_cover(cp, rows_p, count, depth_, None, None, None, C.byref(summ)),
                L.pxb_cover_device(cp, rows_p, count, depth_, None, None, None, None, None)]

    def ranges(cfg_, count=8, chunk=0, q=None, ids_p=None, max_matches=0, flags=0):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= flags
        return L.pxb_cover_range(C.byref(c) if c is not None else None, 0, count, chunk,
                                 C.byref(q) if q is not None else None, ids_p, None, max_matches, C.byref(summ))

    inval = [pxb.PXB_E_INVAL] * 2
    assert calls(None) == inval and ranges(None) == pxb.PXB_E_INVAL
    assert calls(cfg, rows_p=None) == inval
    assert calls(cfg, depth_=4097) == inval
    assert calls(cfg, count=(1 << 30) + 1) == inval
    assert calls(cfg, flags=pxb.CFG_TRACE_PRODUCTION) == inval
    assert ranges(cfg, flags=pxb.CFG_TRACE_PRODUCTION) == pxb.PXB_E_INVAL
    assert ranges(cfg, chunk=(1 << 30) + 1) == pxb.PXB_E_INVAL
    assert ranges(cfg, q=pxb.pxb_cover_query(0, 0, 0, 1)) == pxb.PXB_E_INVAL           # reserved
    assert ranges(cfg, q=pxb.pxb_cover_query(1, 0, 0, 0), max_matches=4) == pxb.PXB_E_INVAL   # a list with no ids buffer
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=10),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=4096),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9)):
        assert calls(bad) == inval and ranges(bad) == pxb.PXB_E_INVAL, bad
        assert CO.host_cover(bad, rows, depth)[0] == pxb.PXB_E_INVAL
    assert CO.host_cover(cfg, rows, depth, cflags=pxb.CFG_TRACE_PRODUCTION)[0] == pxb.PXB_E_INVAL
    # the device form: alignment (an INVAL before any device call)
    c = cfg.to_c(0, 1)
    raw = np.zeros(1024, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16
    for k, off in ((4, 2), (5, 2), (6, 8), (7, 4)):                  # masks, status, results, summary
        args = [C.byref(c), P(rows), 8, depth, None, None, None, None, None]
        args[k] = C.c_void_p(base + off)
        assert L.pxb_cover_device(*args) == pxb.PXB_E_INVAL, k
    assert L.pxb_cover_device(C.byref(c), C.c_void_p(base + 4), 8, depth, None, None, None, None, None) == pxb.PXB_E_INVAL
    if not torch.cuda.is_available():
        assert calls(cfg) == [pxb.PXB_E_NODEV] * 2
        assert calls(cfg, rows_p=None, count=0) == [pxb.PXB_E_NODEV] * 2
        assert ranges(cfg) == pxb.PXB_E_NODEV and ranges(cfg, count=0) == pxb.PXB_E_NODEV
        for call in (lambda: pxb.cover(cfg, rows, depth), lambda: pxb.cover_ids(cfg, [1, 2]),
                     lambda: pxb.cover_range(cfg, 0, 16)):
            with pytest.raises(pxb.PaxosError):
                call()
    with pytest.raises(ValueError, match="required"):
        pxb.cover_device(cfg, None, 4, depth)
    assert pxb.CoverQuery(all_mask=1, none_mask=4).matches(3) and not pxb.CoverQuery(all_mask=1, none_mask=4).matches(5)
    assert not pxb.CoverQuery(any_mask=6).matches(1) and pxb.CoverQuery().matches(0)


# ---- 5. one stand-alone sanitizer program ------------------------------------------------
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_COVER_HOST_MAIN",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
             "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_cover_core_sanitized():
    """cover_host.cpp with its own main (N = 3 on the 8-step wheel) under
    AddressSanitizer + UBSan, one subprocess per case: the first 130 ids of the
    N = 3 cases on that wheel, and the hand-derived rows.  Exit status 0, and the
    output equals the unsanitized host build's."""
    if CO.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([CO.HIPCC, *SAN_FLAGS, "-o", tmp, CO.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    e = dict(os.environ)
    e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    jobs = []
    for name in ("config1-p1n3", "lossy-p2n3", "windows-p2n3", "log-p2n3"):
        cfg, ids, _, _ = CO.case_oracle(name, 130)
        jobs.append((name, cfg, pxb.scripts_empty(cfg, ids, 0), 0))
    for case in KATS:
        cfg, row, depth = CO.kat_row(case)
        jobs.append((case["name"], cfg, row[None, :], depth))
    with tempfile.TemporaryDirectory() as td:
        for name, cfg, rows, depth in jobs:
            rc, m, st, res, s = CO.host_cover(cfg, rows, depth)
            c = cfg.to_c(0, 1)
            inp, out = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
            with open(inp, "wb") as f:
                f.write(bytes(c) + struct.pack("<IQ", depth, len(rows)) + rows.tobytes())
            p = subprocess.run([EXE, inp, out], capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode == 0, "sanitized run failed (rc %d): %s" % (p.returncode, p.stderr[-4000:])
            raw = open(out, "rb").read()
            n = len(rows)
            assert raw[:4 * n] == m.tobytes() and raw[4 * n:8 * n] == st.tobytes(), name
            assert raw[8 * n:24 * n] == res.tobytes(), name
            assert pxb.cover_summary_from(raw[24 * n:]) == s, name
