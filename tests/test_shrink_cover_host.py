"""The shrinker over a coverage predicate (docs/SEMANTICS.md §16) without a GPU.

The logic the kernels share (csrc/shrink_cover_core.h: ShrinkEventDraws under
CoverLane, the candidate's start and predicate; csrc/shrink_core.h: the rank
tables, select and settle, the signature) is compiled for the HOST
(tests/native/shrink_cover_host.cpp) and checked, instance by instance and bit
for bit, against pxb.shrink_cover with the host runners of the scripted lane and
of the coverage lane; then the C-ABI boundary of the new entry points, and one
stand-alone AddressSanitizer + UBSan program (its own main; nothing is loaded
into Python)."""
import ctypes as C
import dataclasses
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cover_oracle as CO
import pxb
import script_oracle as SO
import shrink_cover_oracle as HC
import shrink_oracle as H
from test_shrink_gpu import UNIT_SHAPES
from test_shrink_host import C3_INPUTS

Q = pxb.CoverQuery
B = CO.BIT
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "shrink_cover_host_san")
EXE_PLAIN = os.path.join(HERE, "native", "_build", "shrink_cover_host_plain")
LOSSY = CO._LOSSY
HAVE_ANY = B["HAVE_IDLE"] | B["HAVE_BELOW"] | B["HAVE_RESTART_R1"] | B["HAVE_ABORT_R2"]
_runs = {}


def run_case(cfg, n, query, flag_mask=0, depth=64):
    """(rows given, host-batch outputs, references) of ids 0..n-1, every instance checked; run once."""
    key = (repr(cfg), n, repr(query), flag_mask, depth)
    if key not in _runs:
        rows = SO.host_extract(cfg, range(n), depth)
        o = HC.host_batch(cfg, np.arange(n), query, flag_mask, depth=depth)
        rr = [HC.reference(cfg, rows[i], query, flag_mask, depth=depth, runner=HC.host_runner) for i in range(n)]
        for i, ref in enumerate(rr):
            HC.check(cfg, o, i, ref, depth)
        _runs[key] = (rows, o, rr)
    return _runs[key]


def stats(o, rr):
    """inputs, (min, max) launches and faults left over them, the histogram of faults left, distinct signatures."""
    inputs = [i for i, r in enumerate(rr) if r["status"] != pxb.SHRINK_NOT_INPUT]
    la = [int(o["launches"][i]) for i in inputs]
    nf = [int(o["n_faults"][i]) for i in inputs]
    hist = {v: nf.count(v) for v in sorted(set(nf))}
    sigs = len({int(o["sig"][i]) for i in inputs})
    print("inputs", len(inputs), inputs[:8], "launches", (min(la), max(la)) if la else None,
          "faults", (min(nf), max(nf)) if nf else None, "hist", hist, "signatures", sigs)
    return inputs, ((min(la), max(la)) if la else None), ((min(nf), max(nf)) if nf else None), hist, sigs


# ---- the reference cases -------------------------------------------------------------------------
def test_lossy_q1():
    _, o, rr = run_case(LOSSY, 256, Q(all_mask=B["Q1_FOREIGN_ACCEPT"]))
    inputs, la, nf, hist, sigs = stats(o, rr)
    assert len(inputs) == 76 and inputs[:7] == [0, 3, 5, 10, 11, 14, 15]
    assert la == (4, 20) and nf == (1, 19) and (hist[1], hist[2], hist[3]) == (24, 18, 23) and sigs == 54
    assert all(o["masks"][i] & B["Q1_FOREIGN_ACCEPT"] for i in inputs)


def test_lossy_q7():
    _, o, rr = run_case(LOSSY, 256, Q(all_mask=B["Q7_STALE_EXEC"]))
    inputs, la, nf, _, sigs = stats(o, rr)
    assert len(inputs) == 27 and inputs[:4] == [4, 11, 37, 47]
    assert la == (6, 28) and nf == (1, 24) and sigs == 22


def test_lossy_have_abort_without_panic():
    _, o, rr = run_case(LOSSY, 256, Q(all_mask=B["HAVE_ABORT_R2"], none_mask=B["EXEC_PANIC"]))
    inputs, la, nf, _, sigs = stats(o, rr)
    assert len(inputs) == 127 and la == (4, 12) and nf == (1, 6) and sigs == 87
    assert all(not o["masks"][i] & B["EXEC_PANIC"] for i in inputs)


def test_lossy_no_input_at_all():
    """R2S_REPEAT: no id has it, every row is NOT_INPUT, untouched, launches 1, with its own mask."""
    rows, o, rr = run_case(LOSSY, 256, Q(all_mask=B["R2S_REPEAT"]))
    assert (o["status"] == pxb.SHRINK_NOT_INPUT).all() and (o["rows"] == rows).all() and (o["launches"] == 1).all()
    assert (o["masks"] == CO.host_cover(LOSSY, rows, 64)[1]).all() and o["masks"].any()


def test_lossy_done_without_nacks():
    q = Q(all_mask=B["R2S_DONE"], none_mask=B["ASK_NACK"] | B["PROPOSE_NACK"] | HAVE_ANY)
    _, o, rr = run_case(LOSSY, 64, q)
    inputs, la, nf, _, sigs = stats(o, rr)
    assert inputs == [27] and la == (4, 4) and nf == (3, 3) and sigs == 1


def test_windows_discard_isolated():
    _, o, rr = run_case(CO.CASES["windows-p2n3"][0], 64, Q(all_mask=B["DISCARD_ISOLATED"]))
    inputs, la, nf, hist, sigs = stats(o, rr)
    assert len(inputs) == 30 and la == (4, 6) and hist == {1: 28, 2: 2} and sigs == 29


def test_log_tick_busy_is_benign():
    """A predicate the benign schedule holds: every row shrinks to no faults."""
    _, o, rr = run_case(CO.CASES["log-p2n3"][0], 64, Q(all_mask=B["TICK_BUSY"]))
    inputs, la, nf, _, sigs = stats(o, rr)
    assert len(inputs) == 64 and la == (3, 7) and nf == (0, 0) and sigs == 1
    assert (o["status"] == pxb.SHRINK_MINIMAL).all()


def test_log_tick_busy_and_q7():
    _, o, rr = run_case(CO.CASES["log-p2n3"][0], 64, Q(all_mask=B["TICK_BUSY"] | B["Q7_STALE_EXEC"]))
    inputs, la, nf, _, sigs = stats(o, rr)
    assert inputs == [5, 14, 17, 21, 50, 54, 62] and la == (6, 14) and nf == (1, 18) and sigs == 7


def test_config3_q1():
    _, o, rr = run_case(pxb.CONFIGS[3], 64, Q(all_mask=B["Q1_FOREIGN_ACCEPT"]))
    inputs, la, nf, _, sigs = stats(o, rr)
    assert len(inputs) == 27 and inputs[:5] == [2, 3, 5, 10, 14]
    assert la == (4, 24) and nf == (1, 45) and sigs == 22


# ---- equivalence with the existing shrinker ------------------------------------------------------
def test_equals_shrink_batch_with_a_zero_query():
    """Config 3 ids 0..63, all-zero query, F_PANIC: every output is the existing
    shrinker's (its 24 inputs), and the masks are host_cover of the returned rows."""
    cfg = pxb.CONFIGS[3]
    o = HC.host_batch(cfg, np.arange(64), None, pxb.F_PANIC)
    s = H.host_batch(cfg, np.arange(64), pxb.F_PANIC)
    for k in s:
        assert (o[k] == s[k]).all(), k
    assert [i for i in range(64) if o["status"][i] != pxb.SHRINK_NOT_INPUT] == C3_INPUTS
    assert (o["masks"] == CO.host_cover(cfg, o["rows"], 64)[1]).all()
    ref = HC.reference(cfg, s["rows"][0], None, pxb.F_PANIC, runner=HC.host_runner)     # (a shrunk row: its own fixed point)
    assert ref["status"] == pxb.SHRINK_MINIMAL and (ref["row"] == s["rows"][0]).all()


# ---- the flag and the query together, every shape ------------------------------------------------
ANY_FAULTY = B["DISCARD_DEAD"] | B["DISCARD_ISOLATED"] | B["ASK_NACK"] | B["PROPOSE_NACK"]
UNIT_INPUTS = {"2-1": 2, "2-2": 62, "2-3": 64, "9-1": 34, "9-2": 21, "9-3": 1, "3-2-wheel16": 43}


def unit_config(P, N, delay_max):
    """test_shrink_gpu.test_every_kernel_unit's config."""
    return pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                      delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                      step_cap=256)


@pytest.mark.parametrize("P,N,delay_max,depth", UNIT_SHAPES)
def test_flag_and_query_every_shape(request, P, N, delay_max, depth):
    cfg = unit_config(P, N, delay_max)
    name = request.node.callspec.id
    _, o, rr = run_case(cfg, 64, Q(any_mask=ANY_FAULTY), 0x3F, depth=depth)
    inputs, la, nf, _, _ = stats(o, rr)
    assert len(inputs) == UNIT_INPUTS[name]
    if name == "9-2":
        assert la[1] == 24
    if name == "9-3":
        assert inputs == [49] and la == (22, 22) and nf == (20, 20)
    if name in ("2-1", "9-1"):                          # the query is doing work: the flags alone admit more
        rows = SO.host_extract(cfg, range(64), depth)
        res, status, sent = SO.host_runner(cfg, rows, depth)
        flag_only = sum(bool(status[i] == pxb.TRACE_OK and int(res[i][3]) & 0x3F and int(sent[i].max()) <= depth)
                        for i in range(64))
        assert flag_only == {"2-1": 37, "9-1": 43}[name]


# ---- the budget ----------------------------------------------------------------------------------
@pytest.mark.parametrize("max_launches", [1, 2, 3, 7])
def test_budget(max_launches):
    """The Q1 case's row with the most launches (20), cut short: BUDGET, as the reference."""
    q = Q(all_mask=B["Q1_FOREIGN_ACCEPT"])
    given, full, _ = run_case(LOSSY, 256, q)
    i = int(np.argmax(full["launches"]))
    assert full["launches"][i] == 20
    o = HC.host_batch(LOSSY, given[i:i + 1], q, max_launches=max_launches)
    ref = HC.reference(LOSSY, given[i], q, max_launches=max_launches, runner=HC.host_runner)
    HC.check(LOSSY, o, 0, ref, 64)
    print("id", i, "launches", ref["launches"], "faults", len(ref["faults"]))
    assert o["status"][0] == pxb.SHRINK_BUDGET and o["launches"][0] == (max_launches - 1) | 1
    assert o["n_faults"][0] >= full["n_faults"][i]


# ---- batch independence --------------------------------------------------------------------------
def test_batch_independence():
    """The Q1 case's first 64 ids shuffled, with repeats and non-inputs interleaved."""
    q = Q(all_mask=B["Q1_FOREIGN_ACCEPT"])
    rows, o, _ = run_case(LOSSY, 256, q)
    rng = np.random.default_rng(7)
    order = np.concatenate([rng.permutation(64), rng.integers(0, 64, 16), [10, 10, 1, 10]])
    s = HC.host_batch(LOSSY, rows[order], q)
    for k in HC.KEYS:
        assert (s[k] == o[k][order]).all(), k


# ---- 1-minimality --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["q1", "abort", "log"])
def test_one_minimal(case):
    cfg, n, q = {"q1": (LOSSY, 256, Q(all_mask=B["Q1_FOREIGN_ACCEPT"])),
                 "abort": (LOSSY, 256, Q(all_mask=B["HAVE_ABORT_R2"], none_mask=B["EXEC_PANIC"])),
                 "log": (CO.CASES["log-p2n3"][0], 64, Q(all_mask=B["TICK_BUSY"] | B["Q7_STALE_EXEC"]))}[case]
    _, o, _ = run_case(cfg, n, q)
    HC.one_minimal(cfg, o, q, 0, 64, HC.host_runner)


# ---- the C-ABI boundary --------------------------------------------------------------------------
def test_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call (so on every
    host); the struct's size; the ABI version stays 5."""
    L = pxb.load()
    cfg = pxb.CONFIGS[3]
    depth = 4
    rows = pxb.scripts_empty(cfg, range(8), depth)
    out = np.zeros(8 * 64, np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    base = out.ctypes.data + (-out.ctypes.data % 16)
    assert C.sizeof(pxb.pxb_shrink_pred) == 32 and pxb.pxb_shrink_pred.q.offset == 16

    def calls(cfg_, rows_p=P(rows), count=8, depth_=depth, pr=HC.pred(None, pxb.F_PANIC), which=(0, 1), dev_out=None,
              cflags=0):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= cflags
        cp = C.byref(c) if c is not None else None
        pp = C.byref(pr) if pr is not None else None
        d = dev_out or [None] * 7
        fns = (lambda: L.pxb_shrink_cover_batch(cp, None, rows_p, count, depth_, pp, *([None] * 7)),
               lambda: L.pxb_shrink_cover_batch_device(cp, rows_p, count, depth_, pp, *d, None))
        return [fns[i]() for i in which]

    def inval(*a, **kw):
        got = calls(*a, **kw)
        return len(got) > 0 and all(rc == pxb.PXB_E_INVAL for rc in got)

    def with_(**kw):
        pr = HC.pred(None, pxb.F_PANIC)
        for k, v in kw.items():
            if k in ("all_mask", "any_mask", "none_mask", "qreserved"):
                setattr(pr.q, "reserved" if k == "qreserved" else k, v)
            elif k in ("r0", "r1"):
                pr.reserved[int(k[1])] = v
            else:
                setattr(pr, k, v)
        return pr
    assert inval(None)                                                    # null cfg
    assert inval(cfg, rows_p=None)                                        # null rows, count > 0
    assert inval(cfg, depth_=4097)                                        # depth > 4096
    assert inval(cfg, count=(1 << 30) + 1)                                # count > 2^30
    assert inval(cfg, pr=None)                                            # null pred
    assert inval(cfg, pr=with_(flag_mask=0x100)) and inval(cfg, pr=with_(flag_mask=0x180))
    assert inval(cfg, pr=with_(max_launches=0))
    assert inval(cfg, pr=with_(r0=1)) and inval(cfg, pr=with_(r1=1)) and inval(cfg, pr=with_(qreserved=1))
    for k in ("all_mask", "any_mask", "none_mask"):
        assert inval(cfg, pr=with_(**{k: 1 << 29})) and inval(cfg, pr=with_(**{k: 1 << 31})), k
    assert inval(cfg, cflags=pxb.CFG_TRACE_PRODUCTION)
    assert inval(cfg, rows_p=C.c_void_p(rows.ctypes.data + 4), which=(1,))   # misaligned rows
    for slot, off in ((0, 2), (1, 2), (2, 2), (3, 1), (4, 8), (5, 4), (6, 2)):   # status .. signature, masks
        d = [None] * 7
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
    assert L.pxb_abi_version() == 5 and pxb.ABI_VERSION == 5
    import torch
    if not torch.cuda.is_available():                                     # valid calls, no GPU
        assert calls(cfg, which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(cfg, pr=HC.pred(None, 0), which=(0,)) == [pxb.PXB_E_NODEV]    # flag_mask 0, all-zero query
        assert calls(cfg, pr=HC.pred(Q(all_mask=1 << 28), 0), which=(0,)) == [pxb.PXB_E_NODEV]
        assert calls(cfg, count=0, rows_p=None, which=(0,)) == [pxb.PXB_E_NODEV]


def test_python_argument_checks():
    cfg = pxb.CONFIGS[3]
    q = Q(all_mask=B["Q1_FOREIGN_ACCEPT"])
    with pytest.raises(ValueError):
        pxb.shrink_cover_batch(cfg, [1, 2], q, chunk=0)
    with pytest.raises(ValueError):
        pxb.shrink_cover_batch(cfg, [1, 2], q, depth=4097)
    with pytest.raises(ValueError):
        pxb.shrink_cover_batch(cfg, np.zeros((2, 7), np.uint8), q)
    row = SO.host_extract(cfg, [0], 8)
    with pytest.raises(ValueError):
        pxb.shrink_cover(cfg, row, Q(all_mask=1 << 29), runner=HC.host_runner, depth=8)
    with pytest.raises(ValueError):
        pxb.shrink_cover(cfg, row, q, flag_mask=0x100, runner=HC.host_runner, depth=8)
    with pytest.raises(ValueError):
        pxb.shrink_cover(cfg, np.concatenate([row, row]), q, runner=HC.host_runner, depth=8)
    with pytest.raises(ValueError):                      # no input: R2S_REPEAT and its absence at once
        pxb.shrink_cover(cfg, row, Q(all_mask=B["R2S_REPEAT"], none_mask=B["R2S_REPEAT"]), runner=HC.host_runner, depth=8)
    # pxb.shrink through the shared loop: its 3-tuple runner and its 3-tuple result
    r, faults, launches = pxb.shrink(cfg, SO.host_extract(cfg, [0], 64), pxb.F_PANIC, runner=SO.host_runner)
    assert launches >= 2 and faults and r.shape == (pxb.script_stride(cfg, 64),)


# ---- one stand-alone sanitizer program -----------------------------------------------------------
SAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAIN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_SHRINK_COVER_HOST_MAIN",
              "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_shrink_cover_core_sanitized():
    """shrink_cover_host.cpp with its own main (one shape: P = 2, N = 3, W = 8)
    under AddressSanitizer + UBSan, as a subprocess over the lossy config's ids
    0..31 at depth 12 with the Q1 query, every buffer sized exactly: exit status
    0, and the output equals the unsanitized build's and the library build's."""
    for exe, extra in ((EXE, SAN_FLAGS), (EXE_PLAIN, [])):
        if HC.stale(exe):
            os.makedirs(os.path.dirname(exe), exist_ok=True)
            tmp = "%s.%d" % (exe, os.getpid())
            subprocess.run([SO.HIPCC, *MAIN_FLAGS, *extra, "-o", tmp, HC.SRC], check=True, timeout=900)
            os.replace(tmp, exe)
    n, depth = 32, 12
    q = Q(all_mask=B["Q1_FOREIGN_ACCEPT"])
    got = []
    with tempfile.TemporaryDirectory() as td:
        inp = os.path.join(td, "i.bin")
        with open(inp, "wb") as f:
            f.write(bytes(LOSSY.to_c(0, 1)) + bytes(HC.pred(q)) + np.array([depth], "<u4").tobytes() +
                    np.array([0, n], "<u8").tobytes())
        for exe in (EXE, EXE_PLAIN):
            out = os.path.join(td, "o.bin")
            e = dict(os.environ)
            e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
            p = subprocess.run([exe, inp, out], capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode == 0, "%s failed (rc %d): %s" % (exe, p.returncode, p.stderr[-4000:])
            got.append(np.fromfile(out, dtype=np.uint8))
    assert len(got[0]) == len(got[1]) and (got[0] == got[1]).all()
    o = HC.host_batch(LOSSY, np.arange(n), q, depth=depth)
    want = np.concatenate([o[k].reshape(-1).view(np.uint8) for k in HC.KEYS])
    assert len(want) == len(got[0]) and (want == got[0]).all()
    assert (o["status"] != pxb.SHRINK_NOT_INPUT).any()
