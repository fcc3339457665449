"""The HOST-buffer forms of the C ABI, called through ctypes as a C caller
would: what a form writes to an output does not depend on which other optional
outputs were asked for; the tracing forms truncate to the capacity and write
nothing behind it; count == 0 touches nothing; pxb_explore's chunking, the two
inputs of pxb_shrink_batch, the wire host forms and the handler hooks.

Config 3 (P = 2, N = 5), 130 ids or rows (two full waves and a partial one),
depth 8, rows from pxb_schedule_extract."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_c
import pxb

pytestmark = pytest.mark.gpu
CFG = pxb.CONFIGS[3]
P, N = CFG.n_proposers, CFG.n_acceptors
COUNT, DEPTH, GUARD = 130, 8, 0xA5
IDS = np.arange(1000, 1000 + COUNT, dtype=np.uint64)
STEP_BYTES, EVENT_BYTES = 4 * pxb.TRACE_WORDS, pxb.EVENT_BYTES
_cache = {}


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def guard(shape, dtype):
    """An output buffer prefilled with the guard byte."""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = GUARD
    return a


def cfg_c(cfg=CFG, n=1):
    return cfg.to_c(0, n)


def rows_of(lib):
    """The 130 rows, extracted once by the host form."""
    if "rows" not in _cache:
        rows = guard((COUNT, pxb.script_stride(CFG, DEPTH)), np.uint8)
        assert lib.pxb_schedule_extract(C.byref(cfg_c()), ptr(IDS), COUNT, DEPTH, ptr(rows)) == 0
        assert lib.pxb_script_stride(P, N, DEPTH) == rows.shape[1]
        _cache["rows"] = rows
    return _cache["rows"]


def each_alone(call, spec, always=()):
    """call(bufs) with every output of `spec` (name -> (shape, dtype)) given,
    then with each alone: a given output equals the full call's byte for byte.
    `always` names outputs handed to every call.  Returns the full call's."""
    full = {k: guard(*v) for k, v in spec.items()}
    assert call(full) == 0
    assert any((b.view(np.uint8) != GUARD).any() for b in full.values())
    for k in spec:
        if k in always:
            continue
        one = {j: guard(*spec[j]) if j == k or j in always else None for j in spec}
        assert call(one) == 0, k
        for j, b in one.items():
            assert b is None or b.tobytes() == full[j].tobytes(), (k, j)
    return full


# ---- optional outputs -----------------------------------------------------------------------
def test_run_scripted_outputs_alone(gpu_lib):
    rows = rows_of(gpu_lib)
    spec = {"out": ((COUNT, 4), np.uint32), "dig": ((COUNT, N), np.uint32), "acc": ((COUNT, N, 4), np.uint32),
            "status": ((COUNT,), np.uint32), "sent": ((COUNT, 2, P, N), np.uint16)}

    def call(b):
        return gpu_lib.pxb_run_scripted(C.byref(cfg_c()), ptr(rows), COUNT, DEPTH, ptr(b["out"]), ptr(b["dig"]),
                                        ptr(b["acc"]), ptr(b["status"]), ptr(b["sent"]))
    full = each_alone(call, spec)
    assert (full["status"] == pxb.TRACE_OK).any()


SHRINK_SPEC = {"rows": None, "status": ((COUNT,), np.uint32), "n_faults": ((COUNT,), np.uint32),
               "launches": ((COUNT,), np.uint32), "sent": ((COUNT, 2, P, N), np.uint16),
               "results": ((COUNT, 4), np.uint32), "signature": ((COUNT,), np.uint64)}


def shrink_call(lib, rows0, ids=None):
    def call(b):
        if ids is None:
            b["rows"][...] = rows0                   # (in and out: every call starts from the same rows)
        return lib.pxb_shrink_batch(C.byref(cfg_c()), ptr(ids), ptr(b["rows"]), COUNT, DEPTH, 0xFF, 64,
                                    ptr(b["status"]), ptr(b["n_faults"]), ptr(b["launches"]), ptr(b["sent"]),
                                    ptr(b["results"]), ptr(b["signature"]))
    return call


def test_shrink_batch_outputs_alone_and_both_inputs(gpu_lib):
    rows0 = rows_of(gpu_lib)
    spec = dict(SHRINK_SPEC, rows=(rows0.shape, np.uint8))
    full = each_alone(shrink_call(gpu_lib, rows0), spec, always=("rows",))
    # the ids given: the rows are extracted on the device first
    by_ids = {k: guard(*v) for k, v in spec.items()}
    assert shrink_call(gpu_lib, rows0, IDS)(by_ids) == 0
    for k in spec:
        assert by_ids[k].tobytes() == full[k].tobytes(), k


def trace_forms(lib):
    """name -> (entry point, record bytes, the arguments before the selection)."""
    rows, c = rows_of(lib), cfg_c()
    return {"trace_batch": (lib.pxb_trace_batch, STEP_BYTES, (C.byref(c), ptr(IDS), COUNT), c),
            "trace_scripted": (lib.pxb_trace_scripted, STEP_BYTES, (C.byref(c), ptr(rows), COUNT, DEPTH), c),
            "trace_events": (lib.pxb_trace_events, EVENT_BYTES, (C.byref(c), ptr(rows), COUNT, DEPTH), c)}


def trace_call(fn, head, rec, capacity, b):
    """One call of a tracing form; b: records, offsets, status, results, n_records (offsets required)."""
    return fn(*head, None, ptr(b["records"]) if capacity else None, capacity, ptr(b["offsets"]), ptr(b["status"]),
              ptr(b["results"]), ptr(b["n_records"]))


def trace_total(fn, head):
    """offsets[count] of a capacity = 0 sizing call."""
    offs = guard((COUNT + 1,), np.uint64)
    assert fn(*head, None, None, 0, ptr(offs), None, None, None) == 0
    return int(offs[COUNT])


@pytest.mark.parametrize("name", ["trace_batch", "trace_scripted", "trace_events"])
def test_trace_outputs_alone_and_truncation(gpu_lib, name):
    fn, rec, head, _keep = trace_forms(gpu_lib)[name]
    total = trace_total(fn, head)
    assert total > 2
    spec = {"records": ((total + 64, rec), np.uint8), "offsets": ((COUNT + 1,), np.uint64),
            "status": ((COUNT,), np.uint32), "results": ((COUNT, 4), np.uint32), "n_records": ((1,), np.uint64)}
    full = each_alone(lambda b: trace_call(fn, head, rec, total if b["records"] is not None else 0, b), spec,
                      always=("offsets",))
    assert int(full["n_records"][0]) == total == int(full["offsets"][COUNT])
    assert (np.diff(full["offsets"].astype(np.int64)) >= 0).all() and full["offsets"][0] == 0
    assert (full["records"][total:] == GUARD).all()
    for capacity in (0, 1, total - 1, total, total + 64):
        b = {k: guard(*v) for k, v in spec.items()}
        assert trace_call(fn, head, rec, capacity, b) == 0, capacity
        m = min(total, capacity)
        assert b["records"][:m].tobytes() == full["records"][:m].tobytes(), capacity
        assert (b["records"][m:] == GUARD).all(), capacity
        for k in ("offsets", "status", "results", "n_records"):
            assert b[k].tobytes() == full[k].tobytes(), (capacity, k)


def explore_call(lib, cfg, rows, depth, space, capacity, b):
    return lib.pxb_explore(C.byref(cfg_c(cfg)), ptr(rows), len(rows), depth, C.byref(space),
                           ptr(b["ids"]) if capacity else None, capacity, ptr(b["n_matches"]), ptr(b["counts"]),
                           ptr(b["status"]))


def test_explore_outputs_alone(gpu_lib):
    rows = rows_of(gpu_lib)
    space = pxb.pxb_explore_space(1, 1, 0xFF, 0)            # T = 1 + 2 P N delay_max = 81 a parent
    T = pxb.explore_total(CFG, 1, 1)
    spec = {"ids": ((COUNT * T,), np.uint64), "n_matches": ((1,), np.uint64), "counts": ((COUNT, 4, 3), np.uint32),
            "status": ((COUNT,), np.uint32)}
    full = each_alone(lambda b: explore_call(gpu_lib, CFG, rows, DEPTH, space, COUNT * T if b["ids"] is not None else 0, b),
                      spec, always=("n_matches",))
    k = int(full["n_matches"][0])
    assert k <= COUNT * T and (full["ids"][k:].view(np.uint8) == GUARD).all()
    assert (np.diff(full["ids"][:k].astype(np.int64)) > 0).all()


def test_run_outputs_alone(gpu_lib):
    spec = {"out": ((COUNT, 4), np.uint32), "dig": ((COUNT, N), np.uint32), "acc": ((COUNT, N, 4), np.uint32),
            "totals": ((pxb.NCOUNTERS,), np.int64)}

    def call(b):
        return gpu_lib.pxb_run(C.byref(CFG.to_c(1000, COUNT)), ptr(b["out"]), ptr(b["dig"]), ptr(b["acc"]),
                               ptr(b["totals"]))
    full = each_alone(call, spec)
    assert pxb.counters_dict(full["totals"])["instances"] == COUNT


# ---- count == 0 -----------------------------------------------------------------------------
def test_count_zero_touches_nothing(gpu_lib):
    lib, c = gpu_lib, cfg_c()
    out = guard((64,), np.uint64)

    def untouched():
        return (out.view(np.uint8) == GUARD).all()
    o = ptr(out)
    assert lib.pxb_schedule_extract(C.byref(c), None, 0, DEPTH, o) == 0 and untouched()
    assert lib.pxb_run_scripted(C.byref(c), None, 0, DEPTH, o, o, o, o, o) == 0 and untouched()
    assert lib.pxb_shrink_batch(C.byref(c), None, None, 0, DEPTH, 0xFF, 64, o, o, o, o, o, o) == 0 and untouched()
    for fn, head in ((lib.pxb_trace_batch, (C.byref(c), None, 0)), (lib.pxb_trace_scripted, (C.byref(c), None, 0, DEPTH)),
                     (lib.pxb_trace_events, (C.byref(c), None, 0, DEPTH))):
        offs, n = guard((2,), np.uint64), guard((1,), np.uint64)
        assert fn(*head, None, o, 8, ptr(offs), o, o, ptr(n)) == 0 and untouched()
        assert offs[0] == 0 and n[0] == 0 and (offs[1:].view(np.uint8) == GUARD).all()
        assert fn(*head, None, None, 0, ptr(offs), None, None, None) == 0
    space, n = pxb.pxb_explore_space(1, 1, 0xFF, 0), guard((1,), np.uint64)
    assert lib.pxb_explore(C.byref(c), None, 0, DEPTH, C.byref(space), o, 8, ptr(n), o, o) == 0 and untouched()
    assert n[0] == 0
    tot = guard((pxb.NCOUNTERS,), np.int64)
    assert lib.pxb_run(C.byref(CFG.to_c(0, 0)), o, o, o, ptr(tot)) == 0 and untouched()
    assert (tot == 0).all()
    offs, n = guard((2,), np.uint64), guard((1,), np.uint64)
    assert lib.pxb_wire_encode_host(None, 0, pxb.WIRE_REQUEST, None, ptr(offs), ptr(n)) == 0
    assert offs[0] == 0 and n[0] == 0 and (offs[1:].view(np.uint8) == GUARD).all()
    assert lib.pxb_wire_decode_host(None, 0, ptr(offs), 0, pxb.WIRE_REQUEST, None, o) == 0 and untouched()
    assert lib.pxb_acceptor_handle(o, o, o, 0) == 0 and lib.pxb_proposer_handle(o, N, o, o, o, 0) == 0 and untouched()


# ---- pxb_explore's chunks -------------------------------------------------------------------
def test_explore_chunks(gpu_lib):
    cfg = pxb.Config(seed=0xE1, n_proposers=1, n_acceptors=3, loss_ppm=100000, delay_max=2, step_cap=256)
    ids = np.arange(4, dtype=np.uint64)
    rows = guard((4, pxb.script_stride(cfg, 8)), np.uint8)
    assert gpu_lib.pxb_schedule_extract(C.byref(cfg_c(cfg)), ptr(ids), 4, 8, ptr(rows)) == 0
    T = pxb.explore_total(cfg, 2, 2)
    assert T == 1 + 12 * 2 + 66 * 4
    space = pxb.pxb_explore_space(2, 2, 0xFF, 0)
    spec = {"ids": ((4 * T,), np.uint64), "n_matches": ((1,), np.uint64), "counts": ((4, 4, 3), np.uint32),
            "status": ((4,), np.uint32)}

    def run():
        b = {k: guard(*v) for k, v in spec.items()}
        assert explore_call(gpu_lib, cfg, rows, 8, space, 4 * T, b) == 0
        return b
    whole = run()
    assert whole["counts"][:, :, 0].sum() > 4               # (candidates ran, not only the parents)
    old = os.environ.get("PXB_EXPLORE_CHUNK")
    os.environ["PXB_EXPLORE_CHUNK"] = str(T - 1)            # less than one parent: a parent a chunk
    gpu_lib.pxb_reload_hooks()
    try:
        parts = run()
    finally:
        if old is None:
            del os.environ["PXB_EXPLORE_CHUNK"]
        else:
            os.environ["PXB_EXPLORE_CHUNK"] = old
        gpu_lib.pxb_reload_hooks()
    for k in spec:
        assert parts[k].tobytes() == whole[k].tobytes(), k


# ---- the wire host forms --------------------------------------------------------------------
def wire_msgs(kind):
    rng = np.random.default_rng(7 + kind)
    tag = rng.integers(0, 3, COUNT)
    x = rng.integers(-5, 1 << 14, COUNT)
    code = (rng.integers(1, 256, COUNT) << 24) | rng.integers(1, 1 << 24, COUNT)
    m = np.zeros((COUNT, 4), np.int64)
    m[:, 0] = tag
    if kind == pxb.WIRE_REQUEST:
        m[:, 1], m[:, 3] = x, np.where(tag == pxb.Propose, code, 0)
    else:
        has = (tag == pxb.Round1OK) & (rng.random(COUNT) < 0.6)
        m[:, 1] = np.where(tag == pxb.Round2Success, 0, x)
        m[:, 2], m[:, 3] = np.where(has, rng.integers(0, 1 << 14, COUNT), 0), np.where(has, code, 0)
    return m.astype(np.uint32)


@pytest.mark.parametrize("kind", [pxb.WIRE_REQUEST, pxb.WIRE_RESPONSE])
def test_wire_host_round_trip(gpu_lib, kind):
    msgs = wire_msgs(kind)
    data, offs, nb = guard((COUNT * pxb.WIRE_MAX_BYTES,), np.uint8), guard((COUNT + 1,), np.uint64), guard((1,), np.uint64)
    assert gpu_lib.pxb_wire_encode_host(ptr(msgs), COUNT, kind, ptr(data), ptr(offs), ptr(nb)) == 0
    n = int(nb[0])
    assert offs[0] == 0 and offs[COUNT] == n and (np.diff(offs.astype(np.int64)) > 0).all()
    assert COUNT <= n <= len(data) and (data[n:] == GUARD).all()
    back, status = guard((COUNT, 4), np.uint32), guard((COUNT,), np.uint32)
    assert gpu_lib.pxb_wire_decode_host(ptr(data), n, ptr(offs), COUNT, kind, ptr(back), ptr(status)) == 0
    assert (status == pxb.WIRE_OK).all() and np.array_equal(back, msgs)
    alone = guard((COUNT, 4), np.uint32)
    assert gpu_lib.pxb_wire_decode_host(ptr(data), n, ptr(offs), COUNT, kind, ptr(alone), None) == 0
    assert alone.tobytes() == back.tobytes()


# ---- the handler hooks ----------------------------------------------------------------------
def test_handler_hooks_match_the_oracle(gpu_lib):
    rng, n = np.random.default_rng(1), COUNT
    st = np.zeros((n, 4), np.uint32)
    st[:, 0] = rng.integers(0, 8, n)
    st[:, 1] = rng.integers(0, 8, n)
    st[:, 2] = np.where(rng.random(n) < 0.5, 0, (rng.integers(1, 4, n) << 24) | 1)
    st[:, 3] = rng.integers(0, 5, n) | (np.where(rng.random(n) < 0.1, 1, 0) << 31).astype(np.uint32)
    msg = np.zeros((n, 4), np.uint32)
    msg[:, 0] = rng.integers(0, 3, n)
    msg[:, 1] = rng.integers(0, 9, n)
    msg[:, 3] = (rng.integers(1, 4, n) << 24) | 1
    est, erep = oracle_c.acceptor_handle(st, msg)
    gst, grep = st.copy(), guard((n, 4), np.uint32)
    assert gpu_lib.pxb_acceptor_handle(ptr(gst), ptr(msg), ptr(grep), n) == 0
    assert np.array_equal(gst, est) and np.array_equal(grep, erep)

    ps = np.zeros((n, 10), np.uint32)
    ps[:, 0] = rng.integers(0, 8, n)                       # ticket
    ps[:, 1] = (rng.integers(1, 4, n) << 24) | 1           # cmd
    ps[:, 2] = rng.integers(0, 5, n)                       # acks
    ps[:, 3] = rng.integers(0, 3, n)                       # state
    ps[:, 4] = rng.integers(0, 8, n)                       # mr_t
    ps[:, 5] = np.where(rng.random(n) < 0.5, 0, (rng.integers(1, 4, n) << 24) | 1)
    ps[:, 6] = ps[:, 0]
    ps[:, 7] = (rng.integers(1, 4, n) << 24) | 1
    ps[:, 8] = rng.integers(0, 2, n)
    ps[:, 9] = rng.integers(1, 4, n)
    pm = np.zeros((n, 4), np.uint32)
    pm[:, 0] = rng.integers(0, 4, n)                       # 3 = Tick
    pm[:, 1] = rng.integers(0, 9, n)
    pm[:, 2] = rng.integers(0, 8, n)
    pm[:, 3] = np.where(rng.random(n) < 0.4, 0, (rng.integers(1, 4, n) << 24) | 1)
    for na in (2, 5, 9):
        est, ebc, enb = oracle_c.proposer_handle(ps, na, pm)
        gps, gbc, gnb = ps.copy(), np.zeros((n, 2, 4), np.uint32), np.zeros(n, np.uint32)
        assert gpu_lib.pxb_proposer_handle(ptr(gps), na, ptr(pm), ptr(gbc), ptr(gnb), n) == 0
        assert np.array_equal(gps, est) and np.array_equal(gbc, ebc) and np.array_equal(gnb, enb)
