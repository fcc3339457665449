"""pxb_trace_batch on the GPU: many instances traced in one launch give, id by
id, exactly what pxb_trace_instance gives one call at a time, in the order of
the id list, with the window / tail selection and the capacity rule applied."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ev_matrix as M
import pxb
from test_trace_batch_host import SELECTIONS, U32, check_against_oracle, select

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A


def single(cfg, inst, production=False, max_records=4200):
    """pxb_trace_instance's raw rows and result (None, None where it returns PXB_E_INVAL)."""
    lib = pxb.load()
    buf = np.zeros((max_records, pxb.TRACE_WORDS), dtype=np.uint32)
    n = C.c_uint32(0)
    res = np.zeros(4, dtype=np.uint32)
    c = cfg.to_c(inst, 1)
    if production:
        c.flags |= pxb.CFG_TRACE_PRODUCTION
    rc = lib.pxb_trace_instance(C.byref(c), inst, C.c_void_p(buf.ctypes.data), max_records, C.byref(n),
                                C.c_void_p(res.ctypes.data))
    if rc == pxb.PXB_E_INVAL:
        return None, None
    assert rc == pxb.PXB_OK
    return buf[:n.value].copy(), res


def runs(rec, offs):
    return [rec[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


@pytest.mark.parametrize("production", [False, True])
@pytest.mark.parametrize("c", [3, 4, 5, 7, "3-wheel16"])
def test_equals_the_single_trace(gpu_lib, c, production):
    """ids 0..129 (two full waves and a two-lane third; config 5: 0..255, which
    hold instances beyond the link capacities; config 3 with delays up to 12,
    the 16-step wheel: 0..63): every instance's records and result are
    pxb_trace_instance's, byte for byte, and it is BAILED exactly where
    pxb_trace_instance refuses."""
    cfg = dataclasses.replace(pxb.CONFIGS[3], delay_max=12) if c == "3-wheel16" else pxb.CONFIGS[c]
    ids = np.arange({5: 256, "3-wheel16": 64}.get(c, 130), dtype=np.uint64)
    rec, offs, status, res = pxb.trace_batch(cfg, ids, production=production)
    assert offs[0] == 0 and offs[-1] == len(rec) and (np.diff(offs.astype(np.int64)) >= 0).all()
    got = runs(rec, offs)
    for i, inst in enumerate(ids):
        rows, r = single(cfg, int(inst), production)
        if rows is None:
            assert status[i] == pxb.TRACE_BAILED and len(got[i]) == 0 and not res[i].any(), inst
        else:
            assert status[i] == pxb.TRACE_OK, inst
            assert np.array_equal(got[i], rows), inst
            assert np.array_equal(res[i], r), inst
    nb = int((status == pxb.TRACE_BAILED).sum())
    assert nb <= 0.02 * len(ids)
    if c == 5:
        assert nb >= 1 and (status == pxb.TRACE_OK).any()
    # the decoded form is trace_instance's
    k = int(np.flatnonzero(status == pxb.TRACE_OK)[0])
    d, r = pxb.trace_instance(cfg, k, production=production)
    mine = pxb.trace_records(got[k])
    assert len(mine) == len(d) > 0
    for a, b in zip(mine, d):
        assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)


def test_against_the_oracle_directly(gpu_lib):
    """24 ids of config 4 from 2^32 - 40 .. 2^32 + 40, in descending order with
    one repeated: every record equals the reference model's end-of-step state
    (test_trace_matches_oracle_steps' rules); the repeated id's two runs are
    identical."""
    cfg = pxb.CONFIGS[4]
    pick = np.sort(np.random.default_rng(0x7B4).choice(81, 23, replace=False))
    ids = [(1 << 32) - 40 + int(k) for k in pick][::-1]
    ids.insert(9, ids[2])
    assert len(ids) == 24 and min(ids) < (1 << 32) < max(ids)
    rec, offs, status, res = pxb.trace_batch(cfg, ids)
    got = runs(rec, offs)
    assert (status == pxb.TRACE_OK).all()
    for i, inst in enumerate(ids):
        check_against_oracle(pxb.trace_records(got[i]), res[i], cfg, inst)
    assert len(got[2]) and np.array_equal(got[2], got[9]) and np.array_equal(res[2], res[9])


def test_results_equal_the_batch_run(gpu_lib):
    cfg = pxb.CONFIGS[4]
    n = 4096
    _, offs, status, res = pxb.trace_batch(cfg, np.arange(n, dtype=np.uint64), capacity=0)
    want = pxb.run(cfg, 0, n, want_digests=False)[0]
    assert (status == pxb.TRACE_OK).all()
    assert np.array_equal(res, want)
    # the count of every instance's records: at least its last step, at most its steps
    cnt = np.diff(offs.astype(np.int64))
    assert (cnt >= 1).all() and (cnt <= (want[:, 3] >> 16)).all()


_full = {}


def full3():
    """config 3, ids 0..199, every record (computed once, read-only)."""
    if not _full:
        ids = np.arange(200, dtype=np.uint64)
        rec, offs, status, res = pxb.trace_batch(pxb.CONFIGS[3], ids)
        for a in (rec, offs, status, res):
            a.setflags(write=False)
        _full["v"] = (ids, rec, offs, status, res)
    return _full["v"]


@pytest.mark.parametrize("sel", SELECTIONS)
def test_window_and_tail(gpu_lib, sel):
    ids, frec, foffs, fstatus, fres = full3()
    rec, offs, status, res = pxb.trace_batch(pxb.CONFIGS[3], ids, step_min=sel[0], step_max=sel[1], tail=sel[2])
    assert np.array_equal(status, fstatus) and np.array_equal(res, fres)
    got, full = runs(rec, offs), runs(frec, foffs)
    assert offs[-1] == len(rec)
    for i in range(len(ids)):
        want = select(full[i], sel)
        assert len(got[i]) == len(want), i
        if want:
            assert np.array_equal(got[i], np.array(want)), i
    if sel == (7, 3, 0):
        assert offs[-1] == 0 and all(offs[i + 1] == offs[i] for i in range(len(ids)))
    if sel == (0, U32, 1):
        ok = fstatus == pxb.TRACE_OK
        assert all(len(g) == 1 for g, k in zip(got, ok) if k)
        assert all(int(g[0][0]) == (int(r[3]) >> 16) - 1 for g, r, k in zip(got, fres, ok) if k)


def device_call(cfg, ids, capacity, pad=0, records=True, stream=None, **sel):
    import torch
    dev = torch.device("cuda:0")
    n = len(ids)
    d_ids = torch.tensor(np.asarray(ids, dtype=np.int64), device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    d_res = torch.full((max(n, 1), 4), -1, dtype=torch.int32, device=dev)
    d_rec = torch.full((capacity + pad, pxb.TRACE_WORDS), SENT, dtype=torch.int32, device=dev) if records else None
    pxb.trace_batch_device(cfg, d_ids if n else None, n, d_off, d_rec, capacity if records else 0, d_st, d_res,
                           stream=stream, **sel)
    return d_rec, d_off, d_st, d_res


def host(t):
    import torch
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint64)


def test_capacity_bounds_the_records_not_the_offsets(gpu_lib):
    import torch
    ids, frec, foffs, fstatus, fres = full3()
    total = int(foffs[-1])
    capacity = total // 2
    if capacity in set(int(x) for x in foffs):
        capacity += 1
    assert capacity not in set(int(x) for x in foffs)       # an instance is cut in the middle
    d_rec, d_off, d_st, d_res = device_call(pxb.CONFIGS[3], ids, capacity, pad=64)
    torch.cuda.synchronize()
    rec = host(d_rec)
    assert np.array_equal(host(d_off), foffs)
    assert np.array_equal(rec[:capacity], frec[:capacity])
    assert (rec[capacity:] == SENT).all()
    assert np.array_equal(host(d_st)[:len(ids)], fstatus) and np.array_equal(host(d_res), fres)
    # the sizing call: no record buffer at all, the same offsets
    _, d_off0, d_st0, d_res0 = device_call(pxb.CONFIGS[3], ids, 0, records=False)
    torch.cuda.synchronize()
    assert np.array_equal(host(d_off0), foffs) and np.array_equal(host(d_res0), fres)
    # ... and the host form allocates and returns min(total, capacity) records
    r, o, _, _ = pxb.trace_batch(pxb.CONFIGS[3], ids, capacity=capacity)
    assert len(r) == capacity and np.array_equal(r, frec[:capacity]) and np.array_equal(o, foffs)


@pytest.mark.parametrize("count", [0, 1, 64, 65])
def test_edge_counts(gpu_lib, count):
    import torch
    ids, frec, foffs, fstatus, fres = full3()
    rec, offs, status, res = pxb.trace_batch(pxb.CONFIGS[3], ids[:count])
    assert len(offs) == count + 1 and np.array_equal(offs, foffs[:count + 1])
    assert np.array_equal(rec, frec[:int(foffs[count])])
    assert np.array_equal(status, fstatus[:count]) and np.array_equal(res, fres[:count])
    d_rec, d_off, d_st, d_res = device_call(pxb.CONFIGS[3], ids[:count], 4096, pad=8)
    torch.cuda.synchronize()
    assert np.array_equal(host(d_off), foffs[:count + 1])
    k = min(int(foffs[count]), 4096)
    assert np.array_equal(host(d_rec)[:k], frec[:k]) and (host(d_rec)[k:] == SENT).all()
    if count == 0:
        assert (host(d_st) == U32).all() and (host(d_res) == U32).all()      # untouched


def test_two_streams_at_once(gpu_lib):
    import torch
    ids, frec, foffs, fstatus, fres = full3()
    cfg = pxb.CONFIGS[3]
    sels = [dict(step_min=10, step_max=40, tail=0), dict(step_min=0, step_max=U32, tail=2)]
    serial = []
    for s in sels:
        out = device_call(cfg, ids, 8192, **s)
        torch.cuda.synchronize()
        serial.append([host(t).copy() for t in out])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    both = []
    for s, st in zip(sels, streams):
        with torch.cuda.stream(st):            # (the buffers are filled on the stream the call runs on)
            both.append(device_call(cfg, ids, 8192, stream=st.cuda_stream, **s))
    torch.cuda.synchronize()
    for want, out in zip(serial, both):
        for w, t in zip(want, out):
            assert np.array_equal(w, host(t))
    assert not np.array_equal(serial[0][1], serial[1][1])   # the two selections differ


def test_sweep_then_trace_batch(gpu_lib):
    """The workflow: sweep for the panics, trace the last two steps of each."""
    from test_query_gpu import SWEEP_FIRST, SWEEP_N
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY)
    ids, matched, n_matches, _, _, _ = pxb.sweep(pxb.CONFIGS[3], SWEEP_FIRST, SWEEP_N, q, 512)
    assert len(ids) == 512 <= n_matches
    rec, offs, status, res = pxb.trace_batch(pxb.CONFIGS[3], ids, tail=2)
    assert (status == pxb.TRACE_OK).all()
    assert (res[:, 3] & pxb.F_PANIC).all() and np.array_equal(res, matched)
    for i, g in enumerate(runs(rec, offs)):
        assert 1 <= len(g) <= 2, i
        last = pxb.trace_records(g[-1:])[0]
        assert (last["acc"][:, 3] >> 31).any(), int(ids[i])
        assert last["step"] == (int(res[i][3]) >> 16) - 1


@pytest.mark.parametrize("production", [False, True])
def test_capped_instance_records_its_last_visited_step(gpu_lib, production):
    """Config 3, id 33 ends at the step cap from step 253 (its next message falls
    due past the cap): the single and the batched trace both record 253 and,
    last, 255 (the default variant with the same state, and its records are the
    oracle's step by step)."""
    cfg = pxb.CONFIGS[3]
    rows, r = single(cfg, 33, production)
    rec, offs, status, res = pxb.trace_batch(cfg, [33], production=production)
    assert status[0] == pxb.TRACE_OK and np.array_equal(rec, rows) and np.array_equal(res[0], r)
    assert int(r[3]) & pxb.F_STEP_CAP
    steps = [int(x[0]) for x in rec]
    assert steps[-1] == 255 and 253 in steps and steps == sorted(set(steps))
    if not production:
        assert steps[-2:] == [253, 255] and np.array_equal(rec[-2][1:], rec[-1][1:])
        check_against_oracle(pxb.trace_records(rec), r, cfg, 33)
    tail = pxb.trace_batch(cfg, [33], tail=1, production=production)[0]
    assert len(tail) == 1 and np.array_equal(tail[0], rec[-1])


@pytest.mark.parametrize("P,N,mode", M.LANE_SHAPES, ids=M.LANE_SHAPE_IDS)
def test_every_shape_equals_the_oracle(gpu_lib, P, N, mode):
    """Every shape of the family (csrc/lane_shapes.h: P in 1..3, N in 2..9, both
    wheels and log mode) on the lossy schedule of tests/ev_matrix.py: 128
    consecutive ids, their last record each.  The result of every id that ends
    OK is the oracle's, at least 7/8 of the ids do, and an OK id's one record is
    its last step's."""
    cfg = M.lane_cfg(P, N, mode)
    eres = M.lane_oracle(P, N, mode)[0]
    rec, offs, status, res = pxb.trace_batch(cfg, M.LANE_IDS, tail=1)
    ok = status == pxb.TRACE_OK
    assert int((~ok).sum()) <= M.LANE_CAP
    assert np.array_equal(res[ok], eres[ok])
    assert offs[-1] == len(rec) and (np.diff(offs.astype(np.int64))[ok] == 1).all()
    assert np.array_equal(rec[offs[:-1][ok].astype(np.int64), 0], (eres[ok][:, 3] >> 16) - 1)
