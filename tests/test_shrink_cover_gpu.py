"""The shrinker over a coverage predicate (docs/SEMANTICS.md §16) on the GPU:
pxb.shrink_cover_batch against pxb.shrink_cover with its default (GPU) runner,
instance by instance and bit for bit, masks included; against the existing
shrinker with the all-zero query; every kernel unit; 1-minimality and replay of
what it returns; the device form; the edges."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import cover_oracle as CO
import pxb
import shrink_cover_oracle as HC
import shrink_oracle as H
from test_shrink_gpu import UNIT_SHAPES

pytestmark = pytest.mark.gpu
DEPTH = 64
OTHER_SEED = 0x0123456789ABCDEF
Q = pxb.CoverQuery
B = CO.BIT
LOSSY = CO._LOSSY
Q1 = Q(all_mask=B["Q1_FOREIGN_ACCEPT"])
ANY_FAULTY = B["DISCARD_DEAD"] | B["DISCARD_ISOLATED"] | B["ASK_NACK"] | B["PROPOSE_NACK"]
_q1 = {}


def compare(cfg, ids, query, flag_mask=0, depth=DEPTH, **kw):
    """shrink_cover_batch over ids equals one pxb.shrink_cover per id; returns (rows given, outputs, references)."""
    rows = pxb.extract_schedule(cfg, ids, depth)
    o = HC.as_dict(pxb.shrink_cover_batch(cfg, ids, query, flag_mask, depth=depth, **kw))
    rr = [HC.reference(cfg, rows[i], query, flag_mask, depth=depth) for i in range(len(ids))]
    for i, ref in enumerate(rr):
        HC.check(cfg, o, i, ref, depth)
    return rows, o, rr


def lossy_q1():
    """Test 1's batch and references, computed once."""
    if not _q1:
        ids = np.arange(64, dtype=np.uint64)
        _q1["v"] = (ids,) + compare(LOSSY, ids, Q1)
    return _q1["v"]


def gpu_runner(cfg, rows, depth):
    return pxb._run_cover_runner(cfg, rows, depth)


def test_against_the_specification(gpu_lib):
    """Lossy P2 N3, ids 0..63, Q1: 19 inputs, launches 6..14, 18 signatures."""
    _, rows, o, rr = lossy_q1()
    inputs = [i for i, r in enumerate(rr) if r["status"] != pxb.SHRINK_NOT_INPUT]
    la = [int(o["launches"][i]) for i in inputs]
    print("inputs", inputs, "launches", la)
    assert len(inputs) == 19 and (min(la), max(la)) == (6, 14)
    assert len({int(o["sig"][i]) for i in inputs}) == 18
    for i in range(64):
        if i not in inputs:
            assert (o["rows"][i] == rows[i]).all() and o["launches"][i] == 1
    assert (o["masks"][inputs] & B["Q1_FOREIGN_ACCEPT"]).all()


def test_against_the_existing_shrinker(gpu_lib):
    """The first 64 PANIC ids of a sweep of config 3, all-zero query, F_PANIC:
    every output is pxb.shrink_batch's; the masks are pxb.cover of the returned rows."""
    cfg = pxb.CONFIGS[3]
    ids, _, n, _, _, _ = pxb.sweep(cfg, 0, 4096, pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY), 64)
    ids = np.sort(np.asarray(ids[:min(int(n), 64)], dtype=np.uint64))
    assert len(ids) == 64
    o = HC.as_dict(pxb.shrink_cover_batch(cfg, ids, None, pxb.F_PANIC))
    s = H.as_dict(pxb.shrink_batch(cfg, ids, pxb.F_PANIC))
    for k in s:
        assert (o[k] == s[k]).all(), k
    assert (o["status"] == pxb.SHRINK_MINIMAL).sum() >= 32
    assert (o["masks"] == pxb.cover(cfg, o["rows"], DEPTH)[0]).all()


@pytest.mark.parametrize("P,N,delay_max,depth", UNIT_SHAPES)
def test_every_kernel_unit(gpu_lib, P, N, delay_max, depth):
    """Every proposer-count unit, the smallest and the largest acceptor count, both
    wheels: the outcome flags and the query together."""
    cfg = pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                     delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                     step_cap=256)
    _, _, rr = compare(cfg, np.arange(64, dtype=np.uint64), Q(any_mask=ANY_FAULTY), 0x3F, depth=depth)
    assert sum(r["status"] != pxb.SHRINK_NOT_INPUT for r in rr) >= 1


def test_log_mode(gpu_lib):
    _, o, rr = compare(CO.CASES["log-p2n3"][0], np.arange(64, dtype=np.uint64),
                       Q(all_mask=B["TICK_BUSY"] | B["Q7_STALE_EXEC"]))
    assert [i for i, r in enumerate(rr) if r["status"] != pxb.SHRINK_NOT_INPUT] == [5, 14, 17, 21, 50, 54, 62]


def test_minimal_and_replays(gpu_lib):
    """Test 1's MINIMAL rows hold the predicate by run_scripted + cover, every
    single neutralisation loses it, and moved to another seed and base a row
    gives the same result, sent and mask."""
    _, _, o, _ = lossy_q1()
    keep = HC.one_minimal(LOSSY, o, Q1, 0, DEPTH, gpu_runner)
    moved = o["rows"][keep].copy()
    pxb.script_base(moved)[:] = 987654321012 + np.arange(len(keep), dtype=np.uint64)
    res, status, sent, masks = gpu_runner(dataclasses.replace(LOSSY, seed=OTHER_SEED), moved, DEPTH)
    assert (status == pxb.TRACE_OK).all() and (res == o["res"][keep]).all() and (sent == o["sent"][keep]).all()
    assert (masks == o["masks"][keep]).all()


def test_device_form(gpu_lib):
    """Rows extracted into a tensor and shrunk in place on a non-default stream
    equal the host form's; outputs passed as NULL are not written."""
    import torch
    ids, _, o, _ = lossy_q1()
    cfg = LOSSY
    n, P, N = len(ids), cfg.n_proposers, cfg.n_acceptors
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_ids = torch.from_numpy(ids.astype(np.int64)).to(dev)
        d_rows = torch.zeros(n * pxb.script_stride(cfg, DEPTH), dtype=torch.uint8, device=dev)
        d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_nf = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_la = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_sent = torch.full((n, 2, P, N), -7, dtype=torch.int16, device=dev)
        d_res = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
        d_sig = torch.full((n,), -7, dtype=torch.int64, device=dev)
        d_masks = torch.full((n,), -7, dtype=torch.int32, device=dev)
        pxb.extract_schedule_device(cfg, d_ids, n, DEPTH, d_rows, stream=st.cuda_stream)
        pxb.shrink_cover_batch_device(cfg, d_rows, n, DEPTH, Q1, d_status=d_status, d_n_faults=d_nf, d_launches=d_la,
                                      d_sent=d_sent, d_results=d_res, d_signature=d_sig, d_masks=d_masks,
                                      stream=st.cuda_stream)
        st.synchronize()
        assert (d_rows.cpu().numpy().reshape(n, -1) == o["rows"]).all()
        for t, k, dt in ((d_status, "status", np.uint32), (d_nf, "n_faults", np.uint32), (d_la, "launches", np.uint32),
                         (d_sent, "sent", np.uint16), (d_res, "res", np.uint32), (d_sig, "sig", np.uint64),
                         (d_masks, "masks", np.uint32)):
            assert (t.cpu().numpy().view(dt) == o[k]).all(), k
        # only the rows and the masks this time: the other buffers keep what they hold
        pxb.extract_schedule_device(cfg, d_ids, n, DEPTH, d_rows, stream=st.cuda_stream)
        d_masks.fill_(-7)
        d_status.fill_(-7)
        pxb.shrink_cover_batch_device(cfg, d_rows, n, DEPTH, Q1, d_masks=d_masks, stream=st.cuda_stream)
        st.synchronize()
        assert (d_rows.cpu().numpy().reshape(n, -1) == o["rows"]).all()
        assert (d_masks.cpu().numpy().view(np.uint32) == o["masks"]).all() and (d_status.cpu().numpy() == -7).all()


def test_edges(gpu_lib):
    """count == 0; chunk = 8 equals the single call; a batch with no input at all."""
    ids, rows, o, _ = lossy_q1()
    e = pxb.shrink_cover_batch(LOSSY, np.zeros(0, np.uint64), Q1)
    assert all(len(x) == 0 for x in e)
    c = LOSSY.to_c(0, 1)
    pr = HC.pred(Q1)
    assert pxb.load().pxb_shrink_cover_batch_device(C.byref(c), None, 0, DEPTH, C.byref(pr), None, None, None, None,
                                                    None, None, None, None) == pxb.PXB_OK
    s = HC.as_dict(pxb.shrink_cover_batch(LOSSY, ids, Q1, chunk=8))
    for k in o:
        assert (s[k] == o[k]).all(), k
    r = HC.as_dict(pxb.shrink_cover_batch(LOSSY, ids, Q(all_mask=B["R2S_REPEAT"])))
    assert (r["status"] == pxb.SHRINK_NOT_INPUT).all() and (r["rows"] == rows).all() and (r["launches"] == 1).all()
    assert not r["n_faults"].any() and not r["sent"].any() and not r["sig"].any()
    m, _, res, _ = pxb.cover(LOSSY, rows, DEPTH)
    assert (r["masks"] == m).all() and (r["res"] == res).all()
