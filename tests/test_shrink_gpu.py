"""The batched shrinker (docs/SEMANTICS.md §11) on the GPU: pxb.shrink_batch
against pxb.shrink with its default (GPU) runner, instance by instance and bit
for bit; 1-minimality and replay of what it returns; every kernel unit; the
device form; the edges."""
import dataclasses

import numpy as np
import pytest

import pxb
import shrink_oracle as H

pytestmark = pytest.mark.gpu
DEPTH = 64
OTHER_SEED = 0x0123456789ABCDEF
_c3 = {}


def compare(cfg, ids, mask, depth=DEPTH, **kw):
    """shrink_batch over ids equals one pxb.shrink per id; returns (rows given, outputs, references)."""
    rows = pxb.extract_schedule(cfg, ids, depth)
    o = H.as_dict(pxb.shrink_batch(cfg, ids, mask, depth=depth, **kw))
    rr = [H.reference(cfg, rows[i], mask, depth=depth) for i in range(len(ids))]
    for i, ref in enumerate(rr):
        H.check(cfg, o, i, ref, depth)
    return rows, o, rr


def config3():
    """Test 1's sweep, batch and references, computed once."""
    if not _c3:
        cfg = pxb.CONFIGS[3]
        ids, _, n, _, _, _ = pxb.sweep(cfg, 0, 4096, pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY), 64)
        ids = np.sort(np.asarray(ids[:min(int(n), 64)], dtype=np.uint64))
        _c3["v"] = (cfg, ids) + compare(cfg, ids, pxb.F_PANIC)
    return _c3["v"]


def test_config3_sweep_matches(gpu_lib):
    """The first 64 PANIC ids of a sweep over 0..4095: rows, faults, launches and
    status equal 64 pxb.shrink calls; a match pxb.shrink refuses is NOT_INPUT."""
    cfg, ids, rows, o, rr = config3()
    assert len(ids) == 64
    assert sum(r["status"] == pxb.SHRINK_MINIMAL for r in rr) >= 32
    for i, r in enumerate(rr):
        if r["status"] == pxb.SHRINK_NOT_INPUT:
            assert (o["rows"][i] == rows[i]).all() and o["launches"][i] == 1


@pytest.mark.parametrize("c, n, mask", [(5, 32, 0x3E), (7, 16, pxb.F_PANIC)])
def test_configs_5_and_7(gpu_lib, c, n, mask):
    _, _, rr = compare(pxb.CONFIGS[c], np.arange(n, dtype=np.uint64), mask)
    assert any(r["status"] == pxb.SHRINK_MINIMAL for r in rr)


def test_minimal_and_replays(gpu_lib):
    """Test 1's outputs re-checked in two run_scripted launches: every returned
    row holds the predicate with the reported sent and result, every single
    neutralisation of it loses the predicate, and the row moved to another seed
    and base gives the same result and sent."""
    cfg, ids, _, o, _ = config3()
    keep = [i for i in range(len(ids)) if o["status"][i] == pxb.SHRINK_MINIMAL]
    cand, owner = [], []
    for i in keep:
        for f in pxb.script_faults(cfg, o["rows"][i], DEPTH, o["sent"][i]):
            r = o["rows"][i].copy()
            pxb.script_neutralise(cfg, r, DEPTH, f)
            cand.append(r)
            owner.append(i)
    assert len(cand) == int(o["n_faults"][keep].sum()) > 0
    res, _, _, status, sent = pxb.run_scripted(cfg, np.array(cand), DEPTH, want_digests=False)
    held = (status == pxb.TRACE_OK) & ((res[:, 3] & 0xFF & pxb.F_PANIC) != 0) & (sent.reshape(len(cand), -1).max(1) <= DEPTH)
    assert not held.any(), [owner[j] for j in np.nonzero(held)[0]]
    moved = o["rows"][keep].copy()
    pxb.script_base(moved)[:] = 987654321012 + np.arange(len(keep), dtype=np.uint64)
    both = np.concatenate([o["rows"][keep], moved])
    res, _, _, status, sent = pxb.run_scripted(cfg, both[:len(keep)], DEPTH, want_digests=False)
    res2, _, _, status2, sent2 = pxb.run_scripted(dataclasses.replace(cfg, seed=OTHER_SEED), both[len(keep):], DEPTH,
                                                  want_digests=False)
    assert (status == pxb.TRACE_OK).all() and ((res[:, 3] & pxb.F_PANIC) != 0).all()
    assert (res == o["res"][keep]).all() and (sent == o["sent"][keep]).all()
    assert (status2 == status).all() and (res2 == res).all() and (sent2 == sent).all()


# (P, N, delay_max, depth): every proposer-count unit with the smallest and the
# largest acceptor count on the 8-step wheel, and one shape on the 16-step wheel
UNIT_SHAPES = [pytest.param(p, n, 4, 32, id="%d-%d" % (n, p)) for n in (2, 9) for p in (1, 2, 3)] + [
    pytest.param(2, 3, 12, 12, id="3-2-wheel16")]


@pytest.mark.parametrize("P,N,delay_max,depth", UNIT_SHAPES)
def test_every_kernel_unit(gpu_lib, P, N, delay_max, depth):
    """Every proposer-count unit, the smallest and the largest acceptor count; both wheels."""
    cfg = pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                     delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                     step_cap=256)
    _, _, rr = compare(cfg, np.arange(64, dtype=np.uint64), 0x3F, depth=depth)
    assert sum(r["status"] != pxb.SHRINK_NOT_INPUT for r in rr) >= 1


def test_device_form(gpu_lib):
    """Rows extracted into a tensor and shrunk in place on a non-default stream
    equal the host form's; outputs passed as NULL are not written."""
    import torch
    cfg, ids, _, o, _ = config3()
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
        pxb.extract_schedule_device(cfg, d_ids, n, DEPTH, d_rows, stream=st.cuda_stream)
        pxb.shrink_batch_device(cfg, d_rows, n, DEPTH, pxb.F_PANIC, d_status=d_status, d_n_faults=d_nf,
                                d_launches=d_la, d_sent=d_sent, d_results=d_res, d_signature=d_sig,
                                stream=st.cuda_stream)
        st.synchronize()
        assert (d_rows.cpu().numpy().reshape(n, -1) == o["rows"]).all()
        for t, k, dt in ((d_status, "status", np.uint32), (d_nf, "n_faults", np.uint32), (d_la, "launches", np.uint32),
                         (d_sent, "sent", np.uint16), (d_res, "res", np.uint32), (d_sig, "sig", np.uint64)):
            assert (t.cpu().numpy().view(dt) == o[k]).all(), k
        # only the rows and the status this time: the other buffers keep what they hold
        pxb.extract_schedule_device(cfg, d_ids, n, DEPTH, d_rows, stream=st.cuda_stream)
        d_status.fill_(-7)
        d_nf.fill_(-7)
        pxb.shrink_batch_device(cfg, d_rows, n, DEPTH, pxb.F_PANIC, d_status=d_status, stream=st.cuda_stream)
        st.synchronize()
        assert (d_rows.cpu().numpy().reshape(n, -1) == o["rows"]).all()
        assert (d_status.cpu().numpy().view(np.uint32) == o["status"]).all() and (d_nf.cpu().numpy() == -7).all()


def test_edges(gpu_lib):
    """count == 0; one parent alone (config 3 id 10: 592 candidates over ten
    blocks, down to one message fault); chunk = 8 equals the single call."""
    cfg, ids, _, o, _ = config3()
    e = pxb.shrink_batch(cfg, np.zeros(0, np.uint64), pxb.F_PANIC)
    assert all(len(x) == 0 for x in e)
    import ctypes as C
    c = cfg.to_c(0, 1)
    assert pxb.load().pxb_shrink_batch_device(C.byref(c), None, 0, DEPTH, pxb.F_PANIC, 64, None, None, None, None, None,
                                              None, None) == pxb.PXB_OK
    _, one, rr = compare(cfg, np.array([10], dtype=np.uint64), pxb.F_PANIC)
    assert one["status"][0] == pxb.SHRINK_MINIMAL and one["n_faults"][0] == 1
    (kind, dirn, p, a, k), = rr[0]["faults"]
    assert kind == "link" and pxb.script_links(cfg, one["rows"], DEPTH)[0, dirn, p, a, k] != 1   # lost or delayed
    s = H.as_dict(pxb.shrink_batch(cfg, ids, pxb.F_PANIC, chunk=8))
    for k in o:
        assert (s[k] == o[k]).all(), k
