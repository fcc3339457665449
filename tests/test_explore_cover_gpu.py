"""pxb_explore_cover on the GPU (docs/SEMANTICS.md §15): pxb.explore_cover and
pxb.explore_cover_device against the yardstick, every candidate materialised by
pxb.explore_rows and pushed through pxb.run_scripted and pxb.cover, with the
predicate, the subset rule and pxb.explore_reach_of in Python
(explore_cover_oracle.brute): ids, counts, reach records and status exactly
equal."""
import numpy as np
import pytest

import cover_oracle as CO
import explore_cover_oracle as XC
import explore_oracle as X
import pxb
from test_explore_gpu import UNIT_SHAPES

pytestmark = pytest.mark.gpu
GPU = dict(runner=pxb._run_scripted_runner, coverer=XC.gpu_coverer)
BIT = CO.BIT


def explore_cover_both(cfg, parents, depth, sd, R, query, mask):
    """pxb.explore_cover in both listing modes against the yardstick; the minimal-mode outputs."""
    want = XC.brute(cfg, parents, depth, sd, R, query, mask, **GPU)
    out = None
    for minimal in (False, True):
        out = pxb.explore_cover(cfg, parents, depth, sd, R, query, mask, minimal=minimal)
        XC.check(*out, want, minimal)
    return out


# ---- 1. the pinned shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_pinned_shapes(gpu_lib, name):
    """(a): T = 2,049, the first wave holds radii 0, 1 and 2 and the last one
    straddles the parent's end; (d): log mode."""
    cfg, row, depth, sd, R, T = X.shape(name)
    for q, mask in XC.QUERIES.values():
        ids, n, counts, reach, status = explore_cover_both(cfg, row, depth, sd, R, q, mask)
    import json
    kat = json.load(open(XC.KAT_PATH))["shapes"][name]
    r = pxb.explore_cover(cfg, row, depth, sd, R)[3][0]
    dist = pxb.reach_distance(r)
    assert pxb.cover_names(r.parent_mask) == kat["parent"]
    assert {n_: {"first": f, "count": c[:R + 1], "distance": dist[pxb.COVER_BIT[n_]]} for n_, (f, c) in r.by_name().items()} \
        == kat["classes"]


# ---- 2. five parents in one call -----------------------------------------------------------------------
def test_five_parents(gpu_lib):
    """Shape (a): parent boundaries inside waves; the bad parent's neighbours are
    unaffected and the repeated parent gives an equal record."""
    cfg, parents, depth, sd, R, T = XC.five_parents()
    q, mask = XC.QUERIES["cover"]
    ids, n, counts, reach, status = explore_cover_both(cfg, parents, depth, sd, R, q, mask)
    assert list(status) == [0, pxb.SCRIPT_BAD, 0, 0, 0] and not counts[1].any()
    assert reach[1].union == 0 == reach[1].parent_mask and set(reach[1].first) == {pxb.REACH_NONE}
    assert not any(any(r) for r in reach[1].counts)
    assert reach[0] == reach[4] and reach[0] != reach[2] and (counts[0] == counts[4]).all()
    alone = pxb.explore_cover(cfg, parents[0], depth, sd, R, q, mask)
    assert alone[3][0] == reach[0] and (alone[2][0] == counts[0]).all()
    per = [ids[ids // np.uint64(T) == i] - np.uint64(i * T) for i in range(5)]
    assert len(per[0]) and np.array_equal(per[0], per[4]) and np.array_equal(per[0], alone[0]) and len(per[1]) == 0
    assert (np.diff(ids.astype(np.int64)) > 0).all()


def test_keep_sites_of_absent_proposers(gpu_lib):
    cfg, parents, depth, sd, R, T = XC.keep_parents()
    ids, n, counts, reach, status = explore_cover_both(cfg, parents, depth, sd, R, None, 0)
    sk = pxb.explore_skipped(cfg, parents, depth, sd, R, np.arange(5 * T)).reshape(5, T)
    assert list(status) == [0, 0, pxb.SCRIPT_BAD, 0, 0] and reach[0] == reach[4]
    assert (counts[:, :, 0].sum(axis=1) <= (~sk).sum(axis=1)).all() and not sk.reshape(-1)[ids.astype(np.int64)].any()


# ---- 3. the device form ------------------------------------------------------------------------------------
def device_call(cfg, parents, depth, sd, R, query, mask, minimal, capacity, first_parent=0, d_ids=None, d_n=None,
                stream=None, want_reach=True):
    import torch
    dev = torch.device("cuda:0")
    rows = pxb._script_rows(cfg, parents, depth)
    n = len(rows)
    d_rows = torch.from_numpy(rows.reshape(-1).copy()).to(dev)
    if d_n is None:
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    if d_ids is None and capacity:
        d_ids = torch.full((capacity + 8,), -7, dtype=torch.int64, device=dev)
    d_counts = torch.full((n, 4, 3), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    # (guard bytes behind the records: nothing past count records is touched)
    d_reach = torch.full((n * pxb.EXPLORE_REACH_BYTES + 64,), 0x5A, dtype=torch.uint8, device=dev) if want_reach else None
    pxb.explore_cover_device(cfg, d_rows, n, depth, sd, R, d_n, query=query, flag_mask=mask, d_ids=d_ids, capacity=capacity,
                             d_counts=d_counts, d_reach=d_reach, d_status=d_status, first_parent=first_parent,
                             minimal=minimal, stream=stream)
    return d_rows, d_ids, d_n, d_counts, d_reach, d_status


def records(d_reach, n):
    raw = d_reach.cpu().numpy()
    assert (raw[n * pxb.EXPLORE_REACH_BYTES:] == 0x5A).all()
    return raw[:n * pxb.EXPLORE_REACH_BYTES].view(pxb.reach_dtype())


def test_capacity_and_cursor(gpu_lib):
    import torch
    cfg, row, depth, sd, R, T = X.shape("a")
    q, mask = XC.QUERIES["cover"]
    want = XC.brute(cfg, row, depth, sd, R, q, mask, **GPU)
    held = want["held"].astype(np.int64)
    k = len(held)
    assert k > 100
    # capacity 0: sizes only
    _, d_ids, d_n, d_counts, d_reach, d_status = device_call(cfg, row, depth, sd, R, q, mask, False, 0)
    torch.cuda.synchronize()
    assert d_ids is None and int(d_n.item()) == k
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), want["counts"]) and int(d_status.item()) == 0
    assert records(d_reach, 1).tobytes() == want["reach"].tobytes()
    # a capacity below the matches: the first 100, the guard values past them untouched; no reach records asked for
    _, d_ids, d_n, _, _, _ = device_call(cfg, row, depth, sd, R, q, mask, False, 100, want_reach=False)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == k and np.array_equal(got[:100], held[:100]) and (got[100:] == -7).all()
    # two calls, first_parent 0 and 1, append to one list
    d_ids = torch.full((2 * k + 16,), -7, dtype=torch.int64, device="cuda:0")
    _, _, d_n, _, _, _ = device_call(cfg, row, depth, sd, R, q, mask, False, 2 * k + 16, d_ids=d_ids)
    device_call(cfg, row, depth, sd, R, q, mask, False, 2 * k + 16, first_parent=1, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == 2 * k and np.array_equal(got[:2 * k], np.concatenate([held, held + T])) and (got[2 * k:] == -7).all()
    # a cursor already past the capacity: counted, nothing written
    d_ids.fill_(-7)
    d_n.fill_(5)
    m = len(want["minimal"])
    device_call(cfg, row, depth, sd, R, q, mask, True, 4, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == 5 + m and (d_ids.cpu().numpy() == -7).all()
    # count == 0
    d_rows = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    pxb.explore_cover_device(cfg, d_rows, 0, depth, sd, R, d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == 5 + m
    assert pxb.explore_cover(cfg, np.zeros((0, len(row)), np.uint8), depth, sd, R)[1] == 0


def test_ids_past_2_32(gpu_lib):
    """first_parent = 250,000 with shape (b): every g is past 2^32; the records'
    `first` stay candidates c < T."""
    import torch
    cfg, row, depth, sd, R, T = X.shape("b")
    q = pxb.CoverQuery(all_mask=BIT["R2S_REPEAT"])
    want = XC.brute(cfg, row, depth, sd, R, q, 0, **GPU)
    _, d_ids, d_n, _, d_reach, _ = device_call(cfg, row, depth, sd, R, q, 0, True, 8, first_parent=250000)
    torch.cuda.synchronize()
    k = len(want["minimal"])
    assert 250000 * T > 1 << 32 and 0 < k <= 8
    assert int(d_n.item()) == k and list(d_ids.cpu().numpy()[:k + 1]) == [250000 * T + int(c) for c in want["minimal"]] + [-7]
    assert records(d_reach, 1).tobytes() == want["reach"].tobytes()


def test_device_form_beside_a_run(gpu_lib):
    """explore_cover_device on one stream while pxb_run_device runs on another:
    both give what they give alone."""
    import torch
    cfg, row, depth, sd, R, T = X.shape("b")
    q, mask = XC.QUERIES["both"]
    want = XC.brute(cfg, row, depth, sd, R, q, mask, **GPU)
    c3, n3 = pxb.CONFIGS[3], 1 << 16
    dev = torch.device("cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_res = torch.zeros((n3, 4), dtype=torch.int32, device=dev)
    d_tot = torch.zeros(pxb.NCOUNTERS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    pxb.run_device(c3, 0, n3, d_results=d_res, d_totals=d_tot, stream=s2.cuda_stream)
    keep = device_call(cfg, row, depth, sd, R, q, mask, True, 2000, stream=s1.cuda_stream)
    pxb.run_device(c3, n3, n3, d_results=d_res, d_totals=d_tot, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _, d_ids, d_n, d_counts, d_reach, d_status = keep
    n = int(d_n.item())
    assert 0 < n <= 2000
    XC.check(d_ids.cpu().numpy()[:n].astype(np.uint64), n, d_counts.cpu().numpy().view(np.uint32), records(d_reach, 1),
             d_status.cpu().numpy().view(np.uint32), want, True)
    res2 = pxb.run(c3, n3, n3, want_digests=False)[0]
    assert np.array_equal(d_res.cpu().numpy().view(np.uint32), res2)
    pxb.stream_release(0, s2.cuda_stream)


# ---- 4. host-form chunking ----------------------------------------------------------------------------------
def test_host_form_chunks(gpu_lib):
    """PXB_EXPLORE_CHUNK = 5000 with the five parents of shape (a) (T = 2,049):
    two parents a chunk, three chunks; 1: a parent a chunk.  Every output equals
    the one-chunk call's."""
    cfg, parents, depth, sd, R, T = XC.five_parents()
    q, mask = XC.QUERIES["both"]
    whole = pxb.explore_cover(cfg, parents, depth, sd, R, q, mask, minimal=False)
    assert whole[1] > 50 and whole[0][-1] >= 4 * T
    for chunk in (5000, 1):
        with pxb.hooks(PXB_EXPLORE_CHUNK=chunk):
            got = pxb.explore_cover(cfg, parents, depth, sd, R, q, mask, minimal=False)
            part = pxb.explore_cover(cfg, parents, depth, sd, R, q, mask, minimal=False, capacity=50)
        assert got[1] == whole[1] and got[3] == whole[3]
        assert all(np.array_equal(a, b) for a, b in zip((got[0], got[2], got[4]), (whole[0], whole[2], whole[4])))
        assert part[1] == whole[1] and np.array_equal(part[0], whole[0][:50]) and part[3] == whole[3]


# ---- 5. every kernel unit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,delay_max", UNIT_SHAPES)
def test_every_kernel_unit(gpu_lib, P, N, delay_max):
    """test_explore_gpu's shapes (every proposer-count unit with the smallest and
    the largest acceptor count, and the 16-step wheel) at radius 1, site_depth 1,
    deep enough that candidates run OK: ids in both modes, counts, reach and status equal
    the host build's (tests/native/explore_cover_host.cpp) exactly."""
    cfg, parents, depth, sd, R = XC.unit_case(P, N, delay_max)
    q = pxb.CoverQuery(any_mask=BIT["PROPOSE_NACK"] | BIT["HAVE_BELOW"] | BIT["DISCARD_DEAD"] | BIT["R1OK_STALE"] |
                       BIT["ASK_NACK"] | BIT["DISCARD_ISOLATED"])
    for minimal in (False, True):
        h = XC.host_explore_cover(cfg, parents, depth, sd, R, q, 0, minimal=minimal)
        ids, n, counts, reach, status = pxb.explore_cover(cfg, parents, depth, sd, R, q, 0, minimal=minimal)
        assert n == h["n"] and np.array_equal(ids, h["ids"])
        assert np.array_equal(counts, h["counts"]) and np.array_equal(status, h["status"])
        assert XC.reach_records(reach).tobytes() == h["reach"].tobytes()
    assert (status == pxb.TRACE_OK).all() and reach[0].union != 0 and reach[1].union != 0 and n > 0


# ---- 6. the ties to pxb.explore and pxb.cover ---------------------------------------------------------------------
@pytest.mark.parametrize("mask", [X.PANIC, 0xFE])
def test_flag_only_predicate_equals_explore(gpu_lib, mask):
    cfg, row, depth, sd, R, T = X.shape("b")
    for minimal in (False, True):
        e = pxb.explore(cfg, row, depth, sd, R, mask, minimal=minimal)
        c = pxb.explore_cover(cfg, row, depth, sd, R, None, mask, minimal=minimal)
        assert e[1] == c[1] > 0 and np.array_equal(e[0], c[0]) and np.array_equal(e[2], c[2]) and np.array_equal(e[3], c[4])


def test_round_trip_through_cover(gpu_lib):
    """pxb.cover of the materialised rows of a listed set has the queried bits in
    every row, and the witness of a class has it."""
    cfg, row, depth, sd, R, T = X.shape("b")
    q = pxb.CoverQuery(all_mask=BIT["Q1_FOREIGN_ACCEPT"] | BIT["HAVE_ABORT_R2"], none_mask=BIT["EXEC_PANIC"])
    ids, n, _, reach, _ = pxb.explore_cover(cfg, row, depth, sd, R, q, minimal=False)
    assert n == len(ids) > 0
    masks, status, _, _ = pxb.cover(cfg, pxb.explore_rows(cfg, row, depth, sd, R, ids), depth)
    assert (status == pxb.TRACE_OK).all() and all(q.matches(int(m)) for m in masks)
    firsts = [(b, f) for b, f in enumerate(reach[0].first) if f != pxb.REACH_NONE]
    masks, _, _, _ = pxb.cover(cfg, pxb.explore_rows(cfg, row, depth, sd, R, [f for _, f in firsts]), depth)
    assert all((int(m) >> b) & 1 for (b, _), m in zip(firsts, masks))
