"""The explorer on the GPU (docs/SEMANTICS.md §12): pxb.explore and
pxb.explore_device against the yardstick, pxb.run_scripted over pxb.explore_rows
of ALL T candidates of every parent with the predicate and the subset rule in
Python (explore_oracle.brute): the held set, the counts, the status and both
listings exactly equal, and the pinned numbers of the shapes (a), (b), (d)."""
import numpy as np
import pytest

import explore_oracle as X
import pxb
import script_oracle as SO

pytestmark = pytest.mark.gpu
GPU = pxb._run_scripted_runner


def explore_both(cfg, parents, depth, sd, R, mask):
    """pxb.explore in both listing modes against the yardstick; the minimal-mode outputs."""
    want = X.brute(cfg, parents, depth, sd, R, mask, runner=GPU)
    out = None
    for minimal in (False, True):
        ids, n, counts, status = pxb.explore(cfg, parents, depth, sd, R, mask, minimal=minimal)
        X.check(ids, n, counts, status, want, minimal)
        out = (ids, n, counts, status)
    return out


# ---- 1. the pinned shapes ----------------------------------------------------------------------------
def test_shape_a(gpu_lib):
    """T = 2,049 (not a multiple of 64: the last wave straddles the parent's end)."""
    cfg, row, depth, sd, R, T = X.shape("a")
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.PANIC)
    assert [int(x) for x in counts[0, :, 1]] == [0, 3, 45, 294] and list(ids) == [4, 8, 12] and counts[0, :, 0].sum() == T
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.STUCK)
    assert counts[0, :, 1].sum() == 598 and [int(x) for x in counts[0, :, 2]] == [0, 0, 36, 0] and list(ids[:3]) == [32, 36, 40]
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, 0xFE)
    assert counts[0, :, 1].sum() == 940 and [int(x) for x in counts[0, :, 2]] == [0, 3, 21, 0]


def test_shape_b(gpu_lib):
    cfg, row, depth, sd, R, T = X.shape("b")
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.PANIC)
    assert [int(x) for x in counts[0, :, 1]] == [0, 0, 3, 105] and list(ids) == [140, 208, 292]
    assert T - counts[0, :, 0].sum() == 2445
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.STUCK)
    assert counts[0, :, 1].sum() == 1526 and [int(x) for x in counts[0, :, 2]] == [0, 0, 36, 68]
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.LOG_DIV)
    assert [int(x) for x in counts[0, :, 1]] == [0, 0, 0, 36] == [int(x) for x in counts[0, :, 2]] and ids[0] == 1472
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, 0xFE)
    assert counts[0, :, 1].sum() == 1625 and counts[0, :, 2].sum() == 110


def test_shape_d_log_mode(gpu_lib):
    cfg, row, depth, sd, R, T = X.shape("d")
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.LOG_DIV)
    assert counts[0, :, 1].sum() == 74 and [int(x) for x in counts[0, :, 2]] == [0, 2, 12, 0] and list(ids[:2]) == [16, 22]
    ids, n, counts, _ = explore_both(cfg, row, depth, sd, R, X.PANIC)
    assert n == 0 and not counts[0, :, 1].any()


# ---- 2. five parents in one call -----------------------------------------------------------------------
def test_five_parents(gpu_lib):
    """The benign row, a failing explicit row (the minimal panic 140 of (b)), the
    benign row, a malformed row, the benign row: the duplicates give the same
    per-parent results shifted by T, the bad row lists nothing and has zero
    counts, and g ascends across the parents."""
    cfg, row, depth, sd, _, _ = X.shape("b")
    R = 2
    T = pxb.explore_total(cfg, sd, R)
    assert T == 1153
    failing = pxb.explore_rows(cfg, row, depth, sd, R, [140])[0]
    bad = row.copy()
    bad[9] = 1
    parents = np.stack([row, failing, row, bad, row])
    for mask in (X.PANIC, 0xFE):
        ids, n, counts, status = explore_both(cfg, parents, depth, sd, R, mask)
        assert list(status) == [0, 0, 0, pxb.SCRIPT_BAD, 0] and not counts[3].any()
        assert (counts[0] == counts[2]).all() and (counts[0] == counts[4]).all() and counts[1, 0, 1] == 1
        per = [ids[ids // np.uint64(T) == i] - np.uint64(i * T) for i in range(5)]
        assert len(per[0]) and np.array_equal(per[0], per[2]) and np.array_equal(per[0], per[4]) and len(per[3]) == 0
        assert list(per[1]) == [0]                     # the failing parent holds itself: nothing else is minimal
        assert (np.diff(ids.astype(np.int64)) > 0).all()


# ---- 3. keep sites ---------------------------------------------------------------------------------------
def test_keep_sites(gpu_lib):
    """Config 5 (P 3, N 9, delay_max 8, RANDOMIZE), extracted rows at depth 8,
    site_depth 1, R 2 (T = 92,017), of ids whose drawn P is 1, 2 and 3: the links
    of absent proposers are 0xFF, and a candidate that changes one is neither ran
    OK nor held; the rest equal run_scripted."""
    cfg, depth, sd, R = pxb.CONFIGS[5], 8, 1, 2
    T = pxb.explore_total(cfg, sd, R)
    assert T == 92017
    rows = pxb.extract_schedule(cfg, np.arange(64), depth)
    drawn = pxb.script_n_proposers(rows)
    parents = np.stack([rows[np.nonzero(drawn == p)[0][0]] for p in (1, 2, 3)])
    sk = pxb.explore_skipped(cfg, parents, depth, sd, R, np.arange(3 * T)).reshape(3, T)
    assert sk[0].any() and sk[1].any() and not sk[2].any() and sk[0].sum() > sk[1].sum()
    want = X.brute(cfg, parents, depth, sd, R, 0x3E, runner=GPU)
    assert not want["bytes"][sk].any()
    ids, n, counts, status = explore_both(cfg, parents, depth, sd, R, 0x3E)
    assert (counts[:, :, 0].sum(axis=1) <= (~sk).sum(axis=1)).all() and counts[:, :, 0].sum() > 0
    assert not sk.reshape(-1)[want["held"].astype(np.int64)].any()


# ---- 4, 5, 8. the device form ------------------------------------------------------------------------------
def device_call(cfg, parents, depth, sd, R, mask, minimal, capacity, first_parent=0, d_ids=None, d_n=None, stream=None,
                want_counts=True):
    import torch
    dev = torch.device("cuda:0")
    rows = pxb._script_rows(cfg, parents, depth)
    n = len(rows)
    d_rows = torch.from_numpy(rows.reshape(-1).copy()).to(dev)
    if d_n is None:
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    if d_ids is None and capacity:
        d_ids = torch.full((capacity + 8,), -7, dtype=torch.int64, device=dev)
    d_counts = torch.full((n, 4, 3), -7, dtype=torch.int32, device=dev) if want_counts else None
    d_status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    pxb.explore_device(cfg, d_rows, n, depth, sd, R, mask, d_n, d_ids=d_ids, capacity=capacity, d_counts=d_counts,
                       d_status=d_status, first_parent=first_parent, minimal=minimal, stream=stream)
    return d_rows, d_ids, d_n, d_counts, d_status


def test_capacity_and_cursor(gpu_lib):
    import torch
    cfg, row, depth, sd, R, T = X.shape("a")
    want = X.brute(cfg, row, depth, sd, R, X.PANIC, runner=GPU)
    held = want["held"].astype(np.int64)
    assert len(held) == 342
    # capacity 0: sizes only
    _, d_ids, d_n, d_counts, d_status = device_call(cfg, row, depth, sd, R, X.PANIC, False, 0)
    torch.cuda.synchronize()
    assert d_ids is None and int(d_n.item()) == 342
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), want["counts"]) and int(d_status.item()) == 0
    # a capacity below the matches: the first 100, the sentinels past them untouched
    _, d_ids, d_n, _, _ = device_call(cfg, row, depth, sd, R, X.PANIC, False, 100, want_counts=False)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == 342 and np.array_equal(got[:100], held[:100]) and (got[100:] == -7).all()
    # two calls, first_parent 0 and 1, append to one list
    d_ids = torch.full((700,), -7, dtype=torch.int64, device="cuda:0")
    _, _, d_n, _, _ = device_call(cfg, row, depth, sd, R, X.PANIC, False, 700, d_ids=d_ids)
    device_call(cfg, row, depth, sd, R, X.PANIC, False, 700, first_parent=1, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy()
    assert int(d_n.item()) == 684 and np.array_equal(got[:684], np.concatenate([held, held + T])) and (got[684:] == -7).all()
    # a cursor already past the capacity: counted, nothing written
    d_ids.fill_(-7)
    d_n.fill_(5)
    device_call(cfg, row, depth, sd, R, X.PANIC, True, 4, d_ids=d_ids, d_n=d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == 8 and (d_ids.cpu().numpy() == -7).all()
    # count == 0
    d_rows = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    pxb.explore_device(cfg, d_rows, 0, depth, sd, R, X.PANIC, d_n)
    torch.cuda.synchronize()
    assert int(d_n.item()) == 8
    assert pxb.explore(cfg, np.zeros((0, len(row)), np.uint8), depth, sd, R, X.PANIC)[1] == 0


def test_ids_past_2_32(gpu_lib):
    """first_parent = 250,000 with shape (b): every g is past 2^32."""
    import torch
    cfg, row, depth, sd, R, T = X.shape("b")
    _, d_ids, d_n, _, _ = device_call(cfg, row, depth, sd, R, X.PANIC, True, 8, first_parent=250000)
    torch.cuda.synchronize()
    assert 250000 * T > 1 << 32
    assert int(d_n.item()) == 3 and list(d_ids.cpu().numpy()[:4]) == [250000 * T + c for c in (140, 208, 292)] + [-7]


def test_device_form_beside_a_run(gpu_lib):
    """explore_device on one stream while pxb_run_device runs on another: both
    give what they give alone."""
    import torch
    cfg, row, depth, sd, R, T = X.shape("b")
    want = X.brute(cfg, row, depth, sd, R, X.STUCK, runner=GPU)
    c3, n3 = pxb.CONFIGS[3], 1 << 16
    res, _, _, tot = pxb.run(c3, 0, n3, want_digests=False)
    dev = torch.device("cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_res = torch.zeros((n3, 4), dtype=torch.int32, device=dev)
    d_tot = torch.zeros(pxb.NCOUNTERS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    pxb.run_device(c3, 0, n3, d_results=d_res, d_totals=d_tot, stream=s2.cuda_stream)
    keep = device_call(cfg, row, depth, sd, R, X.STUCK, True, 200, stream=s1.cuda_stream)
    pxb.run_device(c3, n3, n3, d_results=d_res, d_totals=d_tot, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _, d_ids, d_n, d_counts, d_status = keep
    X.check(d_ids.cpu().numpy()[:int(d_n.item())].astype(np.uint64), int(d_n.item()), d_counts.cpu().numpy().view(np.uint32),
            d_status.cpu().numpy().view(np.uint32), want, True)
    res2 = pxb.run(c3, n3, n3, want_digests=False)[0]
    assert np.array_equal(d_res.cpu().numpy().view(np.uint32), res2)
    pxb.stream_release(0, s2.cuda_stream)


# ---- 6. host-form chunking ----------------------------------------------------------------------------------
def test_host_form_chunks(gpu_lib):
    """PXB_EXPLORE_CHUNK = 20000 with 4 parents of shape (b) (T = 17,345): one
    parent a chunk; 40000: two; both equal the unchunked call."""
    cfg, row, depth, sd, R, T = X.shape("b")
    parents = np.stack([row] + list(pxb.explore_rows(cfg, row, depth, sd, R, [140, 1472])) + [row])
    whole = pxb.explore(cfg, parents, depth, sd, R, 0xFE, minimal=True)
    assert whole[1] > 0 and (whole[2][0] == whole[2][3]).all() and not (whole[2][0] == whole[2][1]).all()
    assert (np.diff(whole[0].astype(np.int64)) > 0).all() and whole[0][-1] >= 3 * T
    for chunk in (20000, 40000, 1):
        with pxb.hooks(PXB_EXPLORE_CHUNK=chunk):
            got = pxb.explore(cfg, parents, depth, sd, R, 0xFE, minimal=True)
            part = pxb.explore(cfg, parents, depth, sd, R, 0xFE, minimal=True, capacity=50)
        assert got[1] == whole[1] and all(np.array_equal(a, b) for a, b in zip((got[0],) + got[2:], (whole[0],) + whole[2:]))
        assert part[1] == whole[1] and np.array_equal(part[0], whole[0][:50])


# ---- 7. the loop closes ---------------------------------------------------------------------------------------
def test_minimal_candidates_through_shrink_batch(gpu_lib):
    cfg, row, depth, sd, R, T = X.shape("b")
    ids, n, _, _ = pxb.explore(cfg, row, depth, sd, R, X.LOG_DIV)
    assert n == 36 and ids[0] == 1472
    rows = pxb.explore_rows(cfg, row, depth, sd, R, ids)
    _, status, n_faults, launches, _, res, _ = pxb.shrink_batch(cfg, rows, X.LOG_DIV, depth=depth)
    assert (status == pxb.SHRINK_MINIMAL).all() and (n_faults == 3).all() and (launches == 2).all()
    assert ((res[:, 3] & X.LOG_DIV) != 0).all()
    # and the README's line: the first of them traced
    rec, offs, st, _ = pxb.trace_scripted(cfg, rows[:1], depth)
    assert st[0] == pxb.TRACE_OK and len(rec) == offs[1] > 0


# ---- 8. every kernel unit ---------------------------------------------------------------------------------------
# (P, N, delay_max): every proposer-count unit with the smallest and the largest
# acceptor count on the 8-step wheel, and one shape on the 16-step wheel
UNIT_SHAPES = [pytest.param(p, n, 4, id="%d-%d" % (p, n)) for p in (1, 2, 3) for n in (2, 9)] + [
    pytest.param(2, 3, 12, id="2-3-wheel16")]


def unit_case(P, N, delay_max):
    """(cfg, parents, depth, site_depth, radius): the benign row and an extracted
    row of a faulty config, every site changed once (T <= 1 + 54 * 4)."""
    cfg = pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                     delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                     step_cap=256)
    depth = 8
    return cfg, np.stack([X.benign_row(cfg, depth), SO.host_extract(cfg, [1], depth)[0]]), depth, 1, 1


@pytest.mark.parametrize("P,N,delay_max", UNIT_SHAPES)
def test_every_kernel_unit(gpu_lib, P, N, delay_max):
    """The list in both modes, the counts and the status equal the host build's
    (tests/native/explore_host.cpp) exactly."""
    cfg, parents, depth, sd, R = unit_case(P, N, delay_max)
    for minimal in (False, True):
        h = X.host_explore(cfg, parents, depth, sd, R, 0xFE, minimal=minimal)
        ids, n, counts, status = pxb.explore(cfg, parents, depth, sd, R, 0xFE, minimal=minimal)
        assert n == h["n"] and np.array_equal(ids, h["ids"])
        assert np.array_equal(counts, h["counts"]) and np.array_equal(status, h["status"])
    assert (status == pxb.TRACE_OK).all()
