"""GPU checks of the result queries: pxb_query_device on synthetic records and
pxb_sweep on real runs, against a numpy restatement of the semantics of
include/paxos_batch.h (ref_query below).  Integers only: every comparison is
exact."""
import numpy as np
import pytest

import oracle_c
import pxb

pytestmark = pytest.mark.gpu

FIRST = (1 << 32) - 1000          # the synthetic records' first instance: ids cross 2^32
N_MAX = (1 << 22) + 5
SENT = -0x0123456789ABCDEF        # what untouched id slots hold
SENT32 = 0x5A5A5A5A               # ... and untouched words of the matched records
PAD = 64                          # sentinel entries after the `capacity` ones
U32 = 0xFFFFFFFF


def ref_query(res, first, q, capacity, cursor=0, hist_steps=None, hist_rounds=None):
    """The semantics, restated: (ids written, records written, slots they land
    in, new cursor, steps bins, rounds bins) for uint32 (n, 4) records."""
    flags, rounds = res[:, 3], res[:, 2]
    f, steps = flags & np.uint32(q.flag_mask), flags >> np.uint32(16)
    fl = {pxb.Q_ANY: f != 0, pxb.Q_ALL: f == q.flag_mask, pxb.Q_NONE: f == 0}[q.flag_mode]
    m = fl & (steps >= q.steps_min) & (steps <= q.steps_max) & (rounds >= q.rounds_min) & (rounds <= q.rounds_max)
    idx = np.nonzero(m)[0]
    slots = cursor + np.arange(idx.size)
    keep = slots < capacity
    hs = np.zeros(q.n_bins_steps, np.int64) if hist_steps is None else hist_steps.copy()
    hr = np.zeros(q.n_bins_rounds, np.int64) if hist_rounds is None else hist_rounds.copy()
    if q.n_bins_steps:
        hs += np.bincount(np.minimum(steps[m], q.n_bins_steps - 1), minlength=q.n_bins_steps)
    if q.n_bins_rounds:
        hr += np.bincount(np.minimum(rounds[m], q.n_bins_rounds - 1), minlength=q.n_bins_rounds)
    ids = (np.uint64(first) + idx.astype(np.uint64))[keep]
    return ids, res[idx[keep]], slots[keep], cursor + idx.size, hs, hr


@pytest.fixture(scope="module")
def records(gpu_lib):
    """Random uint32 quadruples (flag bits 8..15 random too: the mask must
    ignore them); every other record's rounds are below 9000 so that the rounds
    bins are spread as well as clamped.  (host array, device tensor), read-only."""
    import torch
    rng = np.random.default_rng(0x5EED51)
    res = rng.integers(0, 1 << 32, size=(N_MAX, 4), dtype=np.uint32)
    res[1::2, 2] %= 9000
    d_res = torch.from_numpy(res.view(np.int32)).cuda()
    res.setflags(write=False)
    return res, d_res


def device_query(d_res, first, n, q, capacity, cursor=0, hist_steps=None, hist_rounds=None, lists=True):
    """One pxb_query_device call into sentinel-filled buffers.  Returns the
    whole id and record buffers (capacity + PAD entries), the cursor and bins."""
    import torch
    dev = d_res.device
    d_ids = torch.full((capacity + PAD,), SENT, dtype=torch.int64, device=dev) if lists else None
    d_m = torch.full((capacity + PAD, 4), SENT32, dtype=torch.int32, device=dev) if lists else None
    d_cur = torch.tensor([cursor], dtype=torch.int64, device=dev)

    def bins(nb, init):
        if not nb:
            return None
        return torch.zeros(nb, dtype=torch.int64, device=dev) if init is None else torch.from_numpy(init.copy()).to(dev)
    d_hs, d_hr = bins(q.n_bins_steps, hist_steps), bins(q.n_bins_rounds, hist_rounds)
    pxb.query_device(d_res[:n], first, n, q, d_cur, d_ids, d_m, capacity, d_hs, d_hr)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(d_ids), host(d_m), int(d_cur.item()), host(d_hs), host(d_hr)


def check(got, exp, capacity):
    ids, recs, cur, hs, hr = got
    eids, erecs, slots, ecur, ehs, ehr = exp
    assert cur == ecur
    want_ids = np.full(capacity + PAD, SENT, np.int64)
    want_ids[slots] = eids.view(np.int64)
    want_recs = np.full((capacity + PAD, 4), SENT32, np.int32)
    want_recs[slots] = erecs.view(np.int32)
    bad = np.nonzero(ids != want_ids)[0]
    assert bad.size == 0, "first differing id slot %d: %d, expected %d" % (bad[0], ids[bad[0]], want_ids[bad[0]])
    assert np.array_equal(recs, want_recs)
    assert (hs is None and ehs.size == 0) or np.array_equal(hs, ehs)
    assert (hr is None and ehr.size == 0) or np.array_equal(hr, ehr)


# the three flag modes with a mix of ranges, and the three LDS shapes of the
# count pass (both full histograms, small ones, none)
QUERIES = [
    pxb.Query(flag_mask=0x05, flag_mode=pxb.Q_ANY, n_bins_steps=257, n_bins_rounds=pxb.HIST_MAX_BINS),
    pxb.Query(flag_mask=0x03, flag_mode=pxb.Q_ALL, steps_min=10000, steps_max=50000, n_bins_steps=1024),
    pxb.Query(flag_mask=0xF0, flag_mode=pxb.Q_NONE, rounds_min=1 << 30, rounds_max=3 << 30),
    pxb.Query(flag_mask=0x81, flag_mode=pxb.Q_ANY, steps_min=123, steps_max=40000, rounds_min=17, rounds_max=8000,
              n_bins_steps=pxb.HIST_MAX_BINS, n_bins_rounds=100),
]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 200003, N_MAX])
def test_query_matches_numpy(records, n):
    res, d_res = records
    for q in QUERIES:
        exp = ref_query(res[:n], FIRST, q, n)
        if n >= 4095:
            assert 0 < exp[3] < n                     # (a real split)
        check(device_query(d_res, FIRST, n, q, n), exp, n)


def test_all_none_and_last_only(records):
    import torch
    res, d_res = records
    n = 200003
    everything = pxb.Query(n_bins_steps=300, n_bins_rounds=300)
    exp = ref_query(res[:n], FIRST, everything, n)
    assert exp[3] == n and exp[4].sum() == n
    check(device_query(d_res, FIRST, n, everything, n), exp, n)
    for nothing in (pxb.Query(steps_min=5, steps_max=4, n_bins_steps=300),         # min > max
                    pxb.Query(rounds_min=U32, rounds_max=0),
                    pxb.Query(flag_mask=0xFF, flag_mode=pxb.Q_ALL, steps_min=70000)):
        exp = ref_query(res[:n], FIRST, nothing, n)
        assert exp[3] == 0
        check(device_query(d_res, FIRST, n, nothing, n), exp, n)
    last = res[:n].copy()
    last[:, 2] = 5
    last[-1, 2] = 7
    only_last = pxb.Query(rounds_min=7, rounds_max=7, n_bins_rounds=8)
    exp = ref_query(last, FIRST, only_last, n)
    assert exp[3] == 1 and exp[0][0] == FIRST + n - 1
    check(device_query(torch.from_numpy(last.view(np.int32)).cuda(), FIRST, n, only_last, n), exp, n)


def test_append_two_halves_equal_one_call(records):
    import torch
    res, d_res = records
    n, h = 200003, 100001
    for q in QUERIES:
        whole = device_query(d_res, FIRST, n, q, n)
        dev = d_res.device
        d_ids = torch.full((n + PAD,), SENT, dtype=torch.int64, device=dev)
        d_m = torch.full((n + PAD, 4), SENT32, dtype=torch.int32, device=dev)
        d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        d_hs = torch.zeros(q.n_bins_steps, dtype=torch.int64, device=dev) if q.n_bins_steps else None
        d_hr = torch.zeros(q.n_bins_rounds, dtype=torch.int64, device=dev) if q.n_bins_rounds else None
        pxb.query_device(d_res[:h], FIRST, h, q, d_cur, d_ids, d_m, n, d_hs, d_hr)
        pxb.query_device(d_res[h:n], FIRST + h, n - h, q, d_cur, d_ids, d_m, n, d_hs, d_hr)
        torch.cuda.synchronize()
        assert int(d_cur.item()) == whole[2] == ref_query(res[:n], FIRST, q, n)[3]
        assert np.array_equal(d_ids.cpu().numpy(), whole[0]) and np.array_equal(d_m.cpu().numpy(), whole[1])
        for d, w in ((d_hs, whole[3]), (d_hr, whole[4])):
            assert (d is None and w is None) or np.array_equal(d.cpu().numpy(), w)


@pytest.mark.parametrize("capacity,cursor", [(1, 0), (1000, 0), (1000, 990), (1000, 1000), (1000, 5000), (4097, 3)])
def test_capacity_bounds_the_list_not_the_count(records, capacity, cursor):
    """Fewer slots than matches: exactly the slots below `capacity` are written
    (from the cursor on), the count is the full total, and the sentinel entries
    after the buffer's `capacity` entries are untouched."""
    res, d_res = records
    n, q = 200003, QUERIES[0]
    exp = ref_query(res[:n], FIRST, q, capacity, cursor)
    assert exp[3] - cursor > capacity and exp[0].size == max(0, capacity - cursor)
    got = device_query(d_res, FIRST, n, q, capacity, cursor)
    check(got, exp, capacity)
    assert (got[0][capacity:] == SENT).all() and (got[1][capacity:] == SENT32).all()


def test_capacity_zero_is_histogram_only(records):
    res, d_res = records
    n, q = 200003, QUERIES[0]
    _, _, _, total, ehs, ehr = ref_query(res[:n], FIRST, q, 0)
    ids, recs, cur, hs, hr = device_query(d_res, FIRST, n, q, 0, lists=False)     # null id and record pointers
    assert ids is None and recs is None and cur == total
    assert np.array_equal(hs, ehs) and np.array_equal(hr, ehr)


@pytest.mark.parametrize("n_bins", [1, 2, 257, pxb.HIST_MAX_BINS])
def test_histogram_clamps_into_the_last_bin(records, n_bins):
    res, d_res = records
    n = 200003
    q = pxb.Query(flag_mask=0x10, flag_mode=pxb.Q_ANY, n_bins_steps=n_bins, n_bins_rounds=n_bins)
    exp = ref_query(res[:n], FIRST, q, 0)
    assert exp[4].sum() == exp[5].sum() == exp[3] and exp[4][-1] > 0 and exp[5][-1] > 0
    _, _, cur, hs, hr = device_query(d_res, FIRST, n, q, 0, lists=False)
    assert cur == exp[3] and np.array_equal(hs, exp[4]) and np.array_equal(hr, exp[5])


def test_histogram_one_hot_bin_and_accumulation(gpu_lib):
    """Every record in one bin (what a fault-free run gives: one value for all
    of a wave's lanes), and counts added to pre-filled bins over two calls."""
    import torch
    n = 200003
    res = np.zeros((n, 4), np.uint32)
    res[:, 2] = 6
    res[:, 3] = (256 << 16) | pxb.F_STEP_CAP
    d_res = torch.from_numpy(res.view(np.int32)).cuda()
    for n_bins in (257, pxb.HIST_MAX_BINS):
        q = pxb.Query(flag_mask=pxb.F_STEP_CAP, flag_mode=pxb.Q_ALL, n_bins_steps=n_bins, n_bins_rounds=n_bins)
        pre_s, pre_r = np.arange(n_bins, dtype=np.int64), np.arange(n_bins, dtype=np.int64)[::-1] * 3
        _, _, cur, hs, hr = device_query(d_res, 0, n, q, 0, hist_steps=pre_s, hist_rounds=pre_r, lists=False)
        want_s, want_r = pre_s.copy(), pre_r.copy()
        want_s[256] += n
        want_r[6] += n
        assert cur == n and np.array_equal(hs, want_s) and np.array_equal(hr, want_r)
        _, _, cur, hs, hr = device_query(d_res, 0, n, q, 0, cursor=cur, hist_steps=hs, hist_rounds=hr, lists=False)
        want_s[256] += n
        want_r[6] += n
        assert cur == 2 * n and np.array_equal(hs, want_s) and np.array_equal(hr, want_r)


def test_same_call_twice_is_byte_identical(records):
    res, d_res = records
    for q in QUERIES:
        a = device_query(d_res, FIRST, N_MAX, q, N_MAX)
        b = device_query(d_res, FIRST, N_MAX, q, N_MAX)
        assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        for x, y in ((a[3], b[3]), (a[4], b[4])):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- pxb_sweep against pxb_run -------------------------------------------------
SWEEP_FIRST, SWEEP_N = (1 << 32) - 5000, 20000      # five 4096-chunks, ragged last, crossing 2^32
SWEEPS = {
    3: pxb.Query(flag_mask=pxb.F_PANIC | pxb.F_LOG_DIVERGENCE, flag_mode=pxb.Q_ANY, n_bins_steps=257),
    4: pxb.Query(flag_mask=pxb.F_STEP_CAP, flag_mode=pxb.Q_ANY, n_bins_steps=257),     # one hot bin: the step cap
    7: pxb.Query(flag_mask=pxb.F_STUCK, flag_mode=pxb.Q_NONE, n_bins_steps=257),       # log mode
}
_runs = {}


def full_run(c):
    """pxb.run's results and totals of the sweep's instances (computed once)."""
    if c not in _runs:
        res, _, _, cnt = pxb.run(pxb.CONFIGS[c], SWEEP_FIRST, SWEEP_N, want_digests=False)
        res.setflags(write=False)
        _runs[c] = (res, cnt)
    return _runs[c]


@pytest.mark.parametrize("c", sorted(SWEEPS))
def test_sweep_equals_query_over_run(gpu_lib, c):
    q = SWEEPS[c]
    res, cnt = full_run(c)
    eids, erecs, _, total, ehs, _ = ref_query(res, SWEEP_FIRST, q, SWEEP_N)
    assert 0 < total < SWEEP_N                           # not vacuous
    with pxb.hooks(PXB_SWEEP_CHUNK=4096):
        ids, matched, n_matches, hs, hr, totals = pxb.sweep(pxb.CONFIGS[c], SWEEP_FIRST, SWEEP_N, q, SWEEP_N)
    assert n_matches == total and ids.dtype == np.uint64
    assert np.array_equal(ids, eids) and np.array_equal(matched, erecs)
    assert ids.min() < (1 << 32) <= ids.max()            # the list crosses 2^32
    assert np.array_equal(hs, ehs) and hs.sum() == total and hr.size == 0
    assert totals == cnt
    # ... and the ids are the ones the C oracle's results give
    ores = oracle_c.run_cpu(pxb.CONFIGS[c], SWEEP_FIRST, SWEEP_N, threads=8)[0]
    assert np.array_equal(ids, ref_query(ores, SWEEP_FIRST, q, SWEEP_N)[0])
    # the default chunk (one chunk here) gives the same answer
    one = pxb.sweep(pxb.CONFIGS[c], SWEEP_FIRST, SWEEP_N, q, SWEEP_N)
    assert np.array_equal(one[0], ids) and np.array_equal(one[1], matched) and one[2] == total
    assert np.array_equal(one[3], hs) and one[5] == cnt


def test_sweep_capacity_ten(gpu_lib):
    q = SWEEPS[3]
    res, cnt = full_run(3)
    eids, erecs, _, total, _, _ = ref_query(res, SWEEP_FIRST, q, SWEEP_N)
    assert total > 10
    with pxb.hooks(PXB_SWEEP_CHUNK=4096):
        ids, matched, n_matches, hs, _, totals = pxb.sweep(pxb.CONFIGS[3], SWEEP_FIRST, SWEEP_N, q, 10)
    assert n_matches == total and totals == cnt and hs.sum() == total
    assert np.array_equal(ids, eids[:10]) and np.array_equal(matched, erecs[:10])      # the ten smallest ids


def test_sweep_of_nothing(gpu_lib):
    ids, matched, n_matches, hs, hr, totals = pxb.sweep(pxb.CONFIGS[3], 5, 0, pxb.Query(n_bins_rounds=4), 8)
    assert ids.size == 0 and matched.shape == (0, 4) and n_matches == 0
    assert not hs.size and not hr.any() and not any(totals.values())


def test_sweep_then_trace(gpu_lib):
    """The workflow: sweep for the panics, trace the first id."""
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY)
    with pxb.hooks(PXB_SWEEP_CHUNK=4096):
        ids, matched, n_matches, _, _, totals = pxb.sweep(pxb.CONFIGS[3], SWEEP_FIRST, SWEEP_N, q, 4)
    assert 0 < n_matches < SWEEP_N and n_matches == totals["panic"]
    _, result = pxb.trace_instance(pxb.CONFIGS[3], int(ids[0]))
    assert result[3] & pxb.F_PANIC
    assert np.array_equal(result, matched[0])
