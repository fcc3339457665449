"""Handler events of scripted rows on the GPU (docs/SEMANTICS.md §13):
pxb_trace_events against the host build of the same lane and reorder step
(which tests/test_events_host.py ties to the reference model), against the
event oracle directly for some rows, against pxb.trace_scripted,
pxb.run_scripted and pxb.run, and at the end of the sweep -> shrink loop."""
import dataclasses

import numpy as np
import pytest

import event_oracle as EO
import pxb
from test_events_host import FX, check_row, fixture_events, fixture_row

pytestmark = pytest.mark.gpu
ACROSS = list(range((1 << 32) - 65, (1 << 32) + 65))        # 130 ids across 2^32: two full waves and a ragged third
DEPTH = 16
GUARD = 0xA5


def _c(**kw):
    return pxb.Config(**dict(dict(seed=0xE7E27, loss_ppm=100000, skew_max=3, step_cap=96), **kw))


GRID = {
    "p1n3-w8": _c(n_proposers=1, n_acceptors=3, delay_max=4),
    "p2n3-w8": _c(n_proposers=2, n_acceptors=3, delay_max=4),
    "p3n9-w16": _c(n_proposers=3, n_acceptors=9, delay_max=15, loss_ppm=50000),
    "log-p2n3": dataclasses.replace(pxb.LOG_FAULTY_CONFIG, n_acceptors=3, step_cap=96),
}
_grid = {}


def grid_rows(cfg, seed):
    """Explicit rows of ACROSS (extracted on the GPU) with about 10 % of the link
    entries overridden (a quarter of those lost, the rest delays up to delay_max
    + 3), some proposer-count, skew and window overrides, and every fifth row
    all-keep under its overrides."""
    rng = np.random.default_rng(seed)
    rows = pxb.extract_schedule(cfg, ACROSS, DEPTH)
    keep = pxb.scripts_empty(cfg, ACROSS, DEPTH)
    rows[4::5] = keep[4::5]
    lk = pxb.script_links(cfg, rows, DEPTH)
    m = rng.random(lk.shape) < 0.10
    v = np.where(rng.random(lk.shape) < 0.25, 0, rng.integers(1, cfg.delay_max + 4, lk.shape)).astype(np.uint8)
    lk[m] = v[m]
    for i in range(len(rows)):
        if rng.random() < 0.25:
            pxb.script_n_proposers(rows)[i] = rng.integers(1, cfg.n_proposers + 1)
        if rng.random() < 0.25:
            pxb.script_skews(rows)[i, rng.integers(0, 3)] = rng.integers(0, 6)
        if rng.random() < 0.25:
            c0 = int(rng.integers(0, 12))
            pxb.script_windows(cfg, rows)[i, rng.integers(0, cfg.n_acceptors)] = (c0, c0 + int(rng.integers(0, 10)))
    return rows


def grid(name):
    """(cfg, rows, the device's (events, offsets, status, results)), once per config."""
    if name not in _grid:
        cfg = GRID[name]
        rows = grid_rows(cfg, 40 + list(GRID).index(name))
        _grid[name] = (cfg, rows, pxb.trace_events(cfg, rows, DEPTH))
    return _grid[name]


@pytest.mark.parametrize("name", list(GRID))
def test_e1_grid_equals_the_host_lane_and_the_oracle(gpu_lib, name):
    cfg, rows, (ev, offs, st, res) = grid(name)
    rc, hev, hoffs, hst, hres, total = EO.host_events(cfg, rows, DEPTH)
    assert rc == 0
    assert np.array_equal(offs, hoffs) and np.array_equal(st, hst) and np.array_equal(res, hres)
    assert len(ev) == total and ev.tobytes() == hev.tobytes()
    ok = np.flatnonzero(st == pxb.TRACE_OK)
    assert len(ok) >= 0.9 * len(rows) and total > 0
    for i in ok[:16]:
        check_row(cfg, rows[i], DEPTH, ev[int(offs[i]):int(offs[i + 1])])


@pytest.mark.parametrize("case", FX["cases"], ids=[c["name"] for c in FX["cases"]])
def test_e1_hand_derived_events_on_the_device(gpu_lib, case):
    """tests/golden/kat_events.json (one proposer: the unit of P = 1) through the
    device: the fixture's bytes, alone and as rows of a ragged second wave."""
    cfg, row, depth = fixture_row(case)
    want = fixture_events(case)
    ev, offs, st, res = pxb.trace_events(cfg, row, depth)
    assert st[0] == pxb.TRACE_OK and offs.tolist() == [0, len(want)]
    assert pxb.event_lines(ev) == pxb.event_lines(want) and ev.tobytes() == want.tobytes()
    ev, offs, st, res = pxb.trace_events(cfg, np.stack([row] * 67), depth)
    assert (st == pxb.TRACE_OK).all() and ev.tobytes() == want.tobytes() * 67


def test_e2_repeated_rows_give_identical_events(gpu_lib):
    cfg, rows, (ev, offs, st, res) = grid("p2n3-w8")
    i = next(j for j in range(len(rows)) if st[j] == pxb.TRACE_OK and offs[j + 1] - offs[j] > 8)
    rep = np.stack([rows[i]] * 70)                              # (a full wave and part of a second)
    ev2, offs2, st2, res2 = pxb.trace_events(cfg, rep, DEPTH)
    one = ev[int(offs[i]):int(offs[i + 1])].tobytes()
    assert ev2.tobytes() == one * 70 and (np.diff(offs2) == len(one) // 96).all()
    assert (st2 == st[i]).all() and (res2 == res[i]).all()


def test_e3_capacity_cut_device_form(gpu_lib):
    """A capacity in the middle of the batch (inside a row, inside a step): the
    prefix equals the full call's, the guard behind it stays intact; the sizing
    call and count == 0."""
    import torch
    cfg, rows, (ev, offs, st, res) = grid("p3n9-w16")
    n, total = len(rows), len(ev)
    d_rows = torch.tensor(rows.reshape(-1), device="cuda:0")
    steps = ev["step"]
    r = next(j for j in range(66, n) if offs[j + 1] - offs[j] > 20)     # (a row of the second wave)
    cut = next(k for k in range(int(offs[r]) + 1, int(offs[r + 1]))
               if steps[k] == steps[k - 1] and ev["actor"][k - 1] != ev["actor"][k])
    for cap in (cut, int(offs[64]), total):
        pad = 300
        d_ev = torch.full(((cap + pad) * 96,), GUARD, dtype=torch.uint8, device="cuda:0")
        d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        d_res = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
        pxb.trace_events_device(cfg, d_rows, n, DEPTH, d_offs, d_ev, cap, d_st, d_res)
        torch.cuda.synchronize()
        got = d_ev.cpu().numpy()
        assert got[:cap * 96].tobytes() == ev[:cap].tobytes(), cap
        assert (got[cap * 96:] == GUARD).all(), cap
        assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), offs)
        assert np.array_equal(d_st.cpu().numpy().view(np.uint32), st)
        assert np.array_equal(d_res.cpu().numpy().view(np.uint32), res)
    d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    pxb.trace_events_device(cfg, d_rows, n, DEPTH, d_offs)      # the sizing call
    torch.cuda.synchronize()
    assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), offs)
    d_one = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    pxb.trace_events_device(cfg, None, 0, DEPTH, d_one)         # count == 0
    torch.cuda.synchronize()
    assert d_one.cpu().numpy().tolist() == [0]
    # a step window through the host form
    wev, woffs, wst, wres = pxb.trace_events(cfg, rows, DEPTH, step_min=3, step_max=9)
    keep = (ev["step"] >= 3) & (ev["step"] <= 9)
    assert wev.tobytes() == ev[keep].tobytes() and np.array_equal(wst, st) and np.array_equal(wres, res)
    assert [int(x) for x in np.diff(woffs)] == [int(keep[int(offs[i]):int(offs[i + 1])].sum()) for i in range(n)]


@pytest.mark.parametrize("name", list(GRID))
def test_e4_consistent_with_the_scripted_trace_and_run(gpu_lib, name):
    """Per row and step with events, the last "after" of each actor equals
    pxb.trace_scripted's step record; results and status equal
    pxb.run_scripted's."""
    cfg, rows, (ev, offs, st, res) = grid(name)
    rres, _, _, rstatus, _ = pxb.run_scripted(cfg, rows, DEPTH)
    assert np.array_equal(rres, res) and np.array_equal(rstatus, st)
    rec, roffs, tst, tres = pxb.trace_scripted(cfg, rows, DEPTH)
    assert np.array_equal(tst, st) and np.array_equal(tres, res)
    recs = pxb.trace_records(rec)
    for i in range(len(rows)):
        by_step = {int(r["step"]): r for r in recs[int(roffs[i]):int(roffs[i + 1])]}
        mine = ev[int(offs[i]):int(offs[i + 1])]
        assert (st[i] == pxb.TRACE_OK) or len(mine) == 0
        for s, (acc, prop) in EO.last_after(mine, cfg.n_acceptors, cfg.n_proposers).items():
            r = by_step[s]
            for a, after in acc.items():
                assert after == tuple(int(x) for x in r["acc"][a]) + (int(r["digest"][a]),), (i, s, a)
            for p, after in prop.items():
                assert after == tuple(int(x) for x in r["prop"][p]), (i, s, p)


def test_e5_plain_instances_and_the_shrink_loop(gpu_lib):
    """Config 3's PANIC ids of a 2^16 sweep: trace_events_ids gives pxb.run's
    results; shrink_batch on 64 of them, then trace_events on the shrunk rows:
    every OK row shows the acceptor dying."""
    cfg = pxb.CONFIGS[3]
    n = 1 << 16
    ids, _, n_matches, _, _, _ = pxb.sweep(cfg, 0, n, pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY), 256)
    assert n_matches >= 64 and len(ids) >= 64
    want, _, _, _ = pxb.run(cfg, 0, n)
    ev, offs, st, res = pxb.trace_events_ids(cfg, ids)
    ok = st == pxb.TRACE_OK
    assert ok.sum() >= 0.95 * len(ids) and np.array_equal(res[ok], want[ids[ok].astype(np.int64)])
    assert not res[~ok].any() and (np.diff(offs)[~ok] == 0).all() and (np.diff(offs)[ok] > 0).all()
    depth = 64
    rows, sstatus, n_faults, _, sent, sres, _ = pxb.shrink_batch(cfg, ids[:64], pxb.F_PANIC, depth=depth)
    ev, offs, st, res = pxb.trace_events(cfg, rows, depth)
    shown = 0
    for i in range(64):
        if st[i] != pxb.TRACE_OK:
            continue
        mine = ev[int(offs[i]):int(offs[i + 1])]
        died = (mine["actor"] == pxb.EVT_ACCEPTOR) & (mine["after"][:, 3] >> 31 == 1)
        assert died.any() and int(res[i][3]) & pxb.F_PANIC, i
        first = mine[np.argmax(died)]                           # the Execute that found nothing stored
        assert first["in"]["kind"] == 2 and first["n_out"] == 0 and first["after"][2] == 0
        shown += 1
        if int(sent[i].max()) <= depth and not (pxb.script_links(cfg, rows[i:i + 1], depth) == 0xFF).any():
            chart = pxb.message_chart(cfg, rows[i], depth, mine)
            assert len(chart) == int(sent[i].sum())
    assert shown >= 48
