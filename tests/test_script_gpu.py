"""Scripted schedules on the GPU (docs/SEMANTICS.md §10): pxb_schedule_extract,
pxb_run_scripted and pxb_trace_scripted against pxb.run / pxb.trace_batch for
all-keep rows, against the Python builder for the extract, against the host
build of the same lane (which tests/test_script_host.py ties to the reference
model) for overridden rows, the step KATs S1-S8, and pxb.shrink end to end."""
import dataclasses

import numpy as np
import pytest

import ev_matrix as M
import pxb
import script_oracle as SO
from test_ev_matrix import lane_host
from test_trace_batch_host import SELECTIONS

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A
OTHER_SEED = 0x0123456789ABCDEF
ACROSS = list(range((1 << 32) - 65, (1 << 32) + 65))        # 130 ids across 2^32


def runs(rec, offs):
    return [rec[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


@pytest.mark.parametrize("c", [3, 4, 5, 7])
def test_g1_all_keep_rows_equal_the_batch_run(gpu_lib, c):
    """All-keep rows (depth 0 and 8) give pxb.run's results, digests and acceptor
    records for the same ids wherever the lane does not bail; the status equals
    pxb.trace_batch's, BAILED within its 2 %."""
    cfg = pxb.CONFIGS[c]
    n = 256 if c == 5 else 130
    ids = np.arange(n, dtype=np.uint64)
    want_res, want_dig, want_acc, _ = pxb.run(cfg, 0, n, want_acceptors=True)
    _, _, tstatus, tres = pxb.trace_batch(cfg, ids, capacity=0)
    for depth in (0, 8):
        res, dig, acc, status, sent = pxb.run_scripted(cfg, pxb.scripts_empty(cfg, ids, depth), depth, want_acceptors=True)
        assert np.array_equal(status, tstatus) and np.array_equal(res, tres)
        ok = status == pxb.TRACE_OK
        assert np.array_equal(res[ok], want_res[ok]) and np.array_equal(dig[ok], want_dig[ok])
        assert np.array_equal(acc[ok], want_acc[ok])
        assert not res[~ok].any() and not dig[~ok].any() and not acc[~ok].any() and not sent[~ok].any()
        assert (sent[ok].reshape(int(ok.sum()), -1).sum(axis=1) > 0).all()
    assert int((~ok).sum()) <= 0.02 * n


@pytest.mark.parametrize("c", [3, 5])
def test_g2_extract_equals_the_python_builder(gpu_lib, c):
    cfg = pxb.CONFIGS[c]
    ids = ACROSS[53:77]                                 # 24 ids, 12 on each side of 2^32
    want = SO.build_rows(cfg, ids, 64)
    for depth in (1, 7, 64):
        got = pxb.extract_schedule(cfg, ids, depth)
        assert got.shape == (len(ids), pxb.script_stride(cfg, depth))
        off = pxb.script_links_off(cfg)
        assert np.array_equal(got[:, :off], want[:, :off])
        assert np.array_equal(pxb.script_links(cfg, got, depth), pxb.script_links(cfg, want, 64)[..., :depth])
        assert not got[:, off + 2 * cfg.n_proposers * cfg.n_acceptors * depth:].any()


def test_g2_extract_device_form(gpu_lib):
    import torch
    cfg = pxb.CONFIGS[4]
    depth, n = 7, 130
    stride = pxb.script_stride(cfg, depth)
    d_ids = torch.tensor(np.asarray(ACROSS, dtype=np.uint64).view(np.int64), device="cuda:0")
    d_rows = torch.full((n * stride + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    pxb.extract_schedule_device(cfg, d_ids, n, depth, d_rows)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy()
    assert (got[n * stride:] == 0x5A).all()
    assert np.array_equal(got[:n * stride].reshape(n, stride), SO.host_extract(cfg, ACROSS, depth))


@pytest.mark.parametrize("c", [3, 5])
def test_g3_extracted_rows_replay_under_another_seed_and_base(gpu_lib, c):
    cfg = pxb.CONFIGS[c]
    depth, n = 64, 130
    ids = np.arange(n, dtype=np.uint64)
    rows = pxb.extract_schedule(cfg, ids, depth)
    want_res, want_dig, _, _ = pxb.run(cfg, 0, n)
    moved = rows.copy()
    pxb.script_base(moved)[:] = np.random.default_rng(3).permutation(ids) + np.uint64((1 << 32) - 50)
    res, dig, _, status, sent = pxb.run_scripted(dataclasses.replace(cfg, seed=OTHER_SEED), moved, depth)
    h = SO.host_run(dataclasses.replace(cfg, seed=OTHER_SEED), moved, depth)
    assert np.array_equal(sent, h["sent"]) and np.array_equal(status, h["status"]) and np.array_equal(res, h["res"])
    covered = (status == pxb.TRACE_OK) & (sent.reshape(n, -1).max(axis=1) <= depth)
    assert covered.sum() >= n // 2
    assert np.array_equal(res[covered], want_res[covered]) and np.array_equal(dig[covered], want_dig[covered])


def test_g4_step_kats_through_trace_scripted(gpu_lib):
    """S1-S8 as explicit scripts under an unrelated seed and base: the result
    and every checkpoint equal the hand-derived fixtures."""
    for case, cfg, row, depth in SO.kat_cases():
        want = case["result"]
        rec, offs, status, res = pxb.trace_scripted(cfg, row, depth)
        assert status[0] == pxb.TRACE_OK, case["name"]
        assert list(res[0]) == [want["decided_val"], want["decided_ticket"], want["rounds"],
                                want["flags"] | (want["steps"] << 16)], case["name"]
        recs = {r["step"]: r for r in pxb.trace_records(rec)}
        for cp in case["checkpoints"]:
            g = recs[cp["step"]]
            assert g["acc"].tolist() == cp["acc"] and [list(p[:4]) for p in g["prop"].tolist()] == cp["prop"]
            if "in_flight" in cp:
                assert g["in_flight"] == cp["in_flight"]
        _, _, _, st, sent = pxb.run_scripted(cfg, row, depth)
        assert st[0] == pxb.TRACE_OK and int(sent.sum()) == want["messages"]


@pytest.mark.parametrize("c", [3, 4, 5, 7])
def test_g5_random_overrides_equal_the_host_build(gpu_lib, c):
    """The random-override rows of tests/test_script_host.py (which ties the host
    build to the reference model): results, digests, acceptor records, send
    counts and full traces equal the host build's."""
    cfg = pxb.CONFIGS[c]
    depth = 16
    ids = (list(range(64)) + ACROSS)[:130]
    rows = np.concatenate([SO.random_overrides(cfg, ids[:64], depth, seed=1000 + c),
                           SO.random_overrides(cfg, ids[64:], depth, seed=2000 + c)])
    h = SO.host_run(cfg, rows, depth, capacity=cfg.step_cap + 1)
    res, dig, acc, status, sent = pxb.run_scripted(cfg, rows, depth, want_acceptors=True)
    for got, k in ((res, "res"), (dig, "dig"), (acc, "acc"), (status, "status"), (sent, "sent")):
        assert np.array_equal(got, h[k]), k
    rec, offs, tstatus, tres = pxb.trace_scripted(cfg, rows, depth)
    assert np.array_equal(tstatus, status) and np.array_equal(tres, res)
    assert np.array_equal(np.diff(offs.astype(np.int64)), h["n_kept"])
    for i, g in enumerate(runs(rec, offs)):
        assert np.array_equal(g, h["rec"][i][:len(g)]), i
    assert (status == pxb.TRACE_OK).sum() >= 100


def test_g5_bad_rows(gpu_lib):
    cfg = pxb.CONFIGS[3]
    depth = 8
    rows = pxb.scripts_empty(cfg, range(130), depth)
    good = pxb.run_scripted(cfg, rows, depth, want_acceptors=True)
    grec, goffs, _, _ = pxb.trace_scripted(cfg, rows, depth)
    rows[3, 8] = 3
    rows[64, 9] = 1
    rows[129, 8] = 255
    bad = [3, 64, 129]
    got = pxb.run_scripted(cfg, rows, depth, want_acceptors=True)
    rec, offs, status, res = pxb.trace_scripted(cfg, rows, depth)
    keep = np.ones(130, bool)
    keep[bad] = False
    assert (got[3][bad] == pxb.SCRIPT_BAD).all() and np.array_equal(status, got[3])
    for j, (a, b) in enumerate(zip(got, good)):
        assert np.array_equal(a[keep], b[keep]), j
        assert j == 3 or not a[bad].any(), j           # (3: the status; every other output of a bad row is zero)
    gr, rr = runs(grec, goffs), runs(rec, offs)
    for i in range(130):
        assert (len(rr[i]) == 0) if i in bad else np.array_equal(rr[i], gr[i]), i


@pytest.mark.parametrize("sel", [SELECTIONS[1], SELECTIONS[5]])
def test_g6_trace_scripted_all_keep_is_trace_batch(gpu_lib, sel):
    """Records, offsets, status and results byte-equal to pxb.trace_batch(ids),
    for unsorted and repeated rows, under a selection, with a capacity that cuts
    the records (sentinels behind it intact) and in the sizing call."""
    import torch
    cfg = pxb.CONFIGS[3]
    ids = np.random.default_rng(6).permutation(np.arange(128, dtype=np.uint64))
    ids = np.concatenate([ids, ids[[5, 5]]])                       # 130 rows, one id three times
    kw = dict(step_min=sel[0], step_max=sel[1], tail=sel[2])
    want = pxb.trace_batch(cfg, ids, **kw)
    depth = 8
    rows = pxb.scripts_empty(cfg, ids, depth)
    got = pxb.trace_scripted(cfg, rows, depth, **kw)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    total = int(want[1][-1])
    capacity = total // 2
    while capacity in set(int(x) for x in want[1]):
        capacity += 1
    n = len(ids)
    dev = torch.device("cuda:0")
    d_rows = torch.tensor(rows.reshape(-1), device=dev)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_res = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    d_rec = torch.full((capacity + 64, pxb.TRACE_WORDS), SENT, dtype=torch.int32, device=dev)
    pxb.trace_scripted_device(cfg, d_rows, n, depth, d_off, d_rec, capacity, d_st, d_res, **kw)
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[1])
    assert np.array_equal(rec[:capacity], want[0][:capacity]) and (rec[capacity:] == SENT).all()
    assert np.array_equal(d_st.cpu().numpy().view(np.uint32), want[2])
    assert np.array_equal(d_res.cpu().numpy().view(np.uint32), want[3])
    d_off.fill_(-1)
    pxb.trace_scripted_device(cfg, d_rows, n, depth, d_off, None, 0, None, None, **kw)     # the sizing call
    torch.cuda.synchronize()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[1])


def test_g7_sweep_then_shrink(gpu_lib):
    """Config 3's first 4,096 ids swept for PANIC; the first three matches that
    are shrink inputs are shrunk on the GPU: the contract of
    tests/test_script_host.py's shrink test.  A match is a shrink input when its
    extracted row runs on the per-lane state machine (status OK) within `depth`
    entries on every link; pxb.shrink refuses the others (it raises), so they
    are passed over, and the test says how many were if it runs out of matches."""
    cfg = pxb.CONFIGS[3]
    depth = 64
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY)
    ids = pxb.sweep(cfg, 0, 4096, q, 64)[0]
    done, passed_over = 0, []
    for inst in (int(x) for x in ids):
        row0 = pxb.extract_schedule(cfg, [inst], depth)
        r0, _, _, st0, sent0 = pxb.run_scripted(cfg, row0, depth)
        if st0[0] != pxb.TRACE_OK or int(sent0.max()) > depth:
            passed_over.append(inst)                   # (beyond the lane or the table: not a shrink input)
            with pytest.raises(ValueError):
                pxb.shrink(cfg, inst, pxb.F_PANIC, depth=depth)
            continue
        before = pxb.script_faults(cfg, row0, depth, sent0[0])
        row, faults, launches = pxb.shrink(cfg, inst, pxb.F_PANIC, depth=depth)
        res, _, _, st, sent = pxb.run_scripted(cfg, row, depth)
        print("id %d: %d -> %d faults, %d -> %d steps, %d launches" % (
            inst, len(before), len(faults), int(r0[0][3]) >> 16, int(res[0][3]) >> 16, launches))
        assert st[0] == pxb.TRACE_OK and int(res[0][3]) & pxb.F_PANIC and int(sent.max()) <= depth
        assert faults == pxb.script_faults(cfg, row, depth, sent[0]) and 0 < len(faults) <= len(before)
        assert launches <= 64
        cand = np.repeat(row[None, :], len(faults), axis=0)
        for i, f in enumerate(faults):
            pxb.script_neutralise(cfg, cand[i:i + 1], depth, f)
        cr, _, _, cs, csent = pxb.run_scripted(cfg, cand, depth)
        for i in range(len(faults)):
            assert not (cs[i] == pxb.TRACE_OK and int(cr[i][3]) & pxb.F_PANIC and int(csent[i].max()) <= depth), faults[i]
        moved = row.copy()
        pxb.script_base(moved[None, :])[0] = (1 << 40) + inst
        mres, mdig, _, mst, msent = pxb.run_scripted(dataclasses.replace(cfg, seed=OTHER_SEED), moved, depth)
        assert np.array_equal(mres, res) and np.array_equal(msent, sent) and mst[0] == pxb.TRACE_OK
        done += 1
        if done == 3:
            break
    assert done == 3, "%d of %d matches shrunk; passed over (not shrink inputs): %s" % (done, len(ids), passed_over)


# (P, N, delay_max): every proposer-count unit with the smallest and the largest
# acceptor count on the 8-step wheel, and one shape on the 16-step wheel
UNIT_SHAPES = [pytest.param(p, n, 4, id="%d-%d" % (p, n)) for p in (1, 2, 3) for n in (2, 9)] + [
    pytest.param(2, 3, 12, id="2-3-wheel16")]


@pytest.mark.parametrize("P,N,delay_max", UNIT_SHAPES)
def test_g8_every_kernel_unit_launches(gpu_lib, P, N, delay_max):
    """64 rows of P proposers and N acceptors with random overrides: the GPU
    equals the host build (every proposer-count unit, the smallest and the
    largest acceptor count; both wheels)."""
    cfg = pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000,
                     delay_max=delay_max, skew_max=3, crash_ppm=100000, crash_len_max=8, crash_start_max=8,
                     step_cap=256)
    depth = 12
    rows = SO.random_overrides(cfg, list(range(64)), depth, seed=P * 10 + N)
    h = SO.host_run(cfg, rows, depth, capacity=cfg.step_cap + 1)
    res, dig, acc, status, sent = pxb.run_scripted(cfg, rows, depth, want_acceptors=True)
    for got, k in ((res, "res"), (dig, "dig"), (acc, "acc"), (status, "status"), (sent, "sent")):
        assert np.array_equal(got, h[k]), k
    rec, offs, _, _ = pxb.trace_scripted(cfg, rows, depth, tail=2)
    for i, g in enumerate(runs(rec, offs)):
        nk = int(h["n_kept"][i])
        assert len(g) == min(nk, 2) and np.array_equal(g, h["rec"][i][nk - len(g):nk]), i
    assert (status == pxb.TRACE_OK).sum() >= 32


@pytest.mark.parametrize("P,N,mode", M.LANE_SHAPES, ids=M.LANE_SHAPE_IDS)
def test_g9_every_shape_equals_the_oracle(gpu_lib, P, N, mode):
    """Every shape of the family (csrc/lane_shapes.h: P in 1..3, N in 2..9, both
    wheels and log mode) on g8's lossy schedule: 128 all-keep rows give the
    oracle's results, digests and acceptor records on every row that ends OK,
    at least 7/8 of the rows do, and the statuses are the host build's."""
    cfg = M.lane_cfg(P, N, mode)
    rows, h = lane_host(P, N, mode)
    eres, edig, eacc = M.lane_oracle(P, N, mode)
    res, dig, acc, status, sent = pxb.run_scripted(cfg, rows, M.LANE_DEPTH, want_acceptors=True)
    ok = status == pxb.TRACE_OK
    assert int((~ok).sum()) <= M.LANE_CAP
    assert np.array_equal(res[ok], eres[ok]) and np.array_equal(dig[ok], edig[ok]) and np.array_equal(acc[ok], eacc[ok])
    assert np.array_equal(status, h["status"]) and np.array_equal(sent, h["sent"])
