"""pxb_cover / pxb_cover_range on the GPU (docs/SEMANTICS.md §14): the kernels'
masks against the fold of the reference model's events and against the fold of
the GPU's own pxb.trace_events; the summary against numpy over the per-row
outputs; the range form against the rows form, whatever the chunk; the query
and its list; the device form on a stream of its own."""
import numpy as np
import pytest

import cover_oracle as CO
import pxb

pytestmark = pytest.mark.gpu
GPU_ROWS = 256
NONE64 = (1 << 64) - 1


@pytest.fixture(autouse=True)
def _library(gpu_lib):
    """The session's library handle, as the other GPU tests take it: torch finds the device before the library opens it."""


def check_outputs(cfg, rows, depth, want_masks, want_steps, got):
    masks, status, res, s = got
    assert (status == pxb.TRACE_OK).all()
    bad = np.nonzero(masks != want_masks)[0]
    assert len(bad) == 0, "row %d: gpu %s, oracle %s" % (bad[0], pxb.cover_names(masks[bad[0]]),
                                                        pxb.cover_names(want_masks[bad[0]]))
    assert ((res[:, 3] >> 16) == want_steps).all()
    assert CO.summary_dict(s) == CO.expected_summary(masks, status, res) and s.n_matches == 0
    # the counts are numpy's over the masks, the witnesses the argmin of (steps, i)
    steps = (res[:, 3] >> 16).astype(np.int64)
    for b in range(pxb.COVER_CLASSES):
        has = np.nonzero((masks >> b) & 1)[0]
        assert s.counts[b] == len(has)
        if len(has):
            i = int(has[np.lexsort((has, steps[has]))[0]])
            assert (s.witness[b], s.witness_steps[b]) == (i, int(steps[i]))
        else:
            assert (s.witness[b], s.witness_steps[b]) == (NONE64, 0xFFFFFFFF)


@pytest.mark.parametrize("form", ["keep", "extracted"])
@pytest.mark.parametrize("name", list(CO.CASES))
def test_cover_equals_the_oracle_and_the_fold_of_the_gpus_events(name, form):
    cfg, ids, masks, steps = CO.case_oracle(name, GPU_ROWS)
    if form == "keep":
        rows, depth = pxb.scripts_empty(cfg, ids, 0), 0
    else:
        depth = CO.EXTRACT_DEPTH
        rows = pxb.extract_schedule(cfg, ids, depth)
        got = [CO.oracle_row(cfg, rows[i], depth)[:2] for i in range(len(ids))]      # the oracle on the rows themselves
        assert [g[0] for g in got] == masks.tolist() and [g[1] for g in got] == steps.tolist()
    got = pxb.cover(cfg, rows, depth)
    check_outputs(cfg, rows, depth, masks, steps, got)
    ev, offs, st, res = pxb.trace_events(cfg, rows, depth)
    assert (st == got[1]).all() and (res == got[2]).all()
    for i in range(len(rows)):
        assert pxb.cover_of_events(ev[int(offs[i]):int(offs[i + 1])], cfg.n_acceptors) == int(got[0][i]), i


KATS = CO.kat_cases()


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_hand_derived_rows(case):
    cfg, row, depth = CO.kat_row(case)
    masks, status, res, s = pxb.cover(cfg, row, depth)
    assert status[0] == pxb.TRACE_OK and pxb.cover_names(int(masks[0])) == case["mask"]
    assert res[0, 3] >> 16 == case["steps"] and s.rows_ok == 1 and s.union == int(masks[0])
    ev, offs, _, _ = pxb.trace_events(cfg, row, depth)
    per = pxb.cover_of_events(ev, cfg.n_acceptors, per_event=True)
    assert len(ev) == case["n_events"]
    if "class" in case:
        bit = pxb.COVER_BIT[case["class"]]
        first = next(i for i, x in enumerate(per) if (x >> bit) & 1)
        assert first == case["event_index"] and pxb.event_lines(ev[first:first + 1]) == [case["event_line"]]


LOSSY = CO.CASES["lossy-p2n3"][0]
_by_ids = {}


def by_ids(first):
    """pxb.cover_ids of the 300 ids from `first`, once."""
    if first not in _by_ids:
        ids = (np.uint64(first) + np.arange(300, dtype=np.uint64)).astype(np.uint64)
        _by_ids[first] = (ids,) + pxb.cover_ids(LOSSY, ids)
    return _by_ids[first]


@pytest.mark.parametrize("first", [0, (1 << 32) - 50])
def test_cover_range_does_not_depend_on_the_chunk(first):
    ids, masks, status, res, s = by_ids(first)
    want = CO.expected_summary(masks, status, res, ids=[int(x) for x in ids])
    q = pxb.CoverQuery(any_mask=pxb.COVER_ALL)               # every OK row with some class: the list is the masks
    outs = [pxb.cover_range(LOSSY, first, 300, query=q, max_matches=300, chunk=c) for c in (64, 128, 0)]
    for o in outs:
        assert CO.summary_dict(o.summary) == want
        assert o.summary.n_matches == 300 == len(o.match_ids)
        assert o.match_ids.tolist() == [int(x) for x in ids] and (o.match_masks == masks).all()
    assert outs[0].summary == outs[1].summary == outs[2].summary
    # the rows form's summary over the same ids: row indices where the range form has ids
    assert s.counts == outs[0].summary.counts and s.witness_steps == outs[0].summary.witness_steps
    assert [int(ids[w]) if w != NONE64 else NONE64 for w in s.witness] == outs[0].summary.witness
    if first == 0:                                            # the oracle's masks of these ids
        assert (masks[:GPU_ROWS] == CO.case_oracle("lossy-p2n3", GPU_ROWS)[2]).all()
    # no query: no list, n_matches 0, the same summary otherwise
    plain = pxb.cover_range(LOSSY, first, 300, chunk=64)
    assert plain.summary.n_matches == 0 and len(plain.match_ids) == 0 and CO.summary_dict(plain.summary) == want
    empty = pxb.cover_range(LOSSY, first, 0)
    assert empty.summary.counts == [0] * 29 and empty.summary.witness == [NONE64] * 29 and empty.summary.union == 0


def test_cover_range_query_and_truncation():
    ids, masks, status, res, s = by_ids(0)
    q = pxb.CoverQuery(all_mask=pxb.COVER_Q1_FOREIGN_ACCEPT, none_mask=pxb.COVER_EXEC_PANIC)
    want = [int(i) for i, m in zip(ids, masks) if q.matches(int(m))]
    assert len(want) >= 8                                     # (Q1 is common in the duel: 874 of 3,000 in the oracle)
    for chunk in (64, 0):
        full = pxb.cover_range(LOSSY, 0, 300, query=q, max_matches=300, chunk=chunk)
        assert full.summary.n_matches == len(want) and full.match_ids.tolist() == want
        assert full.match_ids.tolist() == sorted(want)
        assert full.match_masks.tolist() == [int(masks[i]) for i in want]
        cut = pxb.cover_range(LOSSY, 0, 300, query=q, max_matches=5, chunk=chunk)
        assert cut.summary.n_matches == len(want) and cut.match_ids.tolist() == want[:5]
        assert cut.match_masks.tolist() == [int(masks[i]) for i in want[:5]]
        none = pxb.cover_range(LOSSY, 0, 300, query=q, max_matches=0, chunk=chunk)
        assert none.summary.n_matches == len(want) and len(none.match_ids) == 0
        assert CO.summary_dict(none.summary) == CO.summary_dict(full.summary)


def test_cover_device_on_a_stream_of_its_own():
    import torch
    cfg, ids, masks, steps = CO.case_oracle("lossy-p2n3", 130)
    depth = 0
    rows = pxb.scripts_empty(cfg, ids, depth)
    n = len(rows)
    want = pxb.cover(cfg, rows, depth)
    dev = torch.device("cuda:0")
    guard = 8
    d_rows = torch.from_numpy(rows.reshape(-1)).to(dev)
    d_masks = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_status = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_res = torch.full((n + guard, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_sum = torch.full((pxb.COVER_SUMMARY_BYTES + 16,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        pxb.cover_device(cfg, d_rows, n, depth, d_masks, d_status, d_res, d_sum[:pxb.COVER_SUMMARY_BYTES],
                         stream=stream.cuda_stream)
    stream.synchronize()                                      # (nothing is read before this)
    got_m = d_masks.cpu().numpy().view(np.uint32)
    got_st = d_status.cpu().numpy().view(np.uint32)
    got_res = d_res.cpu().numpy().view(np.uint32)
    raw = d_sum.cpu().numpy()
    assert (got_m[:n] == want[0]).all() and (got_st[:n] == want[1]).all() and (got_res[:n] == want[2]).all()
    assert (got_m[:n] == masks).all()
    assert (got_m[n:] == 0x5A5A5A5A).all() and (got_st[n:] == 0x5A5A5A5A).all() and (got_res[n:] == 0x5A5A5A5A).all()
    assert (raw[pxb.COVER_SUMMARY_BYTES:] == 0x5A).all()
    assert pxb.cover_summary_from(raw[:pxb.COVER_SUMMARY_BYTES]) == want[3]
    # every output is optional: the summary alone, and the masks alone
    d_sum2 = torch.zeros(pxb.COVER_SUMMARY_BYTES, dtype=torch.uint8, device=dev)
    d_m2 = torch.zeros(n, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        pxb.cover_device(cfg, d_rows, n, depth, d_summary=d_sum2, stream=stream.cuda_stream)
        pxb.cover_device(cfg, d_rows, n, depth, d_masks=d_m2, stream=stream.cuda_stream)
    stream.synchronize()
    assert pxb.cover_summary_from(d_sum2.cpu()) == want[3] and (d_m2.cpu().numpy().view(np.uint32) == want[0]).all()


def test_bad_and_bailed_rows_among_good_ones():
    cfg, rows, i_bad, i_bail = CO.bad_and_bailed_rows()
    masks, status, res, s = pxb.cover(cfg, rows, 0)
    CO.check_bad_and_bailed(cfg, rows, i_bad, i_bail, masks, status, res, s)


def test_counts_off_the_wave_size_and_count_zero():
    cfg, ids, masks, steps = CO.case_oracle("lossy-p2n3", GPU_ROWS)
    for n in (1, 63, 65, 130):
        check_outputs(cfg, None, 0, masks[:n], steps[:n], pxb.cover(cfg, pxb.scripts_empty(cfg, ids[:n], 0), 0))
    m, st, res, s = pxb.cover(cfg, pxb.scripts_empty(cfg, ids[:0], 0), 0)
    assert len(m) == 0 and s.counts == [0] * 29 and s.witness == [NONE64] * 29 and s.union == 0 and s.rows_ok == 0
