"""Handler events of scripted rows (docs/SEMANTICS.md §13) without a GPU.

The event lane the kernels run (csrc/events_core.h: the tapped draw source and
EventLane over the scripted lane) and the reorder step are compiled for the
HOST (tests/native/events_host.cpp) and checked, byte for byte, against the
event list of the reference model (tests/event_oracle.py), which is itself
pinned to the unmodified ``run_instance`` on every case; against two
hand-derived fixtures (tests/golden/kat_events.json); through
``pxb.message_chart``'s invariants; at the C-ABI boundary of the new entry
points; and by one stand-alone AddressSanitizer + UBSan program (its own main;
nothing is loaded into Python)."""
import ctypes as C
import dataclasses
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import event_oracle as EO
import paxos_ref as R
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "events_host_san")
IDS = list(range(12)) + [(1 << 32) - 6 + i for i in range(12)]


def pin_to_run_instance(cfg, row, depth, events, summary):
    """The restated loop against the unmodified run_instance on this row: the
    final result, digests and acceptor records, and every step's last "after"
    of each actor against oracle_trace's end-of-step record."""
    recs, res = SO.oracle_trace(cfg, row, depth)
    dv, dt, rounds, flags, steps, accs = summary
    assert (dv, dt, rounds, steps) == (res.decided_val, res.decided_ticket, res.rounds, res.steps)
    mask = R.F_PANIC | R.F_STEP_CAP | R.F_QUEUE_OVERFLOW
    assert flags & mask == res.flags & mask
    assert [EO._acc_after(a) for a in accs] == [EO._acc_after(a) for a in res.acceptors]
    by_step = {r["step"]: r for r in recs}
    for s, (acc, prop) in EO.last_after(EO.pack(events), cfg.n_acceptors, cfg.n_proposers).items():
        r = by_step[s]
        for a, st in acc.items():
            assert st == tuple(r["acc"][a]) + (r["digest"][a],), (s, a)
        for p, st in prop.items():
            assert st == tuple(r["prop"][p]), (s, p)
    # (a step without events changes nothing: the trace's own tests say so)
    return res


def check_row(cfg, row, depth, ev):
    """ev (the host lane's events of an OK row) equals the pinned event oracle's, byte for byte."""
    oe, summary = EO.oracle_events(cfg, row, depth)
    pin_to_run_instance(cfg, row, depth, oe, summary)
    want = EO.pack(oe)
    if want.tobytes() != ev.tobytes():
        wl, gl = pxb.event_lines(want), pxb.event_lines(ev)
        i = next((j for j in range(min(len(want), len(ev))) if want[j].tobytes() != ev[j].tobytes()), min(len(wl), len(gl)))
        raise AssertionError("event %d of %d / %d:\n oracle %s %s\n host   %s %s" % (
            i, len(want), len(ev), wl[i:i + 1], want[i:i + 1], gl[i:i + 1], ev[i:i + 1]))
    return want


# ---- 1. layout, symbols, validation ----------------------------------------------
def test_event_layout_and_symbols(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "paxos_batch.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(pxb_trace_event), offsetof(pxb_trace_event, step),
         offsetof(pxb_trace_event, actor), offsetof(pxb_trace_event, index), offsetof(pxb_trace_event, peer),
         offsetof(pxb_trace_event, fate), offsetof(pxb_trace_event, n_out), offsetof(pxb_trace_event, reserved),
         offsetof(pxb_trace_event, in), offsetof(pxb_trace_event, out), offsetof(pxb_trace_event, after),
         PXB_ABI_VERSION);
  printf("%zu %zu %u %u %u %u %u %u\n", offsetof(pxb_trace_event, after.acc.log_digest),
         offsetof(pxb_trace_event, after.prop.pending), PXB_EVT_ACCEPTOR, PXB_EVT_PROPOSER, PXB_EVT_HANDLED,
         PXB_EVT_DISCARDED_DEAD, PXB_EVT_DISCARDED_ISOL, PXB_EVT_PEER_TICK);
  return 0;
}'''
    tmp = str(tmp_path / "pxb_event_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(EO.ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [96, 0, 4, 5, 6, 7, 8, 12, 16, 32, 64, 5, 80, 92, 0, 1, 0, 1, 2, 255]
    dt = pxb.event_dtype()
    assert dt.itemsize == 96 == C.sizeof(pxb.pxb_trace_event) and pxb.ABI_VERSION == 5
    assert [dt.fields[k][1] for k in ("step", "actor", "index", "peer", "fate", "n_out", "reserved", "in", "out",
                                      "after")] == [0, 4, 5, 6, 7, 8, 12, 16, 32, 64]
    assert pxb.pxb_trace_event.after.offset == 64 and pxb.pxb_trace_event.in_.offset == 16
    lib_ = pxb.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_trace_events", "pxb_trace_events_device"):
        assert " T %s\n" % name in out and hasattr(lib_, name)


def test_event_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call; a valid call is
    PXB_E_NODEV without a GPU.  The host build refuses the same calls."""
    import torch
    L = pxb.load()
    cfg = pxb.CONFIGS[3]
    depth = 4
    rows = pxb.scripts_empty(cfg, range(8), depth)
    offs = np.zeros(9, np.uint64)
    ev = np.zeros(4, pxb.event_dtype())
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def calls(cfg_, rows_p=P(rows), count=8, depth_=depth, sel=None, ev_p=None, cap=0, offs_p=P(offs), flags=0):
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        if c is not None:
            c.flags |= flags
        cp = C.byref(c) if c is not None else None
        sp = C.byref(sel) if sel is not None else None
        return [L.pxb_trace_events(cp, rows_p, count, depth_, sp, ev_p, cap, offs_p, None, None, None),
                L.pxb_trace_events_device(cp, rows_p, count, depth_, sp, ev_p, cap, offs_p, None, None, None, None)]

    inval = [pxb.PXB_E_INVAL] * 2
    assert calls(None) == inval
    assert calls(cfg, rows_p=None) == inval
    assert calls(cfg, offs_p=None) == inval
    assert calls(cfg, depth_=4097) == inval
    assert calls(cfg, count=(1 << 30) + 1) == inval
    assert calls(cfg, sel=pxb.pxb_trace_sel(0, SO.U32, 0, 1)) == inval        # reserved
    assert calls(cfg, sel=pxb.pxb_trace_sel(0, SO.U32, 3, 0)) == inval        # a tail
    assert calls(cfg, cap=4) == inval                                         # no events, capacity > 0
    assert calls(cfg, flags=pxb.CFG_TRACE_PRODUCTION) == inval
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=10),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=4096),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9)):
        assert calls(bad, ev_p=P(ev), cap=4) == inval, bad
    # the device form: events 16-byte aligned (an INVAL before any device call)
    c = cfg.to_c(0, 1)
    raw = np.zeros(4 * 96 + 32, np.uint8)
    off = (-raw.ctypes.data) % 16 + 8
    assert L.pxb_trace_events_device(C.byref(c), P(rows), 8, depth, None, C.c_void_p(raw.ctypes.data + off), 4, P(offs),
                                     None, None, None, None) == pxb.PXB_E_INVAL
    if not torch.cuda.is_available():
        nodev = [pxb.PXB_E_NODEV] * 2
        assert calls(cfg, ev_p=P(ev), cap=4) == nodev
        assert calls(cfg, rows_p=None, count=0) == nodev
        with pytest.raises(pxb.PaxosError):
            pxb.trace_events(cfg, rows, depth)
        with pytest.raises(pxb.PaxosError):
            pxb.trace_events_ids(cfg, [1, 2])
    # the host build
    for kw in ({"sel": (0, SO.U32, 3, 0)}, {"sel": (0, SO.U32, 0, 1)}, {"cflags": pxb.CFG_TRACE_PRODUCTION}):
        assert EO.host_events(cfg, rows, depth, **kw)[0] == pxb.PXB_E_INVAL
    with pytest.raises(ValueError, match="required"):
        pxb.trace_events_device(cfg, None, 0, 4, None)
    with pytest.raises(ValueError, match="d_events"):
        pxb.trace_events_device(cfg, None, 0, 4, np.zeros(1, np.int64), None, 4)


# ---- 2. the step KATs ---------------------------------------------------------------
KATS = SO.kat_cases()


@pytest.mark.parametrize("case,cfg,row,depth", KATS, ids=[k[0]["name"] for k in KATS])
def test_step_kats_events_equal_the_event_oracle(case, cfg, row, depth):
    """S1-S8 as explicit scripts (S2's panic, S4 / S5 in log mode): the host
    lane's events are the pinned oracle's, byte for byte; results and status are
    the scripted run's."""
    rc, ev, offs, st, res, total = EO.host_events(cfg, row, depth)
    assert rc == 0 and st[0] == pxb.TRACE_OK and total == len(ev) == offs[1] and offs[0] == 0
    want = check_row(cfg, row, depth, ev)
    o = SO.host_run(cfg, row, depth)
    assert (res == o["res"]).all() and (st == o["status"]).all()
    assert (want["reserved"] == 0).all() and len(ev) > 0
    if case["name"].startswith("S2"):                    # the panic: a dead acceptor, and what it then discards
        dead = ev[(ev["actor"] == pxb.EVT_ACCEPTOR) & (ev["after"][:, 3] >> 31 == 1)]
        assert len(dead) >= 1 and int(res[0][3]) & pxb.F_PANIC
        assert (ev["fate"] == pxb.EVT_DISCARDED_ISOL).any()
    if cfg.n_ticks > 1:
        assert (ev[ev["peer"] == pxb.EVT_PEER_TICK]["step"].tolist() == [0, 6])


# ---- 3. random overrides --------------------------------------------------------------
def _c(**kw):
    return pxb.Config(**dict(dict(seed=0xE7E27, loss_ppm=100000, skew_max=3, step_cap=96), **kw))


RANDOM = {
    "p1n3-w8": (_c(n_proposers=1, n_acceptors=3, delay_max=4), 16, 11),
    "p2n3-w8": (_c(n_proposers=2, n_acceptors=3, delay_max=4), 16, 12),
    "p2n5-w16": (_c(n_proposers=2, n_acceptors=5, delay_max=15), 16, 13),
    "p3n9-w16": (_c(n_proposers=3, n_acceptors=9, delay_max=15, loss_ppm=50000), 16, 14),
    "p3n9-w8": (_c(n_proposers=3, n_acceptors=9, delay_max=4, loss_ppm=50000), 16, 15),
    "p1n3-w16": (_c(n_proposers=1, n_acceptors=3, delay_max=15), 16, 16),
    "log-p2n5": (dataclasses.replace(pxb.LOG_FAULTY_CONFIG, step_cap=96), 16, 17),
    "randomize-p3n3": (_c(n_proposers=3, n_acceptors=3, delay_max=4, randomize=True, crash_ppm=200000,
                          crash_len_max=8, crash_start_max=8), 16, 18),
    "windows-p2n5": (_c(n_proposers=2, n_acceptors=5, delay_max=4, crash_ppm=400000, crash_len_max=8,
                        crash_start_max=8), 16, 19),
}
_random = {}


def random_case(name):
    """(cfg, rows, depth, the host lane's outputs), once per config."""
    if name not in _random:
        cfg, depth, seed = RANDOM[name]
        rows = SO.random_overrides(cfg, IDS, depth, seed=seed)
        _random[name] = (cfg, rows, depth, EO.host_events(cfg, rows, depth))
    return _random[name]


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_overrides_events_equal_the_event_oracle(name):
    cfg, rows, depth, (rc, ev, offs, st, res, total) = random_case(name)
    assert rc == 0 and total == offs[-1] == len(ev)
    o = SO.host_run(cfg, rows, depth)
    assert (st == o["status"]).all() and (res == o["res"]).all()
    bailed = int((st == pxb.TRACE_BAILED).sum())
    assert bailed <= 0.10 * len(rows), "%d of %d rows bail" % (bailed, len(rows))
    for i in range(len(rows)):
        mine = ev[int(offs[i]):int(offs[i + 1])]
        if st[i] != pxb.TRACE_OK:                           # (bailed rows: the status only)
            assert st[i] == pxb.TRACE_BAILED and len(mine) == 0 and not res[i].any()
            continue
        check_row(cfg, rows[i], depth, mine)


# ---- 4. the hand-derived fixtures ------------------------------------------------------
FX = json.load(open(os.path.join(HERE, "golden", "kat_events.json")))


def fixture_row(case):
    cfg = pxb.Config(**FX["config"])
    depth = FX["depth"]
    rows = pxb.scripts_empty(cfg, [12345], depth)
    pxb.script_n_proposers(rows)[0] = 1
    pxb.script_skews(rows)[0] = 0
    pxb.script_windows(cfg, rows)[0] = case["windows"]
    pxb.script_links(cfg, rows, depth)[0] = 1
    return cfg, rows[0], depth


def fixture_events(case):
    return EO.pack([dict(e, **{"in": tuple(e["in"]), "out": [tuple(m) for m in e["out"]],
                               "after": tuple(e["after"]) + (0,) * (8 - len(e["after"]))}) for e in case["events"]])


@pytest.mark.parametrize("case", FX["cases"], ids=[c["name"] for c in FX["cases"]])
def test_hand_derived_events(case):
    cfg, row, depth = fixture_row(case)
    want = fixture_events(case)
    rc, ev, offs, st, res, total = EO.host_events(cfg, row, depth)
    assert rc == 0 and st[0] == pxb.TRACE_OK
    assert pxb.event_lines(ev) == pxb.event_lines(want)
    assert ev.tobytes() == want.tobytes()
    oe, summary = EO.oracle_events(cfg, row, depth)
    pin_to_run_instance(cfg, row, depth, oe, summary)
    assert EO.pack(oe).tobytes() == want.tobytes()
    assert len(want) == (16 if case["name"].startswith("E1") else 15)
    assert pxb.event_lines(want[7:8]) == [
        "s=3 acc0 <- p0 Propose(1,c1.1) -> Round2Success | t_max=1 store=(1,c1.1) log=0"
        if case["name"].startswith("E1") else "s=3 acc1 <- p0 Propose(1,c1.1) -> HaveTicket(0) | t_max=0 store=- log=0"]


# ---- 5. the message chart -----------------------------------------------------------------
def chart_invariants(cfg, row, depth, mine, sent, in_flight):
    """pxb.message_chart of one explicit OK row whose links consumed at most
    `depth` entries: sends per link are the run's `sent`; each matched delivery's
    `in` is its send's payload, at least a step later; every delivery has its
    send; the unmatched non-lost sends are the last step record's in_flight."""
    chart = pxb.message_chart(cfg, row, depth, mine)
    per_link = np.zeros_like(sent)
    np.add.at(per_link, (chart["dirn"], chart["p"], chart["a"]), 1)
    assert (per_link == sent).all()
    lk = pxb.script_links(cfg, row[None, :], depth)[0]
    deliveries = {}
    for e in mine:
        if e["actor"] == pxb.EVT_ACCEPTOR:
            deliveries.setdefault((0, int(e["peer"]), int(e["index"])), []).append(e)
        elif e["peer"] != pxb.EVT_PEER_TICK:
            deliveries.setdefault((1, int(e["index"]), int(e["peer"])), []).append(e)
    taken, seqs = {}, {}
    for m in chart:
        link = (int(m["dirn"]), int(m["p"]), int(m["a"]))
        assert m["seq"] == seqs.get(link, 0)
        seqs[link] = int(m["seq"]) + 1
        assert (m["fate"] == pxb.CHART_LOST) == (lk[link + (int(m["seq"]),)] == 0)
        if m["fate"] in (pxb.CHART_HANDLED, pxb.CHART_DISCARDED):
            j = taken.get(link, 0)
            taken[link] = j + 1
            e = deliveries[link][j]
            assert (e["in"]["kind"], e["in"]["x"], e["in"]["y"], e["in"]["z"]) == (m["kind"], m["x"], m["y"], m["z"])
            assert m["delivered_step"] == e["step"] >= m["sent_step"] + 1
            assert (m["fate"] == pxb.CHART_HANDLED) == (e["fate"] == pxb.EVT_HANDLED)
        else:
            assert m["delivered_step"] == -1
    assert all(taken.get(k, 0) == len(v) for k, v in deliveries.items())
    assert int((chart["fate"] == pxb.CHART_IN_FLIGHT).sum()) == in_flight
    return chart


def chart_rows(cfg, rows, depth, ev, offs, st):
    """chart_invariants on every OK row of a call that is explicit (no keep byte)
    and consumed at most `depth` entries a link; a row with a keep byte that a
    send reads is refused.  Returns (rows checked, rows that had to be)."""
    o = SO.host_run(cfg, rows, depth, capacity=cfg.step_cap + 1)
    checked = due = 0
    for i in range(len(rows)):
        if st[i] != pxb.TRACE_OK:
            continue
        mine = ev[int(offs[i]):int(offs[i + 1])]
        lk = pxb.script_links(cfg, rows[i:i + 1], depth)[0]
        sent = o["sent"][i]
        consumed = np.arange(depth) < np.minimum(sent, depth)[..., None]
        if int(sent.max()) > depth or (lk[consumed] == 0xFF).any():    # a send reads a keep entry: refused
            with pytest.raises(ValueError, match="keep"):
                pxb.message_chart(cfg, rows[i], depth, mine)
            continue
        due += 1
        last = pxb.trace_records(o["rec"][i][:o["n_kept"][i]])[-1]
        chart_invariants(cfg, rows[i], depth, mine, o["sent"][i], int(last["in_flight"]))
        checked += 1
    return checked, due


@pytest.mark.parametrize("name", list(RANDOM))
def test_message_chart_invariants(name):
    """Every OK row of every random config that can be charted (explicit, within
    the depth) is; rows that start from all-keep rows are refused."""
    cfg, rows, depth, (rc, ev, offs, st, res, total) = random_case(name)
    checked, due = chart_rows(cfg, rows, depth, ev, offs, st)
    assert checked == due >= 1          # (every chartable row, and the population is not empty)


@pytest.mark.parametrize("case,cfg,row,depth", KATS, ids=[k[0]["name"] for k in KATS])
def test_message_chart_invariants_on_the_step_kats(case, cfg, row, depth):
    rc, ev, offs, st, res, total = EO.host_events(cfg, row, depth)
    assert chart_rows(cfg, row[None, :], depth, ev, offs, st) == (1, 1)


# ---- 6. the window and the capacity rule ----------------------------------------------------
def test_window_selection_and_capacity_rule():
    cfg, rows, depth, (rc, ev, offs, st, res, total) = random_case("p2n3-w8")
    n = len(rows)
    # a window: exactly the events of those steps, the rows' results unchanged
    rc, wev, woffs, wst, wres, wtotal = EO.host_events(cfg, rows, depth, sel=(2, 5, 0, 0))
    assert rc == 0 and (wst == st).all() and (wres == res).all()
    for i in range(n):
        mine = ev[int(offs[i]):int(offs[i + 1])]
        keep = mine[(mine["step"] >= 2) & (mine["step"] <= 5)]
        assert wev[int(woffs[i]):int(woffs[i + 1])].tobytes() == keep.tobytes()
    # capacities that cut inside a step, inside a row and between rows: the prefix, the guard intact,
    # the offsets, status and results those of the full call
    steps = ev["step"]
    inside = next(k for k in range(int(offs[3]) + 1, int(offs[4])) if steps[k] == steps[k - 1] and
                  ev["actor"][k - 1] != ev["actor"][k])
    for cap in (1, inside, int(offs[5]), int(offs[7]) + 1, total - 1, total, total + 5):
        rc, cev, coffs, cst, cres, ctotal = EO.host_events(cfg, rows, depth, capacity=cap, pad=3)
        assert rc == 0 and ctotal == total and (coffs == offs).all() and (cst == st).all() and (cres == res).all()
        m = min(cap, total)
        assert cev[:m].tobytes() == ev[:m].tobytes(), cap
        assert (cev[m:].view(np.uint8) == EO.GUARD).all(), cap
    # the sizing call
    rc, sev, soffs, sst, sres, stotal = EO.host_events(cfg, rows, depth, capacity=0, pad=2)
    assert rc == 0 and stotal == total and (soffs == offs).all() and (sev.view(np.uint8) == EO.GUARD).all()
    # count == 0
    rc, zev, zoffs, zst, zres, ztotal = EO.host_events(cfg, rows[:0], depth)
    assert rc == 0 and ztotal == 0 and zoffs.tolist() == [0] and len(zev) == 0
    # a bad row between good ones
    bad = rows.copy()
    bad[4, 9] = 1
    rc, bev, boffs, bst, bres, btotal = EO.host_events(cfg, bad, depth)
    assert rc == 0 and bst[4] == pxb.SCRIPT_BAD and boffs[5] == boffs[4] and not bres[4].any()
    for i in range(n):
        if i != 4:
            assert bst[i] == st[i] and (bres[i] == res[i]).all()
            assert bev[int(boffs[i]):int(boffs[i + 1])].tobytes() == ev[int(offs[i]):int(offs[i + 1])].tobytes()


def test_a_row_repeated_gives_its_events_again():
    cfg, rows, depth, (rc, ev, offs, st, res, total) = random_case("p2n5-w16")
    i = next(j for j in range(len(rows)) if st[j] == pxb.TRACE_OK and offs[j + 1] - offs[j] > 8)
    rc, ev2, offs2, st2, res2, _ = EO.host_events(cfg, np.stack([rows[i]] * 3), depth)
    one = ev[int(offs[i]):int(offs[i + 1])].tobytes()
    assert rc == 0 and ev2.tobytes() == one * 3 and (np.diff(offs2) == len(one) // 96).all()


# ---- 7. one stand-alone sanitizer program -------------------------------------------------
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_EVENTS_HOST_MAIN",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
             "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_events_core_sanitized():
    """events_host.cpp with its own main (the KATs' shapes: N = 3 on the 8-step
    wheel) under AddressSanitizer + UBSan, as a subprocess per KAT case, with a
    capacity that cuts the events and every buffer exactly as large as the call
    may write.  Exit status 0, and the output equals the unsanitized library's."""
    if EO.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([EO.HIPCC, *SAN_FLAGS, "-o", tmp, EO.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    e = dict(os.environ)
    e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    with tempfile.TemporaryDirectory() as td:
        for case, cfg, row, depth in KATS:
            rows = np.stack([row, row])
            rc, ev, offs, st, res, total = EO.host_events(cfg, rows, depth)
            cap = total - 3
            c = cfg.to_c(0, 1)
            inp, out = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
            with open(inp, "wb") as f:
                f.write(bytes(c) + struct.pack("<IIIQQ", depth, 0, SO.U32, 2, cap) + rows.tobytes())
            p = subprocess.run([EXE, inp, out], capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode == 0, "sanitized run failed (rc %d): %s" % (p.returncode, p.stderr[-4000:])
            raw = open(out, "rb").read()
            assert struct.unpack_from("<Q", raw, 0)[0] == total
            assert raw[8:32] == offs.tobytes() and raw[32:40] == st.tobytes() and raw[40:72] == res.tobytes()
            assert raw[72:] == ev[:cap].tobytes(), case["name"]
