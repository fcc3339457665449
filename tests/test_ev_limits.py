"""The per-lane state machine (csrc/paxos_ev.h) at the limits of its packed
fields, on the CPU: the cells of tests/ev_limits.py through the host build of
the lane.

Two hand-off causes had no pinned instance: EVB_RSEQ, a link's reply seq at the
top of its field, and EVB_LOG, an acceptor's log length at A_LEN_MAX.  And no
test ran the fields that share words -- 12-bit tickets, the 16-bit broadcast
counters, the reference nibbles -- over the longest run the lane is eligible
for, 4,095 steps.  Here, per cell: the routing gives the cell the layouts it
claims; the host lane equals the oracle on every instance it keeps
(test_ev_matrix.expected_handoffs, which also records the hand-offs that
tests/test_ev_limits_gpu.py holds the device to); every hand-off shows the
cause the cell exists for (the header's host-only probes, read by
tests/native/ev_limits_host.cpp); pinned ids stand on each limit and one short
of it; and the high-water mark of every narrow field over the 4,095-step cells
stays inside the field.

Host lane, 4,096 instances a cell (hand-offs by cause):
  A511   0; 4,053 instances end with a reply seq of 255
  A512   4,053 RSEQ (the other 43 decide within 22 steps)
  S512   180 RSEQ; 839 kept instances end with a reply seq of 255
  B      layout 9: 133 RSEQ, layout 8: 0      BHI  layout 9: 127 RSEQ, layout 8: 0
  C      0 (reply seq <= 242)                 C0   layout 9: 1 RSEQ (id 90), layout 8: 0
  D      37 LOG; 34 kept instances end with a full log length, 31
  E      0; 3,334 instances run all 4,095 steps
  F      200: 191 RFIFO, 9 QFIFO
  T512   layout 7: 59 (37 RFIFO, 22 POOL), layout 6: 2 of them
  T512HI layout 7: 53 (32 RFIFO, 21 POOL), layout 6: 3 of them
  K1023  (layout 3 forced) 0; 4,063 instances end with a reply seq of 511
  K1024  4,063 RSEQ
High-water marks over D, E and F: test_headroom_at_4095_steps.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ev_limits as EL
import oracle_c
import pxb
from test_ev_matrix import expected_handoffs
from test_route_plan import plan

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ev_limits_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libev_limits_host.so")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")] + [
                    os.path.join(HERE, "..", "include", "paxos_batch.h")]
# a record's words (ev_limits_host.cpp)
(LW_RES, LW_ROUNDS, LW_EXECS, LW_MSGS, LW_CANON, LW_BAILED, LW_PROBES, LW_ITERS, LW_FLAGS, LW_STEPS, LW_BAIL_AT_INIT,
 LW_HW_TICKET, LW_HW_NSP, LW_HW_BCP, LW_HW_ACKS, LW_HW_REF, LW_HW_LOG, LW_HW_RSEQ, LW_N) = (0, *range(4, 22))
# the header's bail causes (paxos_ev.h)
EVB = dict(RING=1 << 16, RFIFO=1 << 17, POOL=1 << 18, QFIFO=1 << 19, LOG=1 << 20, RSEQ=1 << 21)
_TWO = {(9, 8): "LG2", (7, 6): "TIGHT"}
_ALL = EL.CELLS + EL.TIGHT + EL.HOST_ONLY
_lib = None
_recs = {}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC",
                            "-shared", "-o", tmp, SRC], check=True)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
        assert _lib.ev_limits_words() == LW_N
    return _lib


def records(name, layout=None):
    """The driver's records of a cell's N_INST instances on `layout` (default:
    its first stage's), row i the instance cell.first + i: run once, read-only."""
    cell = EL.BY_ID[name]
    layout = cell.layout1 if layout is None else layout
    if (name, layout) not in _recs:
        ids = np.arange(EL.N_INST, dtype=np.uint32)
        rec = np.zeros((len(ids), LW_N + cell.N), np.uint32)
        c = cell.cfg.to_c(cell.first, EL.N_INST)
        rc = lib().ev_limits_run(C.byref(c), layout, C.c_void_p(ids.ctypes.data), len(ids), C.c_void_p(rec.ctypes.data))
        assert rc == 0, "ev_limits_run rc=%d" % rc
        rec.setflags(write=False)
        _recs[name, layout] = rec
    return _recs[name, layout]


def causes(rec):
    """{cause: hand-offs that show it} of a record array."""
    b = rec[rec[:, LW_BAILED] == 1]
    return {k: int((b[:, LW_PROBES] & v != 0).sum()) for k, v in EVB.items() if (b[:, LW_PROBES] & v).any()}


def _equals_the_oracle(cell, i, r):
    """Instance cell.first + i, which the lane kept: the driver's record against the oracle."""
    g = cell.first + i
    eres, edig, _, cnt = oracle_c.run_cpu(cell.cfg, g, 1)
    assert not r[LW_BAILED], g
    assert list(r[LW_RES:LW_RES + 4]) == list(eres[0]), "instance %d: result words" % g
    assert list(r[LW_N:LW_N + cell.N]) == list(edig[0]), "instance %d: digests" % g
    got = dict(rounds=int(r[LW_ROUNDS]), executes=int(r[LW_EXECS]), messages=int(r[LW_MSGS]),
               canon_bytes=int(r[LW_CANON]), steps=int(r[LW_STEPS]),
               undecided=int(bool(r[LW_FLAGS] & pxb.F_UNDECIDED)), step_cap=int(bool(r[LW_FLAGS] & pxb.F_STEP_CAP)),
               divergence=int(bool(r[LW_FLAGS] & pxb.F_LOG_DIVERGENCE)), panic=int(bool(r[LW_FLAGS] & pxb.F_PANIC)))
    assert got == {k: cnt[k] for k in got}, "instance %d" % g


@pytest.mark.parametrize("cell", EL.CELLS + EL.TIGHT, ids=[EL.cell_id(c) for c in EL.CELLS + EL.TIGHT])
def test_routing(cell):
    """The routing gives the cell the layouts it claims, so the GPU test runs
    the shapes the host lane ran here."""
    p = plan(cell.cfg)
    assert p["kind"] == "EV"
    if cell.layout2 is None:
        assert (p["two"], p["second"], "first" in p) == ("NONE", (cell.P, cell.N, cell.layout1), False), p
    else:
        assert (p["two"], p["first"], p["second"]) == (
            _TWO[cell.layout1, cell.layout2], (cell.P, cell.N, cell.layout1), (cell.P, cell.N, cell.layout2)), p


@pytest.mark.parametrize("cell", EL.HOST_ONLY, ids=[EL.cell_id(c) for c in EL.HOST_ONLY])
def test_routing_cannot_reach_the_compact_limit(cell):
    """The 9-bit reply seq needs more than 512 steps, which the routing gives
    to layout 0: the compact cells run on the host lane only."""
    p = plan(cell.cfg)
    assert cell.cfg.step_cap > 512 and (p["kind"], p["two"], p["second"]) == ("EV", "NONE", (cell.P, cell.N, 0)), p


@pytest.mark.parametrize("cell", _ALL, ids=[EL.cell_id(c) for c in _ALL])
def test_oracle_and_cause(cell):
    name = EL.cell_id(cell)
    # the host lane equals the oracle (results, digests, acceptor records,
    # totals) on every instance it does not hand on
    h1, h2 = expected_handoffs(cell, verify=True)
    assert (len(h1), len(h2)) == EL.HANDOFFS[name]          # (what the GPU test holds the device to)
    rec = records(name)
    # the driver here hands on what tests/native/ev_host.cpp's does
    assert np.array_equal(np.nonzero(rec[:, LW_BAILED])[0], h1)
    assert not rec[:, LW_BAIL_AT_INIT].any()
    by = causes(rec)
    kept = rec[rec[:, LW_BAILED] == 0]
    print("%s: %d first hand-offs %s, %d second; kept: reply seq <= %d, log length <= %d" % (
        name, len(h1), by, len(h2), kept[:, LW_HW_RSEQ].max(), kept[:, LW_HW_LOG].max()))
    if name in EL.NONE:
        assert len(h1) == 0
    elif name in EL.CAUSE:
        # the cell is there for one cause: it is present, and every hand-off shows it alone
        assert len(h1) > 0 and by == {EL.CAUSE[name]: len(h1)}, by
    if cell.layout2 is not None:
        r2 = records(name, cell.layout2)
        assert np.array_equal(np.intersect1d(h1, np.nonzero(r2[:, LW_BAILED])[0]), h2)
        if cell.layout2 == 8:
            # the second stage's 16-bit reply seqs take what the byte could not
            assert len(h2) == 0 and (len(h1) == 0 or int(r2[h1, LW_HW_RSEQ].min()) >= 256)
    limit = {"A511": 255, "K1023": 511}.get(name)
    if limit is not None:
        # the limit reached and not crossed: nothing handed on, reply seqs at the top of the field
        assert len(h1) == 0 and int(rec[:, LW_HW_RSEQ].max()) == limit
        assert int((rec[:, LW_HW_RSEQ] == limit).sum()) > EL.N_INST // 2
    if name == "S512":
        # the straddle: neither none nor nearly all, and kept instances that end on the limit
        assert EL.N_INST // 64 < len(h1) < EL.N_INST // 4
        assert int((kept[:, LW_HW_RSEQ] == 255).sum()) > EL.N_INST // 64
    if name == "D":
        assert int(kept[:, LW_HW_LOG].max()) == 31      # (a full 5-bit length is kept; the 32nd entry is not)
    if name == "E":
        assert len(h1) == 0 and int((rec[:, LW_STEPS] == 4095).sum()) > EL.N_INST // 2


# Pinned ids (offsets from the cell's first), chosen once with the driver over
# the cells' own instances.  Per cause and field width one id that is handed on,
# and one that ends on the last value the field holds -- one short of the
# hand-off -- which the lane keeps and which equals the oracle.
#   (cell, id, cause): handed on, showing that cause alone
HANDED_ON = [("A512", 0, "RSEQ"), ("S512", 97, "RSEQ"),          # layout 5
             ("B", 6, "RSEQ"), ("BHI", 39, "RSEQ"), ("C0", 90, "RSEQ"),   # layout 9
             ("D", 175, "LOG"),                                   # layout 0
             ("K1024", 0, "RSEQ")]                                # layout 3, forced
#   (cell, id, field, the field's high-water mark): kept
ONE_SHORT = [("A511", 0, LW_HW_RSEQ, 255), ("S512", 7, LW_HW_RSEQ, 255),   # layout 5: 255 replies on a link
             ("BHI", 1628, LW_HW_RSEQ, 255),                               # layout 9
             ("D", 74, LW_HW_LOG, 30),                                      # 30 log entries
             ("D", 47, LW_HW_LOG, 31),                                      # 31: the 5-bit length full, and kept
             ("K1024", 1599, LW_HW_RSEQ, 511)]                             # layout 3: 511 replies, to the step cap


@pytest.mark.parametrize("name,i,cause", HANDED_ON, ids=["%s-%d" % t[:2] for t in HANDED_ON])
def test_pinned_id_is_handed_on(name, i, cause):
    r = records(name)[i]
    assert r[LW_BAILED] and not r[LW_BAIL_AT_INIT], i
    assert int(r[LW_PROBES]) & sum(EVB.values()) == EVB[cause], hex(int(r[LW_PROBES]))


@pytest.mark.parametrize("name,i,field,value", ONE_SHORT, ids=["%s-%d" % t[:2] for t in ONE_SHORT])
def test_pinned_id_one_short_equals_the_oracle(name, i, field, value):
    r = records(name)[i]
    assert not r[LW_BAILED] and int(r[field]) == value, (i, int(r[field]))
    _equals_the_oracle(EL.BY_ID[name], i, r)


def test_every_limit_has_both_pins():
    """EVB_RSEQ on both byte layouts (5 and 9) and on the 9-bit one, EVB_LOG on
    layout 0: a handed-on id and a one-short id each."""
    on = {(EL.BY_ID[n].layout1, c) for n, _, c in HANDED_ON}
    short = {(EL.BY_ID[n].layout1, "LOG" if f == LW_HW_LOG else "RSEQ") for n, _, f, _ in ONE_SHORT}
    assert on == short == {(5, "RSEQ"), (9, "RSEQ"), (3, "RSEQ"), (0, "LOG")}


def test_headroom_at_4095_steps():
    """The limits that must be unreachable, over the 4,095-step cells D, E and
    F: every high-water mark stays below its field.  Tickets stay <= step_cap
    and a proposer broadcasts at most three times per ticket value, which is
    what lets the broadcast counters be 16-bit fields of one word
    (paxos_ev.h, "Per-proposer broadcast counters").

    Measured (host lane, kept instances; field limit):
               ticket  nsp    bcp    acks  ref nibble  log length  reply seq
      limit    4095    65535  65535  15    15          31          65534
    """
    worst = np.zeros(LW_N, np.int64)
    for name in EL.LONG:
        cell, rec = EL.BY_ID[name], records(name)
        kept = rec[rec[:, LW_BAILED] == 0]
        hw = kept[:, LW_HW_TICKET:LW_N].max(axis=0).astype(np.int64)
        print("%s: ticket %d nsp %d bcp %d acks %d ref %d log %d rseq %d; %d of %d at step 4095" % (
            name, *hw, int((kept[:, LW_STEPS] == 4095).sum()), len(kept)))
        assert int(kept[:, LW_STEPS].max()) == 4095         # (the cell does run to the cap)
        assert hw[LW_HW_TICKET - LW_HW_TICKET] < 4096 and hw[0] <= cell.cfg.step_cap
        assert hw[LW_HW_NSP - LW_HW_TICKET] < 65536 and hw[LW_HW_BCP - LW_HW_TICKET] < 65536
        # (the argument itself: three broadcasts per ticket value)
        assert hw[LW_HW_NSP - LW_HW_TICKET] < 3 * 4096 and hw[LW_HW_BCP - LW_HW_TICKET] < 3 * 4096
        assert hw[LW_HW_ACKS - LW_HW_TICKET] <= 15 and hw[LW_HW_ACKS - LW_HW_TICKET] <= cell.N // 2 + 1
        assert hw[LW_HW_REF - LW_HW_TICKET] <= 15
        assert hw[LW_HW_LOG - LW_HW_TICKET] <= 31
        assert hw[LW_HW_RSEQ - LW_HW_TICKET] < 65535
        worst[LW_HW_TICKET:] = np.maximum(worst[LW_HW_TICKET:], hw)
    print("D, E, F: ticket %d nsp %d bcp %d acks %d ref %d log %d rseq %d" % tuple(worst[LW_HW_TICKET:]))


# ---- the lane-kernel families at the log-length limit (no next stage: PXB_TRACE_BAILED) ----
_lane_d = {}


def lane_d_host():
    """Cell D's LANE_D_IDS through the host builds of the lane-kernel families'
    shape (tests/native/host_lane.h, the 8-step wheel): the ids, their
    extracted rows, the scripted lane's outputs, the batched trace's (status,
    result) at tail = 1, and the oracle's.  Computed once, read-only."""
    if not _lane_d:
        import script_oracle as SO
        from test_trace_batch_host import host_trace
        cell = EL.BY_ID["D"]
        ids = np.asarray(EL.LANE_D_IDS, np.uint64) + np.uint64(cell.first)
        rows = SO.host_extract(cell.cfg, ids, EL.LANE_DEPTH)
        h = SO.host_run(cell.cfg, rows, EL.LANE_DEPTH)
        t = [host_trace(cell.cfg, int(g), sel=(0, 0xFFFFFFFF, 1), capacity=1)[3:] for g in ids]
        tstatus = np.asarray([x[0] for x in t], np.uint32)
        tres = np.asarray([x[1] for x in t], np.uint32)
        ora = [oracle_c.run_cpu(cell.cfg, int(g), 1, want_acceptors=True)[:3] for g in ids]
        eres, edig, eacc = (np.concatenate([o[k] for o in ora]) for k in range(3))
        for a in (ids, rows, tstatus, tres, eres, edig, eacc, *h.values()):
            a.setflags(write=False)
        _lane_d.update(ids=ids, rows=rows, h=h, tstatus=tstatus, tres=tres, eres=eres, edig=edig, eacc=eacc)
    return _lane_d


def test_lane_families_at_the_log_limit():
    """The list holds D's hand-offs below 1,000; the families' 8-step-wheel
    shape ends exactly those with PXB_TRACE_BAILED (the same 5-bit log length,
    and none of the 128 overflows its FIFOs), every other row equals the
    oracle, and rows extracted at depth 64 carry the 4,095-step runs: past the
    depth an entry reads the row's own Philox stream (script_core.h)."""
    rec = records("D")
    handed = np.nonzero(rec[:1000, LW_BAILED])[0]
    assert handed.tolist() == EL.LANE_D_HANDED_ON and len(EL.LANE_D_IDS) == len(set(EL.LANE_D_IDS)) == 128
    d = lane_d_host()
    bailed = np.isin(EL.LANE_D_IDS, EL.LANE_D_HANDED_ON)
    want = np.where(bailed, pxb.TRACE_BAILED, pxb.TRACE_OK)
    assert np.array_equal(d["h"]["status"], want) and np.array_equal(d["tstatus"], want)
    ok = ~bailed
    assert int((d["eres"][ok][:, 3] >> 16).max()) == 4095      # (rows that run to the cap)
    assert int(d["h"]["sent"].max()) > EL.LANE_DEPTH            # (links that consume more than the depth)
    assert np.array_equal(d["h"]["res"][ok], d["eres"][ok]) and np.array_equal(d["h"]["dig"][ok], d["edig"][ok])
    assert np.array_equal(d["h"]["acc"][ok], d["eacc"][ok])
    assert np.array_equal(d["tres"][ok], d["eres"][ok])
