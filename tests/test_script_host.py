"""Scripted schedules (docs/SEMANTICS.md §10) without a GPU.

The scripted lane the kernels run (csrc/script_core.h over the per-lane state
machine and TraceLane) and the extract's per-entry function are compiled for
the HOST (tests/native/script_host.cpp) and checked against the unmodified
Python reference model driven through an adapter (tests/script_oracle.py), the
C-ABI boundary of the new entry points, pxb.shrink with the host runner, and
one stand-alone AddressSanitizer + UBSan program (its own main; nothing is
loaded into Python)."""
import ctypes as C
import dataclasses
import os
import subprocess
import tempfile

import numpy as np
import pytest

import paxos_ref as R
import pxb
import script_oracle as SO
from test_trace_batch_host import IDS, host_trace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(HERE, "native", "_build", "script_host_san")
CONFIGS = [3, 4, 5, 7]
OTHER_SEED = 0x0123456789ABCDEF
_explicit = {}


def explicit_rows(c, depth):
    """The Python builder's rows of IDS under config c at `depth`, built once at
    depth 64 (the link tables of a smaller depth are its first entries)."""
    cfg = pxb.CONFIGS[c]
    if c not in _explicit:
        _explicit[c] = SO.build_rows(cfg, IDS, 64)
    full = _explicit[c]
    if depth == 64:
        return full.copy()
    rows = pxb.scripts_empty(cfg, IDS, depth)
    rows[:, :pxb.script_links_off(cfg)] = full[:, :pxb.script_links_off(cfg)]
    pxb.script_links(cfg, rows, depth)[:] = pxb.script_links(cfg, full, 64)[..., :depth]
    return rows


# ---- 1. layout, symbols, validation ---------------------------------------------
def test_script_layout_and_symbols(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include <dlfcn.h>
#include "paxos_batch.h"
int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) return 3;
  uint64_t (*stride)(uint32_t, uint32_t, uint32_t) = (uint64_t (*)(uint32_t, uint32_t, uint32_t))dlsym(h, "pxb_script_stride");
  if (!stride || argc != 2) return 4;
  printf("%u %u %u %u %d\n", PXB_SCRIPT_MAX_DEPTH, PXB_SCRIPT_BAD, PXB_SCRIPT_KEEP8, PXB_SCRIPT_KEEP16, PXB_ABI_VERSION);
  /* the documented offsets: header 16, windows 4 N, links 2 P N depth, padded to 8 */
  printf("%llu %llu %llu %llu\n", (unsigned long long)stride(2, 5, 7), (unsigned long long)stride(3, 9, 4096),
         (unsigned long long)stride(1, 2, 0), (unsigned long long)stride(1, 2, 1));
  /* the field offsets: the row's head, the windows behind it, the link table behind those */
  printf("%zu %zu %zu %zu %zu %zu %u %u %u\n", sizeof(pxb_script_head), offsetof(pxb_script_head, base),
         offsetof(pxb_script_head, n_proposers), offsetof(pxb_script_head, reserved), offsetof(pxb_script_head, skew),
         sizeof(pxb_script_window), PXB_SCRIPT_WINDOWS_OFF, PXB_SCRIPT_LINKS_OFF(5), PXB_SCRIPT_LINKS_OFF(9));
  return 0;
}'''
    tmp = str(tmp_path / "pxb_script_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", tmp, tmp + ".c", "-ldl"], check=True)
    p = subprocess.run([tmp, pxb.LIB_PATH], capture_output=True, text=True)
    assert p.returncode == 0, p.returncode
    got = [int(x) for x in p.stdout.split()]
    assert got[:5] == [pxb.SCRIPT_MAX_DEPTH, pxb.SCRIPT_BAD, 0xFF, 0xFFFF, 5] and pxb.ABI_VERSION == 5
    assert got[5:9] == [16 + 20 + 140, 16 + 36 + 2 * 27 * 4096 + 4, 24, 28 + 4]    # (+ the padding to 8)
    assert got[9:] == [16, 0, 8, 9, 10, 4, 16, 36, 52]
    assert (pxb.SCRIPT_HDR, pxb.script_links_off(pxb.CONFIGS[3]), pxb.script_links_off(pxb.CONFIGS[5])) == (16, 36, 52)
    lib_ = pxb.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pxb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pxb_script_stride", "pxb_schedule_extract", "pxb_schedule_extract_device", "pxb_run_scripted",
                 "pxb_run_scripted_device", "pxb_trace_scripted", "pxb_trace_scripted_device"):
        assert " T %s\n" % name in out and hasattr(lib_, name)
    # the stride: library, host build and Python agree; 8-byte aligned; the documented offsets
    for P in (1, 2, 3):
        for N in (2, 5, 9):
            for depth in (0, 1, 7, 64, 4096):
                cfg = pxb.Config(seed=1, n_proposers=P, n_acceptors=N)
                s = lib_.pxb_script_stride(P, N, depth)
                assert s == pxb.script_stride(cfg, depth) == SO.lib().script_host_stride(P, N, depth)
                assert s % 8 == 0 and 0 <= s - (16 + 4 * N + 2 * P * N * depth) < 8
    cfg = pxb.CONFIGS[3]
    rows = pxb.scripts_empty(cfg, [0x1122334455667788, 5], 7)
    assert rows[0, :8].tolist() == [0x88, 0x77, 0x66, 0x55, 0x44, 0x33, 0x22, 0x11] and rows[0, 8] == 0 and rows[0, 9] == 0
    pxb.script_skews(rows)[1] = [1, 2, 0x0304]
    pxb.script_windows(cfg, rows)[1, 4] = [5, 0x0607]
    pxb.script_links(cfg, rows, 7)[1, 1, 1, 4, 6] = 9
    r = rows[1]
    assert r[10:16].tolist() == [1, 0, 2, 0, 4, 3] and r[16 + 16:16 + 20].tolist() == [5, 0, 7, 6]
    assert r[36 + ((1 * 2 + 1) * 5 + 4) * 7 + 6] == 9 and (rows[0, 10:36 + 140] == 0xFF).all()
    assert (rows[:, 36 + 140:] == 0).all()


def test_script_validation_without_a_device_call():
    """Every PXB_E_INVAL case is decided before any device call (so on every
    host); a valid call is PXB_E_NODEV without a GPU."""
    import torch
    L = pxb.load()
    cfg = pxb.CONFIGS[3]
    depth = 4
    rows = pxb.scripts_empty(cfg, range(8), depth)
    ids = np.arange(8, dtype=np.uint64)
    offs = np.zeros(9, np.uint64)
    rec = np.zeros((4, pxb.TRACE_WORDS), np.uint32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    ALL, EXTRACT, TRACE = range(6), (0, 1), (4, 5)

    def calls(which, cfg_, rows_p=P(rows), count=8, depth_=depth, sel=None, rec_p=None, cap=0, offs_p=P(offs),
              ids_p=P(ids)):
        """The entry points `which` only (0, 1: extract, 2, 3: run, 4, 5: trace; host form, device form).  A
        case names exactly those it makes invalid: the host arrays here stand in for device buffers, so a
        call that is valid must never be made where a GPU would run it."""
        c = cfg_.to_c(0, 1) if cfg_ is not None else None
        cp = C.byref(c) if c is not None else None
        sp = C.byref(sel) if sel is not None else None
        fns = (lambda: L.pxb_schedule_extract(cp, ids_p, count, depth_, rows_p),
               lambda: L.pxb_schedule_extract_device(cp, ids_p, count, depth_, rows_p, None),
               lambda: L.pxb_run_scripted(cp, rows_p, count, depth_, None, None, None, None, None),
               lambda: L.pxb_run_scripted_device(cp, rows_p, count, depth_, None, None, None, None, None, None),
               lambda: L.pxb_trace_scripted(cp, rows_p, count, depth_, sp, rec_p, cap, offs_p, None, None, None),
               lambda: L.pxb_trace_scripted_device(cp, rows_p, count, depth_, sp, rec_p, cap, offs_p, None, None, None))
        return [fns[i]() for i in which]

    def inval(which, *a, **kw):
        got = calls(which, *a, **kw)
        return len(got) == len(which) and all(rc == pxb.PXB_E_INVAL for rc in got)
    assert inval(ALL, None)                                              # null cfg
    assert inval(ALL, cfg, rows_p=None)                                  # null rows, count > 0
    assert inval(EXTRACT, cfg, ids_p=None)                               # null ids (the extract's input)
    assert inval(TRACE, cfg, offs_p=None)                                # null offsets
    assert inval(ALL, cfg, depth_=4097)                                  # depth > 4096
    assert inval(ALL, cfg, count=(1 << 30) + 1)                          # count > 2^30
    assert inval(TRACE, cfg, sel=pxb.pxb_trace_sel(0, SO.U32, 0, 1))     # reserved
    assert inval(TRACE, cfg, cap=4)                                      # no records, capacity > 0
    c = cfg.to_c(0, 1)
    c.flags |= pxb.CFG_TRACE_PRODUCTION                                  # the production variant: the trace refuses it
    assert L.pxb_trace_scripted(C.byref(c), P(rows), 8, depth, None, None, 0, P(offs), None, None, None) == pxb.PXB_E_INVAL
    assert L.pxb_trace_scripted_device(C.byref(c), P(rows), 8, depth, None, None, 0, P(offs), None, None,
                                       None) == pxb.PXB_E_INVAL
    for bad in (dataclasses.replace(cfg, n_proposers=4), dataclasses.replace(cfg, n_acceptors=1),
                dataclasses.replace(cfg, n_acceptors=10), dataclasses.replace(cfg, delay_max=0),
                dataclasses.replace(cfg, delay_max=16), dataclasses.replace(cfg, step_cap=0),
                dataclasses.replace(cfg, step_cap=4096),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, delay_max=9),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, tick_period=0),
                dataclasses.replace(pxb.LOG_FAULTY_CONFIG, n_ticks=4097)):
        assert inval(ALL, bad, rec_p=P(rec), cap=4), bad
    if not torch.cuda.is_available():                                    # (valid calls: only where no GPU runs them)
        nodev = [pxb.PXB_E_NODEV] * 6
        assert calls(ALL, cfg, rec_p=P(rec), cap=4) == nodev
        assert calls(ALL, cfg, depth_=0) == nodev
        assert calls(ALL, cfg, rows_p=None, ids_p=None, count=0) == nodev    # count == 0 is valid
        assert calls((2, 3, 4, 5), cfg, ids_p=None) == nodev[:4]         # the run and the trace take no ids
        assert calls((0, 1, 2, 3), cfg, offs_p=None) == nodev[:4]        # nor the extract and the run offsets
        with pytest.raises(pxb.PaxosError):
            pxb.run_scripted(cfg, rows, depth)
        with pytest.raises(pxb.PaxosError):
            pxb.extract_schedule(cfg, [1, 2], depth)


def test_script_device_forms_check_buffers_before_the_abi():
    import torch
    cfg = pxb.CONFIGS[3]
    with pytest.raises(ValueError, match="required"):
        pxb.run_scripted_device(cfg, None, 8, 4)
    with pytest.raises(ValueError, match="CUDA"):
        pxb.run_scripted_device(cfg, torch.zeros(8 * pxb.script_stride(cfg, 4), dtype=torch.uint8), 8, 4)
    with pytest.raises(ValueError, match="depth"):
        pxb.run_scripted_device(cfg, None, 0, 4097)
    with pytest.raises(ValueError, match="required"):
        pxb.trace_scripted_device(cfg, None, 0, 4, None)
    with pytest.raises(ValueError, match="uint8"):
        pxb.run_scripted(cfg, np.zeros((2, 5), np.uint8), 4)


# ---- 2. extract -------------------------------------------------------------------
@pytest.mark.parametrize("c", CONFIGS)
def test_host_extract_equals_the_python_builder(c):
    """Byte for byte, ids 0..63 and 2^32 - 32 .. 2^32 + 31, depths 1, 7 and 64;
    no keep anywhere in what an instance's proposers use."""
    cfg = pxb.CONFIGS[c]
    for depth in (1, 7, 64):
        want = explicit_rows(c, depth)
        got = SO.host_extract(cfg, IDS, depth)
        assert got.shape == want.shape and (got == want).all(), depth
        npr = pxb.script_n_proposers(got)
        assert ((npr >= 1) & (npr <= cfg.n_proposers)).all() and (pxb.script_skews(got) != 0xFFFF).all()
        lk = pxb.script_links(cfg, got, depth)
        for i in range(len(IDS)):
            assert (lk[i, :, :npr[i]] != 0xFF).all() and (lk[i, :, npr[i]:] == 0xFF).all()
    if cfg.randomize:
        assert len(set(pxb.script_n_proposers(got).tolist())) == cfg.n_proposers


# ---- 3. all-keep rows ---------------------------------------------------------------
@pytest.mark.parametrize("c", CONFIGS)
def test_all_keep_rows_are_the_plain_instances(c):
    """Depth 0 and depth 8, all 0xFF: the host per-lane result, status and
    records of the plain instance (tests/native/trace_host.cpp); BAILED exactly
    where the plain host trace bails, within that file's cap."""
    cfg = pxb.CONFIGS[c]
    plain = [host_trace(cfg, inst) for inst in IDS]
    bailed = 0
    for depth in (0, 8):
        o = SO.host_run(cfg, pxb.scripts_empty(cfg, IDS, depth), depth, capacity=1100)
        for i, (rec, nw, nk, st, res) in enumerate(plain):
            assert o["status"][i] == st and (o["res"][i] == res).all() and o["n_kept"][i] == nk
            assert (o["rec"][i][:nk] == rec[:nk]).all() and (o["rec"][i][nk:] == 0xA5A5A5A5).all()
            if st == pxb.TRACE_BAILED:
                assert not o["sent"][i].any() and not o["dig"][i].any() and not o["acc"][i].any()
        bailed = int((o["status"] == pxb.TRACE_BAILED).sum())
    assert bailed <= 0.02 * len(IDS) + 1


# ---- 4. extract, then run under a different seed and base -----------------------------
@pytest.mark.parametrize("c", CONFIGS)
def test_explicit_rows_run_the_same_under_another_seed_and_base(c):
    cfg = pxb.CONFIGS[c]
    depth = 64
    rows = explicit_rows(c, depth)
    o = SO.host_run(cfg, rows, depth)
    moved = rows.copy()
    pxb.script_base(moved)[:] = np.array(IDS[::-1], dtype=np.uint64) + 1000003
    m = SO.host_run(dataclasses.replace(cfg, seed=OTHER_SEED), moved, depth)
    covered = 0
    for i, inst in enumerate(IDS):
        if o["status"][i] != pxb.TRACE_OK:
            continue
        want = R.run_instance(SO.rcfg(cfg), inst)
        assert list(o["res"][i]) == [want.decided_val, want.decided_ticket, want.rounds, want.packed_flags()]
        assert int(o["sent"][i].sum()) == want.messages
        if int(o["sent"][i].max()) <= depth:
            covered += 1
            for k in ("status", "res", "dig", "acc", "sent"):
                assert (m[k][i] == o[k][i]).all(), (inst, k)
    assert covered >= 16       # (config 4's duels mostly outrun 64 entries a link; a population, not a share)


# ---- 5. step KATs -------------------------------------------------------------------
KATS = SO.kat_cases()


@pytest.mark.parametrize("case,cfg,row,depth", KATS, ids=[k[0]["name"] for k in KATS])
def test_step_kats_as_explicit_scripts(case, cfg, row, depth):
    """S1-S6 of kat_step_schedule.json (S6 with the n_proposers byte 3) and S7,
    S8 of kat_scripted.json under an unrelated seed and base: the result and
    every checkpoint equal the hand-derived fixture, on the host build and on
    the adapter-driven Python oracle."""
    want = case["result"]
    if case["name"].startswith("S6"):
        assert row[8] == 3
    assert case["name"][:2] not in ("S7", "S8") or " step " in case["what"]
    o = SO.host_run(cfg, row, depth, capacity=want["steps"] + 1)
    assert o["status"][0] == pxb.TRACE_OK and int(o["sent"][0].max()) <= depth
    assert list(o["res"][0]) == [want["decided_val"], want["decided_ticket"], want["rounds"],
                                 want["flags"] | (want["steps"] << 16)]
    assert int(o["sent"][0].sum()) == want["messages"]
    recs = {r["step"]: r for r in pxb.trace_records(o["rec"][0][:o["n_kept"][0]])}
    states = {}

    def snap(s, accs, props, in_flight):
        states[s] = {"in_flight": in_flight,
                     "acc": [[a.t_max, a.t_store, a.val, len(a.log) | (int(a.dead) << 31)] for a in accs],
                     "prop": [[p.ticket, p.cmd, p.acks, p.rs] for p in props]}
    r = SO.oracle_run(cfg, row, depth, trace=snap)
    assert (r.decided_val, r.decided_ticket, r.rounds, r.flags, r.steps, r.messages, r.canon_bytes, r.executes) == \
        tuple(want[k] for k in ("decided_val", "decided_ticket", "rounds", "flags", "steps", "messages",
                                "canon_bytes", "executes"))
    assert [list(a.log) for a in r.acceptors] == (case["logs"] if "logs" in case else want["logs"])
    for cp in case["checkpoints"]:
        g = recs[cp["step"]]
        assert g["acc"].tolist() == cp["acc"] and [list(p[:4]) for p in g["prop"].tolist()] == cp["prop"], cp["step"]
        assert states[cp["step"]]["acc"] == cp["acc"] and states[cp["step"]]["prop"] == cp["prop"], cp["step"]
        if "in_flight" in cp:
            assert g["in_flight"] == cp["in_flight"] == states[cp["step"]]["in_flight"], cp["step"]


# ---- 6. random overrides ----------------------------------------------------------------
@pytest.mark.parametrize("c", CONFIGS)
def test_random_overrides_match_the_adapter_driven_oracle(c):
    """64 rows with about 10 % of the link entries overridden (lost, or delays
    1 .. delay_max + 3: the clamp), some skew, window and P overrides: every
    trace record and result equals the oracle's, by check_against_oracle's rules;
    digests, acceptor records and send counts are the oracle's final state."""
    cfg = pxb.CONFIGS[c]
    depth = 16
    rows = SO.random_overrides(cfg, IDS[:64], depth, seed=1000 + c)
    o = SO.host_run(cfg, rows, depth, capacity=cfg.step_cap + 1)
    checked = 0
    for i in range(64):
        if o["status"][i] == pxb.TRACE_BAILED:
            assert not o["res"][i].any() and o["n_kept"][i] == 0
            continue
        assert o["status"][i] == pxb.TRACE_OK
        res = SO.check_against_oracle(pxb.trace_records(o["rec"][i][:o["n_kept"][i]]), o["res"][i], cfg, rows[i], depth)
        assert int(o["sent"][i].sum()) == res.messages
        assert o["dig"][i].tolist() == [res.digest(a) for a in range(cfg.n_acceptors)]
        assert o["acc"][i].tolist() == [[a.t_max, a.t_store, a.val, len(a.log) | (int(a.dead) << 31)]
                                        for a in res.acceptors]
        checked += 1
    assert checked >= 48       # (a test of the rows it compares: most of them must run)


def test_override_delays_clamp_to_delay_max():
    """A link byte above cfg.delay_max is delivered with delay_max: the run
    equals the one with the byte written as delay_max (what keeps the timing
    wheel safe), and differs from the unclamped oracle reading only there."""
    cfg = pxb.CONFIGS[3]
    depth = 16
    rows = explicit_rows(3, depth)[:16].copy()
    lk = pxb.script_links(cfg, rows, depth)
    lk[:, :, :, :, ::3] = 0xFE
    clamped = rows.copy()
    pxb.script_links(cfg, clamped, depth)[:, :, :, :, ::3] = cfg.delay_max
    a, b = SO.host_run(cfg, rows, depth, capacity=300), SO.host_run(cfg, clamped, depth, capacity=300)
    for k in ("status", "res", "dig", "acc", "sent", "rec", "n_kept"):
        assert (a[k] == b[k]).all(), k
    assert (a["status"] == pxb.TRACE_OK).sum() >= 12


# ---- 7. malformed rows --------------------------------------------------------------------
def test_bad_rows_give_script_bad_and_leave_their_neighbours_alone():
    cfg = pxb.CONFIGS[3]
    depth = 8
    rows = pxb.scripts_empty(cfg, range(12), depth)
    good = SO.host_run(cfg, rows, depth, capacity=300)
    bad = rows.copy()
    bad[3, 8] = cfg.n_proposers + 1          # n_proposers > P
    bad[7, 9] = 1                            # reserved != 0
    bad[8, 8], bad[8, 9] = 200, 255
    o = SO.host_run(cfg, bad, depth, capacity=300)
    for i in range(12):
        if i in (3, 7, 8):
            assert o["status"][i] == pxb.SCRIPT_BAD and o["n_kept"][i] == 0 and o["n_window"][i] == 0
            assert not o["res"][i].any() and not o["dig"][i].any() and not o["acc"][i].any() and not o["sent"][i].any()
            assert (o["rec"][i] == 0xA5A5A5A5).all()
        else:
            for k in ("status", "res", "dig", "acc", "sent", "rec", "n_kept"):
                assert (o[k][i] == good[k][i]).all(), (i, k)


# ---- 8. the shrinker ------------------------------------------------------------------------
def neutralised(cfg, row, depth, fault):
    r = row.copy()
    pxb.script_neutralise(cfg, r, depth, fault)
    return r


@pytest.mark.parametrize("inst", [10, 0])
def test_shrink_with_the_host_runner(inst):
    """Config 3, ids 10 and 0 (both panic): the shrunk row keeps the predicate,
    is 1-minimal (re-checked by neutralising each survivor), runs the same under
    another seed and base, and has no more faults than the original."""
    cfg = pxb.CONFIGS[3]
    depth = 64
    row0 = SO.build_rows(cfg, [inst], depth)
    o0 = SO.host_run(cfg, row0, depth)
    assert int(o0["res"][0][3]) & pxb.F_PANIC and int(o0["sent"][0].max()) <= depth
    before = pxb.script_faults(cfg, row0, depth, o0["sent"][0])
    row, faults, launches = pxb.shrink(cfg, row0[0], pxb.F_PANIC, runner=SO.host_runner, depth=depth)
    print("id %d: %d -> %d faults, %d -> %d steps, %d launches" % (
        inst, len(before), len(faults), int(o0["res"][0][3]) >> 16,
        int(SO.host_run(cfg, row, depth)["res"][0][3]) >> 16, launches))
    o = SO.host_run(cfg, row, depth)
    assert o["status"][0] == pxb.TRACE_OK and int(o["res"][0][3]) & pxb.F_PANIC and int(o["sent"][0].max()) <= depth
    assert faults == pxb.script_faults(cfg, row, depth, o["sent"][0]) and 0 < len(faults) <= len(before)
    assert 1 < launches <= 64
    # fully explicit, benign 1s past what is consumed
    lk = pxb.script_links(cfg, row[None, :], depth)[0]
    assert row[8] in (1, 2) and (pxb.script_skews(row[None, :])[0][:row[8]] != 0xFFFF).all() and (lk != 0xFF).all()
    assert (pxb.script_windows(cfg, row[None, :]) != 0xFFFF).all()
    for dirn in range(2):
        for p in range(2):
            for a in range(5):
                assert (lk[dirn, p, a, int(o["sent"][0][dirn, p, a]):] == 1).all()
    # 1-minimal
    for f in faults:
        n = SO.host_run(cfg, neutralised(cfg, row, depth, f), depth)
        assert not (n["status"][0] == pxb.TRACE_OK and int(n["res"][0][3]) & pxb.F_PANIC
                    and int(n["sent"][0].max()) <= depth), f
    # seed- and base-independent
    moved = row.copy()
    pxb.script_base(moved[None, :])[0] = 987654321012
    m = SO.host_run(dataclasses.replace(cfg, seed=OTHER_SEED), moved, depth)
    for k in ("status", "res", "dig", "acc", "sent"):
        assert (m[k] == o[k]).all(), k
    # and the adapter-driven oracle agrees on the shrunk row
    want = SO.oracle_run(cfg, row, depth)
    assert list(o["res"][0]) == [want.decided_val, want.decided_ticket, want.rounds, want.packed_flags()]


# ---- 9. one stand-alone sanitizer program ------------------------------------------------------
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-DPXB_SCRIPT_HOST_MAIN",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
             "-Werror=shift-count-overflow", "-Werror=shift-count-negative"]


def test_script_core_sanitized():
    """script_host.cpp with its own main (one shape: P = 2, N = 5, W = 8) under
    AddressSanitizer + UBSan, as a subprocess over 256 config-3 rows with random
    overrides, a window, a tail and a capacity that cuts the kept records: every
    buffer holds exactly what the call may write.  Exit status 0, and the output
    equals the unsanitized library's on the same rows."""
    if SO.stale(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        tmp = "%s.%d" % (EXE, os.getpid())
        subprocess.run([SO.HIPCC, *SAN_FLAGS, "-o", tmp, SO.SRC], check=True, timeout=900)
        os.replace(tmp, EXE)
    cfg = pxb.CONFIGS[3]
    sel, cap, n, depth = (4, 60, 5), 3, 256, 12
    P, N = cfg.n_proposers, cfg.n_acceptors
    stride = pxb.script_stride(cfg, depth)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "o.bin")
        e = dict(os.environ)
        e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
        p = subprocess.run([EXE, out, hex(cfg.seed), "0", str(n), str(depth), "12345", str(cfg.loss_ppm),
                            str(cfg.delay_max), str(cfg.skew_max), str(cfg.step_cap), str(sel[0]), str(sel[1]),
                            str(sel[2]), str(cap)], capture_output=True, text=True, env=e, timeout=600)
        assert p.returncode == 0, "sanitized run failed (rc %d): %s" % (p.returncode, p.stderr[-4000:])
        raw = np.fromfile(out, dtype=np.uint8)
    rows = raw[:n * stride].reshape(n, stride).copy()
    assert (rows != SO.host_extract(cfg, range(n), depth)).any()          # (the overrides are in)
    w = raw[n * stride:].view(np.uint32)
    want = SO.host_run(cfg, rows, depth, sel=sel, capacity=cap)
    sw = (2 * P * N + 1) // 2
    o = 0
    for i in range(n):
        nw, nk, st = (int(x) for x in w[o:o + 3])
        res, dig = w[o + 3:o + 7], w[o + 7:o + 7 + N]
        acc = w[o + 7 + N:o + 7 + 5 * N].reshape(N, 4)
        sent = w[o + 7 + 5 * N:o + 7 + 5 * N + sw].view(np.uint16)[:2 * P * N].reshape(2, P, N)
        o += 7 + 5 * N + sw
        m = min(nk, cap)
        rec = w[o:o + m * pxb.TRACE_WORDS].reshape(m, pxb.TRACE_WORDS)
        o += m * pxb.TRACE_WORDS
        assert (nw, nk, st) == (want["n_window"][i], want["n_kept"][i], want["status"][i]), i
        assert (res == want["res"][i]).all() and (dig == want["dig"][i]).all() and (acc == want["acc"][i]).all(), i
        assert (sent == want["sent"][i]).all() and (rec == want["rec"][i][:m]).all() and nk <= 5, i
    assert o == len(w)
