"""Test-side reference for pxb_cover (docs/SEMANTICS.md §14): the coverage mask
of a script row as a fold over the reference model's event list
(``event_oracle.oracle_events``), written from §14's tables and independently
of ``pxb.cover_of_events``; the two are compared on every case they are used
for.  Also what tests/test_cover_host.py and tests/test_cover_gpu.py share: the
cases, the expected summary of a call from its per-row outputs, and the host
build of the coverage lane (tests/native/cover_host.cpp).  No tests here."""
import ctypes as C
import dataclasses
import json
import os
import subprocess

import numpy as np

import event_oracle as EO
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "cover_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libcover_host.so")
DEPS = EO.DEPS[1:] + [SRC, os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", "cover_core.h")]
HIPCC = SO.HIPCC

ASK, PROPOSE, EXECUTE = 0, 1, 2
R1OK, HAVE, R2S, TICK = 0, 1, 2, 3
IDLE, ROUND1, ROUND2 = 0, 1, 2
BIT = {name: 1 << i for i, name in enumerate((
    "ASK_GRANT_EMPTY", "ASK_GRANT_STORED", "ASK_NACK", "PROPOSE_ACCEPT", "PROPOSE_NACK", "EXEC_APPLY", "EXEC_IGNORED",
    "EXEC_PANIC", "DISCARD_DEAD", "DISCARD_ISOLATED", "Q1_FOREIGN_ACCEPT", "Q7_STALE_EXEC", "TICK_START", "TICK_BUSY",
    "HAVE_IDLE", "HAVE_BELOW", "HAVE_RESTART_R1", "HAVE_ABORT_R2", "R1OK_STALE", "R1OK_ACK", "R1OK_PROPOSE_OWN",
    "R1OK_PROPOSE_ADOPTED", "Q5_ADOPTED_OWN", "Q4_TIE", "R2S_DROPPED", "R2S_ACK", "R2S_DONE", "R2S_RESTART",
    "R2S_REPEAT"))}
ALL = (1 << 29) - 1


class _Acc:
    granted = None
    fresh = False
    log_len = 0


class _Prop:
    def __init__(self):
        self.before = {"ticket": 0, "state": IDLE, "mr_t": 0, "mr_v": 0}
        self.seen = set()


def _acceptor(mem, e):
    if e["fate"] != pxb.EVT_HANDLED:
        return ["DISCARD_DEAD" if e["fate"] == pxb.EVT_DISCARDED_DEAD else "DISCARD_ISOLATED"]
    kind = e["in"][0]
    t_max, t_store, val, meta = e["after"][:4]
    reply = e["out"][0] if e["out"] else None
    names = []
    if kind == ASK:
        if reply[0] == R1OK:
            names.append("ASK_GRANT_STORED" if reply[3] else "ASK_GRANT_EMPTY")
            mem.granted = e["peer"]
        else:
            names.append("ASK_NACK")
    elif kind == PROPOSE:
        if reply[0] == R2S:
            names.append("PROPOSE_ACCEPT")
            if mem.granted != e["peer"]:
                names.append("Q1_FOREIGN_ACCEPT")
        else:
            names.append("PROPOSE_NACK")
    elif kind == EXECUTE:
        length, dead = meta & 0x7FFFFFFF, meta >> 31
        if length > mem.log_len:
            names.append("EXEC_APPLY")
            if not mem.fresh:
                names.append("Q7_STALE_EXEC")
        elif not dead:
            names.append("EXEC_IGNORED")
        if dead:
            names.append("EXEC_PANIC")
    mem.fresh = val != 0 and t_store == t_max
    mem.log_len = meta & 0x7FFFFFFF
    return names


def _proposer(mem, e):
    kind, x, y, z = e["in"]
    ticket, cmd, acks, state, mr_t, mr_v, r2_v, pending = e["after"]
    b = mem.before
    n_out = len(e["out"])
    names = []
    if e["peer"] == pxb.EVT_PEER_TICK:
        names.append("TICK_START" if n_out else "TICK_BUSY")
    elif kind == HAVE:
        names.append("HAVE_IDLE" if b["state"] == IDLE else "HAVE_BELOW" if n_out == 0 else
                     "HAVE_RESTART_R1" if b["state"] == ROUND1 else "HAVE_ABORT_R2")
    elif kind == R1OK:
        if b["state"] != ROUND1 or b["ticket"] != x:
            names.append("R1OK_STALE")
        else:
            if n_out == 0:
                names.append("R1OK_ACK")
            elif pending == 0:
                names.append("R1OK_PROPOSE_OWN")
            else:
                names.append("R1OK_PROPOSE_ADOPTED")
                if r2_v == cmd:
                    names.append("Q5_ADOPTED_OWN")
            if z != 0 and b["mr_v"] != 0 and b["mr_t"] == y:
                names.append("Q4_TIE")
    elif kind == R2S:
        if b["state"] != ROUND2:
            names.append("R2S_DROPPED")
        else:
            names.append(("R2S_ACK", "R2S_DONE", "R2S_RESTART")[n_out])
            if e["peer"] in mem.seen:
                names.append("R2S_REPEAT")
            mem.seen.add(e["peer"])
    if any(m[0] == PROPOSE for m in e["out"]):
        mem.seen = set()
    mem.before = {"ticket": ticket, "state": state, "mr_t": mr_t, "mr_v": mr_v}
    return names


def fold(events, n_acceptors, per_event=False):
    """§14 over event dicts (event_oracle.run_events' form): the row's mask, or one mask per event."""
    accs = [_Acc() for _ in range(n_acceptors)]
    props = {}
    per = []
    for e in events:
        if e["actor"] == pxb.EVT_ACCEPTOR:
            names = _acceptor(accs[e["index"]], e)
        else:
            names = _proposer(props.setdefault(e["index"], _Prop()), e)
        m = 0
        for n in names:
            m |= BIT[n]
        per.append(m)
    if per_event:
        return per
    return int(np.bitwise_or.reduce(np.asarray(per, dtype=np.uint32))) if per else 0


def unpack(ev):
    """A structured event array (pxb.event_dtype()) as event dicts."""
    out = []
    for e in ev:
        n = int(e["n_out"])
        out.append({"step": int(e["step"]), "actor": int(e["actor"]), "index": int(e["index"]), "peer": int(e["peer"]),
                    "fate": int(e["fate"]), "in": tuple(int(e["in"][k]) for k in ("kind", "x", "y", "z")),
                    "out": [tuple(int(e["out"][j][k]) for k in ("kind", "x", "y", "z")) for j in range(n)],
                    "after": tuple(int(v) for v in e["after"])})
    return out


def oracle_row(cfg, row, depth):
    """(mask by this fold, steps, the packed events) of one well-formed row from
    the reference model; the mask by pxb.cover_of_events must agree."""
    events, summary = EO.oracle_events(cfg, row, depth)
    m = fold(events, cfg.n_acceptors)
    packed = EO.pack(events)
    spec = pxb.cover_of_events(packed, cfg.n_acceptors)
    assert spec == m, "the two folds differ: %s vs %s" % (pxb.cover_names(spec), pxb.cover_names(m))
    return m, summary[4], packed


def expected_summary(masks, status, res, ids=None):
    """The summary of a call from its per-row outputs, as a dict of plain values:
    counts and argmin of (steps, i) per class; witnesses as row indices, or as
    ids[i] (Python ints) when ids is given."""
    masks, status = np.asarray(masks, dtype=np.uint32), np.asarray(status)
    steps = (np.asarray(res, dtype=np.uint32).reshape(-1, 4)[:, 3] >> 16).astype(np.int64)
    ok = status == pxb.TRACE_OK
    out = {"rows_ok": int(ok.sum()), "rows_bailed": int((status == pxb.TRACE_BAILED).sum()),
           "rows_bad": int((status == pxb.SCRIPT_BAD).sum()), "counts": [], "witness": [], "witness_steps": [],
           "union": 0}
    idx = np.arange(len(masks), dtype=np.int64)
    for b in range(29):
        has = ok & (((masks >> np.uint32(b)) & np.uint32(1)) != 0)
        n = int(has.sum())
        out["counts"].append(n)
        if n:
            i = int(idx[has][np.lexsort((idx[has], steps[has]))[0]])
            out["witness"].append(i if ids is None else int(ids[i]) & ((1 << 64) - 1))
            out["witness_steps"].append(int(steps[i]))
            out["union"] |= 1 << b
        else:
            out["witness"].append((1 << 64) - 1)
            out["witness_steps"].append(0xFFFFFFFF)
    return out


def summary_dict(s):
    """A pxb.CoverSummary as expected_summary's dict."""
    assert s.tail == [(0, (1 << 64) - 1, 0xFFFFFFFF)] * 3 + [0], s.tail          # bits 29..31 and reserved
    return {"rows_ok": s.rows_ok, "rows_bailed": s.rows_bailed, "rows_bad": s.rows_bad, "counts": s.counts,
            "witness": s.witness, "witness_steps": s.witness_steps, "union": s.union}


# ---- the cases (tests/test_cover_host.py: all ids; tests/test_cover_gpu.py: the first 256) ----
_LOSSY = pxb.Config(seed=0x5EED0003, n_proposers=2, n_acceptors=3, loss_ppm=100000, delay_max=4, skew_max=3,
                    step_cap=64)
_C4, _C5 = pxb.CONFIGS[4], pxb.CONFIGS[5]
CASES = {
    # name: (config, number of ids from 0, also as rows extracted at depth 64)
    "config1-p1n3": (pxb.CONFIGS[1], 8, False),
    "lossy-p2n3": (_LOSSY, 3000, True),
    "windows-p2n3": (dataclasses.replace(_LOSSY, crash_ppm=_C4.crash_ppm, crash_len_max=_C4.crash_len_max,
                                         crash_start_max=_C4.crash_start_max), 2000, False),
    "randomize-p3n3": (dataclasses.replace(_C5, n_acceptors=3, step_cap=64), 2000, False),
    "log-p2n3": (pxb.Config(seed=0x5EED0007, n_proposers=2, n_acceptors=3, loss_ppm=100000, delay_max=4, skew_max=3,
                            step_cap=128, n_ticks=4, tick_period=8), 1000, False),
}
EXTRACT_DEPTH = 64
_oracle = {}


def case_oracle(name, limit=None):
    """(cfg, ids, masks, steps) of a case's first `limit` ids from the reference
    model, as all-keep rows at depth 0; computed once per (case, limit)."""
    cfg, n, _ = CASES[name]
    n = n if limit is None else min(n, limit)
    if (name, n) not in _oracle:
        full = _oracle.get((name, CASES[name][1]))
        if full is not None:
            _oracle[(name, n)] = (cfg, full[1][:n], full[2][:n], full[3][:n])
        else:
            ids = np.arange(n, dtype=np.uint64)
            rows = pxb.scripts_empty(cfg, ids, 0)
            got = [oracle_row(cfg, rows[i], 0)[:2] for i in range(n)]
            _oracle[(name, n)] = (cfg, ids, np.array([g[0] for g in got], dtype=np.uint32),
                                  np.array([g[1] for g in got], dtype=np.uint32))
    return _oracle[(name, n)]


KAT_PATH = os.path.join(HERE, "golden", "kat_cover.json")


def kat_cases():
    return json.load(open(KAT_PATH))["cases"]


def kat_row(case):
    """(cfg, row, depth) of a tests/golden/kat_cover.json case: its explicit row."""
    cfg = pxb.Config(**case["config"])
    depth = case["depth"]
    row = np.frombuffer(bytes.fromhex(case["row_hex"]), dtype=np.uint8).copy()
    assert len(row) == pxb.script_stride(cfg, depth)
    return cfg, row, depth


# ---- a malformed row and a row that bails among good ones ---------------------------
BAIL_CFG = pxb.Config(seed=0xBA11ED, n_proposers=3, n_acceptors=3, delay_max=15, skew_max=3, step_cap=96)
BAIL_ID = 3455          # delays up to 15 and three duelling proposers: a request FIFO takes a fifth entry


def bad_and_bailed_rows():
    """(cfg, rows at depth 0, the index of the malformed row, of the bailing row): ids 0..69 with both among them."""
    ids = np.arange(70, dtype=np.uint64)
    ids[40] = BAIL_ID
    rows = pxb.scripts_empty(BAIL_CFG, ids, 0)
    rows[5, 9] = 1                                      # reserved byte set: malformed
    return BAIL_CFG, rows, 5, 40


def check_bad_and_bailed(cfg, rows, i_bad, i_bail, m, st, res, s):
    good = [i for i in range(len(rows)) if i not in (i_bad, i_bail)]
    assert st[i_bad] == pxb.SCRIPT_BAD and st[i_bail] == pxb.TRACE_BAILED and (st[good] == pxb.TRACE_OK).all()
    assert m[i_bad] == 0 and m[i_bail] == 0 and not res[i_bad].any() and not res[i_bail].any()
    want = [oracle_row(cfg, rows[i], 0)[:2] for i in good]
    assert [int(x) for x in m[good]] == [w[0] for w in want]
    assert [int(x) >> 16 for x in res[good, 3]] == [w[1] for w in want]
    assert (s.rows_ok, s.rows_bailed, s.rows_bad) == (len(good), 1, 1)
    assert summary_dict(s) == expected_summary(m, st, res)
    assert all(w not in (i_bad, i_bail) for w in s.witness)


# ---- the host build of the coverage lane --------------------------------------------
_lib = None


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def lib():
    global _lib
    if _lib is None:
        if stale(OUT):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", tmp, SRC],
                           check=True, timeout=900)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
        vp = C.c_void_p
        _lib.cover_host_run.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
    return _lib


def host_cover(cfg, rows, depth, cflags=0):
    """pxb.cover through the host build: (rc, masks, status, results, summary CoverSummary or None)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim == 1:
        rows = rows[None, :]
    n = len(rows)
    c = cfg.to_c(0, 1)
    c.flags |= cflags
    masks = np.zeros(n, np.uint32)
    status = np.zeros(n, np.uint32)
    res = np.zeros((n, 4), np.uint32)
    s = pxb.pxb_cover_summary()
    rc = lib().cover_host_run(C.addressof(c), rows.ctypes.data if n else None, n, depth, masks.ctypes.data if n else None,
                              status.ctypes.data if n else None, res.ctypes.data if n else None, C.addressof(s))
    return rc, masks, status, res, (pxb.CoverSummary(s) if rc == 0 else None)
