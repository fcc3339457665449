"""Test-side reference for pxb_trace_events (docs/SEMANTICS.md §13): the event
list of a script row from the reference model (oracle/paxos_ref.py).

``run_events`` restates ``run_instance``'s step loop over the SAME handler
functions (``acceptor_handle``, ``proposer_handle``, ``proposer_tick``) and the
same draws (``instance_params`` and ``philox4x32_10``, looked up in the module
at call time, so ``script_oracle.scripted`` drives it as it drives
``run_instance``) and records one event per pop, in the order of the pops.
tests/test_events_host.py pins it to the unmodified ``run_instance`` on every
case it is used for: the same final result, digests and acceptor records, and
the "after" state of the last event of each actor in a step equal to
``oracle_trace``'s end-of-step record.

The oracle does not tell dead from isolated (``if acc.dead or isolated``); the
events label dead first, as the ABI does.

``host``: the host build of the event lane (tests/native/events_host.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import paxos_ref as R
import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "events_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libevents_host.so")
DEPS = [SRC, os.path.join(HERE, "native", "host_lane.h")] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "paxos_trace_core.h", "ev_layouts.h",
              "lane_shapes.h", "script_core.h", "script_lane.h", "events_core.h")] + [
    os.path.join(ROOT, "include", "paxos_batch.h")]
TICK = 3


def _digest(log):
    h = R.FNV_BASIS
    for v in log:
        h = R.fnv1a_u32(h, v)
    return R.fnv1a_u32(h, len(log))


def _acc_after(a):
    return (a.t_max, a.t_store, a.val, len(a.log) | (int(a.dead) << 31), _digest(a.log), 0, 0, 0)


def _prop_after(p):
    return (p.ticket, p.cmd, p.acks, p.rs, p.mr_t, p.mr_v, p.r2_v, int(p.pending))


def run_events(cfg, inst, queue_depth=R.QUEUE_DEPTH):
    """run_instance's step loop, recording an event per pop.  Returns (events,
    summary): events as dicts (step, actor, index, peer, fate, in, out, after),
    summary = (decided_val, decided_ticket, rounds, flags, steps, acceptors)."""
    N = cfg.n_acceptors
    prm = R.instance_params(cfg, inst)
    P = prm.P
    key = (cfg.seed & R.M32, (cfg.seed >> 32) & R.M32)
    lo, hi = inst & R.M32, (inst >> 32) & R.M32
    accs = [R.Acceptor() for _ in range(N)]
    props = [R.Proposer(client_id=p + 1) for p in range(P)]
    req = [[R._Link() for _ in range(N)] for _ in range(P)]
    rsp = [[R._Link() for _ in range(P)] for _ in range(N)]
    flags = rounds = 0
    decided = None
    n_ticks = max(1, cfg.n_ticks)
    period = cfg.tick_period if n_ticks > 1 else 1
    last_tick = max(prm.skew) + (n_ticks - 1) * period
    faulty = prm.loss_thr > 0 or prm.delay_max > 1
    events = []

    def send(link, s, dirn, p, a, msg):
        nonlocal flags
        k = link.seq
        link.seq += 1
        d = 1
        if faulty:
            w = R.philox4x32_10((lo, hi, k, (R.PURPOSE_MSG << 24) | (dirn << 16) | (p << 8) | a), key)
            if w[0] < prm.loss_thr:
                return
            d = 1 + R.mulhi(w[1], prm.delay_max)
        if len(link.q) >= queue_depth:
            flags |= R.F_QUEUE_OVERFLOW
            return
        due = max(s + d, link.last_due)
        link.last_due = due
        link.q.append((due, msg))

    def bcast(p, s, out):
        nonlocal rounds, decided
        for (kind, ticket, val) in out:
            if kind == R.ASK:
                rounds += 1
            if kind == R.EXECUTE and decided is None:
                decided = (props[p].r2_v, ticket)
            for a in range(N):
                send(req[p][a], s, 0, p, a, (kind, ticket, val))

    steps = 0
    for s in range(cfg.step_cap):
        steps = s + 1
        for a in range(N):
            acc = accs[a]
            c0, c1 = prm.iso[a]
            isolated = c0 <= s < c1
            for p in range(P):
                link = req[p][a]
                while link.q and link.q[0][0] <= s:
                    _, (kind, ticket, val) = link.q.popleft()
                    ev = {"step": s, "actor": pxb.EVT_ACCEPTOR, "index": a, "peer": p,
                          "in": (kind, ticket, 0, val), "out": []}
                    events.append(ev)
                    if acc.dead or isolated:
                        ev["fate"] = pxb.EVT_DISCARDED_DEAD if acc.dead else pxb.EVT_DISCARDED_ISOL
                        ev["after"] = _acc_after(acc)
                        continue
                    ev["fate"] = pxb.EVT_HANDLED
                    rep = R.acceptor_handle(acc, kind, ticket, val)
                    if acc.dead:
                        flags |= R.F_PANIC
                    ev["after"] = _acc_after(acc)
                    if rep is not None:
                        ev["out"] = [tuple(rep)]
                        send(rsp[a][p], s, 1, p, a, rep)
        for p in range(P):
            pr = props[p]
            since = s - prm.skew[p]
            if since >= 0 and since % period == 0 and since // period < n_ticks:
                out = R.proposer_tick(pr)
                events.append({"step": s, "actor": pxb.EVT_PROPOSER, "index": p, "peer": pxb.EVT_PEER_TICK,
                               "fate": pxb.EVT_HANDLED, "in": (TICK, 0, 0, 0),
                               "out": [(k, t, 0, v) for (k, t, v) in out], "after": _prop_after(pr)})
                bcast(p, s, out)
            for a in range(N):
                link = rsp[a][p]
                while link.q and link.q[0][0] <= s:
                    _, (kind, x, y, z) = link.q.popleft()
                    out = R.proposer_handle(pr, N, kind, x, y, z)
                    events.append({"step": s, "actor": pxb.EVT_PROPOSER, "index": p, "peer": a,
                                   "fate": pxb.EVT_HANDLED, "in": (kind, x, y, z),
                                   "out": [(k, t, 0, v) for (k, t, v) in out], "after": _prop_after(pr)})
                    bcast(p, s, out)
        in_flight = any(l.q for row in req for l in row) or any(l.q for row in rsp for l in row)
        if not in_flight and s >= last_tick:
            break
    else:
        flags |= R.F_STEP_CAP
    dv, dt = decided if decided else (R.NOTHING, 0)
    return events, (dv, dt, rounds, flags, steps, accs)


def oracle_events(cfg, row, depth):
    """The events of a script row, through script_oracle's adapter."""
    with SO.scripted(cfg, row, depth) as base:
        return run_events(SO.rcfg(cfg), base)


def pack(events):
    """Event dicts as a structured array of pxb.event_dtype(): the bytes the ABI defines."""
    out = np.zeros(len(events), dtype=pxb.event_dtype())
    for r, e in zip(out, events):
        r["step"], r["actor"], r["index"], r["peer"], r["fate"] = e["step"], e["actor"], e["index"], e["peer"], e["fate"]
        r["n_out"] = len(e["out"])
        r["in"] = e["in"]
        for j, m in enumerate(e["out"]):
            r["out"][j] = m
        r["after"] = e["after"]
    return out


def last_after(events, n_acc, n_prop):
    """Per step with events: {step: (acc {a: after}, prop {p: after})}, the after
    state of the last event of each actor in the step."""
    out = {}
    for e in events:
        acc, prop = out.setdefault(int(e["step"]), ({}, {}))
        if e["actor"] == pxb.EVT_ACCEPTOR:
            acc[int(e["index"])] = tuple(int(x) for x in e["after"][:5])
        else:
            prop[int(e["index"])] = tuple(int(x) for x in e["after"])
    return out


# ---- the host build of the event lane ------------------------------------------------
_lib = None
HIPCC = SO.HIPCC


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
        _lib.events_host_run.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]
    return _lib


GUARD = 0xA5


def host_events(cfg, rows, depth, sel=None, capacity=None, pad=0, cflags=0):
    """pxb.trace_events through the host build.  Returns (rc, events, offsets,
    status, results, total); the event buffer has `pad` guard events (bytes
    0xA5) behind `capacity`, returned with it when pad > 0."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim == 1:
        rows = rows[None, :]
    n = len(rows)
    c = cfg.to_c(0, 1)
    c.flags |= cflags
    s = pxb.pxb_trace_sel(*sel) if sel is not None else None
    sp = C.addressof(s) if s is not None else None
    offs = np.zeros(n + 1, np.uint64)
    status = np.zeros(n, np.uint32)
    res = np.zeros((n, 4), np.uint32)
    total = C.c_uint64(0)
    L = lib()
    tail = (offs.ctypes.data, status.ctypes.data if n else None, res.ctypes.data if n else None, C.addressof(total))
    rp = rows.ctypes.data if n else None
    if capacity is None:
        rc = L.events_host_run(C.addressof(c), rp, n, depth, sp, None, 0, *tail)
        if rc:
            return rc, None, offs, status, res, 0
        capacity = total.value
    ev = np.zeros(capacity + pad, dtype=pxb.event_dtype())
    ev.view(np.uint8)[:] = GUARD
    rc = L.events_host_run(C.addressof(c), rp, n, depth, sp, ev.ctypes.data if capacity else None, capacity, *tail)
    m = min(total.value, capacity)
    return rc, (ev if pad else ev[:m]), offs, status, res, total.value
