"""Test-side helpers for scripted schedules (docs/SEMANTICS.md §10).

* ``build_rows``: a Python builder of fully explicit script rows from the
  reference model's own primitives (``instance_params``, ``philox4x32_10``,
  ``mulhi``): what pxb_schedule_extract must write, byte for byte.
* ``scripted``: an adapter that lets the UNMODIFIED reference model
  (oracle/paxos_ref.py) run a script row.  ``run_instance`` looks
  ``instance_params`` and ``philox4x32_10`` up as module globals; the adapter
  swaps both for the duration of one run: the instance parameters become the
  row's (loss threshold 1, delay_max 16), and a message draw answers with
  synthetic words that decode to the row's outcome, w0 = 0 iff lost and
  w1 = (d - 1) << 28.
* ``host``: the host build of the scripted lane (tests/native/script_host.cpp).
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

import paxos_ref as R
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "script_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libscript_host.so")
DEPS = [SRC, os.path.join(HERE, "native", "host_lane.h")] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "paxos_trace_core.h", "ev_layouts.h",
              "lane_shapes.h", "script_core.h", "script_lane.h")] + [os.path.join(ROOT, "include", "paxos_batch.h")]
HIPCC = "/opt/rocm/bin/hipcc"
U32 = 0xFFFFFFFF
_real_params, _real_philox = R.instance_params, R.philox4x32_10


def rcfg(cfg):
    return R.Config(**cfg.__dict__)


def _key(cfg):
    return (cfg.seed & R.M32, (cfg.seed >> 32) & R.M32)


def _skews(cfg, inst):
    if cfg.skew_max <= 0:
        return [0, 0, 0]
    w = _real_philox((inst & R.M32, (inst >> 32) & R.M32, 0, R.PURPOSE_SKEW << 24), _key(cfg))
    return [R.mulhi(w[p], cfg.skew_max + 1) for p in range(3)]


def _link_byte(prm, w):
    """A message draw as a link byte: 0 lost, else the delay."""
    return 0 if w[0] < prm.loss_thr else 1 + R.mulhi(w[1], prm.delay_max)


def build_rows(cfg, ids, depth):
    """The fully explicit rows of ids under cfg: uint8 (n, stride)."""
    P, N = cfg.n_proposers, cfg.n_acceptors
    rc = rcfg(cfg)
    rows = np.zeros((len(ids), pxb.script_stride(cfg, depth)), dtype=np.uint8)
    pxb.script_base(rows)[:] = np.asarray(ids, dtype=np.uint64)
    lk = pxb.script_links(cfg, rows, depth)
    lk[:] = 0xFF
    for i, inst in enumerate(ids):
        inst = int(inst)
        prm = _real_params(rc, inst)
        lo, hi = inst & R.M32, (inst >> 32) & R.M32
        pxb.script_n_proposers(rows)[i] = prm.P
        sk = _skews(rc, inst)
        pxb.script_skews(rows)[i] = [sk[p] if p < prm.P else 0 for p in range(3)]
        pxb.script_windows(cfg, rows)[i] = [(min(c0, 4096), min(c1, 4096)) for c0, c1 in prm.iso]
        for dirn in range(2):
            for p in range(prm.P):
                for a in range(N):
                    for k in range(depth):
                        w = _real_philox((lo, hi, k, (R.PURPOSE_MSG << 24) | (dirn << 16) | (p << 8) | a), _key(rc))
                        lk[i, dirn, p, a, k] = _link_byte(prm, w)
    return rows


@contextlib.contextmanager
def scripted(cfg, row, depth):
    """Within the block, R.run_instance(rcfg(cfg), base) runs the script row."""
    row = np.ascontiguousarray(row, dtype=np.uint8).reshape(1, -1)
    rc = rcfg(cfg)
    P, N = cfg.n_proposers, cfg.n_acceptors
    base = int(pxb.script_base(row)[0])
    npr = int(pxb.script_n_proposers(row)[0])
    assert npr <= P and row[0, 9] == 0, "a malformed row has no oracle run"
    real = _real_params(rc, base)
    lk = pxb.script_links(cfg, row, depth)[0]

    def params(c, inst):
        assert inst == base
        Pi = npr or real.P
        sk = _skews(rc, base)
        skew = [int(v) if v != 0xFFFF else sk[p] for p, v in enumerate(pxb.script_skews(row)[0])][:Pi]
        iso = []
        for a in range(N):
            c0, c1 = (int(x) for x in pxb.script_windows(cfg, row)[0, a])
            if c0 == 0xFFFF and c1 == 0xFFFF:
                iso.append(real.iso[a])
            else:
                c0, c1 = min(c0, 4096), min(c1, 4096)
                iso.append((c0, c1) if c0 < c1 else (0, 0))
        return R.InstanceParams(Pi, 1, 16, skew, iso)

    def philox(ctr, key):
        w = _real_philox(ctr, key)
        c3 = ctr[3]
        if (c3 >> 24) != R.PURPOSE_MSG:
            return w
        dirn, p, a, k = (c3 >> 16) & 0xFF, (c3 >> 8) & 0xFF, c3 & 0xFF, ctr[2]
        b = int(lk[dirn, p, a, k]) if k < depth else 0xFF
        if b == 0xFF:
            b = _link_byte(real, w)
        else:
            b = min(b, cfg.delay_max)
        return (0 if b == 0 else 1, (max(b, 1) - 1) << 28, 0, 0)

    R.instance_params, R.philox4x32_10 = params, philox
    try:
        yield base
    finally:
        R.instance_params, R.philox4x32_10 = _real_params, _real_philox


def oracle_run(cfg, row, depth, trace=None):
    with scripted(cfg, row, depth) as base:
        return R.run_instance(rcfg(cfg), base, trace=trace)


def _digest(log):
    h = R.FNV_BASIS
    for v in log:
        h = R.fnv1a_u32(h, v)
    return R.fnv1a_u32(h, len(log))


def oracle_trace(cfg, row, depth):
    recs = []

    def snap(s, accs, props, in_flight):
        recs.append({"step": s, "in_flight": in_flight,
                     "acc": [(a.t_max, a.t_store, a.val, len(a.log) | (int(a.dead) << 31)) for a in accs],
                     "digest": [_digest(a.log) for a in accs],
                     "prop": [(p.ticket, p.cmd, p.acks, p.rs, p.mr_t, p.mr_v, p.r2_v, int(p.pending))
                              for p in props]})
    return recs, oracle_run(cfg, row, depth, trace=snap)


def as_rec(g):
    return {"step": g["step"], "in_flight": g["in_flight"],
            "acc": [tuple(int(x) for x in r) for r in g["acc"]], "digest": [int(x) for x in g["digest"]],
            "prop": [tuple(int(x) for x in r) for r in g["prop"]]}


def check_against_oracle(g, gres, cfg, row, depth):
    """tests/test_trace_batch_host.py::check_against_oracle's rules for a script
    row: every recorded step equals the adapter-driven oracle's end-of-step
    state; the steps it skips change nothing; the result is the oracle's."""
    want, res = oracle_trace(cfg, row, depth)
    keys = ("acc", "digest", "prop", "in_flight")
    prev = None
    gi = iter(as_rec(x) for x in g)
    cur = next(gi)
    for r in want:
        if cur is not None and r["step"] == cur["step"]:
            assert r == cur, "step %d: oracle %s host %s" % (r["step"], r, cur)
            prev, cur = cur, next(gi, None)
        else:                                          # a skipped step: nothing changed
            assert prev is not None and {k: r[k] for k in keys} == {k: prev[k] for k in keys}, r["step"]
    assert cur is None and g[-1]["step"] == want[-1]["step"]
    assert list(gres) == [res.decided_val, res.decided_ticket, res.rounds, res.packed_flags()]
    return res


# ---- the step KATs as explicit scripts ----------------------------------------------
KAT_SEED, KAT_BASE, KAT_DEPTH = 0xC0FFEE1234567, (1 << 33) + 77, 64


def script_row(cfg, script, depth, base):
    """The row of a kat_scripted.json 'script': listed link outcomes, 1s past them."""
    rows = pxb.scripts_empty(cfg, [base], depth)
    pxb.script_n_proposers(rows)[0] = script["n_proposers"]
    pxb.script_skews(rows)[0] = (list(script["skew"]) + [0, 0, 0])[:3]
    pxb.script_windows(cfg, rows)[0] = script["windows"]
    lk = pxb.script_links(cfg, rows, depth)
    lk[0] = 1
    for name, seq in script["links"].items():
        src, dst = name.split("->")
        dirn = 0 if src[0] == "p" else 1
        p, a = (int(src[1:]), int(dst[1:])) if dirn == 0 else (int(dst[1:]), int(src[1:]))
        lk[0, dirn, p, a, :len(seq)] = seq
    return rows[0]


def kat_cases():
    """S1-S6 (kat_step_schedule.json, read only: each instance's schedule built
    as an explicit row) and S7-S8 (kat_scripted.json, written as scripts), every
    one under an unrelated seed and base: (case, cfg, row, depth)."""
    import json
    out = []
    for case in json.load(open(os.path.join(HERE, "golden", "kat_step_schedule.json")))["cases"]:
        cfg = pxb.Config(**case["config"])
        row = build_rows(cfg, [case["instance"]], KAT_DEPTH)[0]
        pxb.script_base(row[None, :])[0] = KAT_BASE
        out.append((case, pxb.Config(**dict(case["config"], seed=KAT_SEED)), row, KAT_DEPTH))
    fx = json.load(open(os.path.join(HERE, "golden", "kat_scripted.json")))
    for case in fx["cases"]:
        cfg = pxb.Config(**dict(case["config"], seed=KAT_SEED))
        out.append((case, cfg, script_row(cfg, case["script"], fx["depth"], KAT_BASE), fx["depth"]))
    return out


# ---- the host build of the scripted lane -------------------------------------------
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
        _lib.script_host_stride.argtypes = [C.c_uint32] * 3
        _lib.script_host_stride.restype = C.c_uint64
        _lib.script_host_extract.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp]
        _lib.script_host_run.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64] + [vp] * 7
    return _lib


def host_extract(cfg, ids, depth):
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    rows = np.full((len(ids), pxb.script_stride(cfg, depth)), 0xA5, dtype=np.uint8)
    c = cfg.to_c(0, 1)
    assert lib().script_host_extract(C.addressof(c), ids.ctypes.data, len(ids), depth, rows.ctypes.data) == 0
    return rows


def host_run(cfg, rows, depth, sel=None, capacity=0, pad=0):
    """The rows through the host build: a dict of rec (n, capacity + pad,
    TRACE_WORDS) sentinel-filled, n_window, n_kept, status, res, dig, acc, sent."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim == 1:
        rows = rows[None, :]
    assert rows.shape[1] == pxb.script_stride(cfg, depth)
    n, P, N = len(rows), cfg.n_proposers, cfg.n_acceptors
    cap = capacity + pad
    o = {"rec": np.full((n, cap, pxb.TRACE_WORDS), 0xA5A5A5A5, dtype=np.uint32),
         "n_window": np.zeros(n, np.uint32), "n_kept": np.zeros(n, np.uint32), "status": np.zeros(n, np.uint32),
         "res": np.zeros((n, 4), np.uint32), "dig": np.zeros((n, N), np.uint32), "acc": np.zeros((n, N, 4), np.uint32),
         "sent": np.zeros((n, 2, P, N), np.uint16)}
    c = cfg.to_c(0, 1)
    s = pxb.pxb_trace_sel(*sel, 0) if sel is not None else None
    if pad:                                            # (rows `cap` apart, `capacity` of them writable: one call a row)
        for i in range(n):
            rc = lib().script_host_run(C.addressof(c), rows[i].ctypes.data, 1, depth,
                                       C.addressof(s) if s is not None else None, o["rec"][i].ctypes.data, capacity,
                                       o["n_window"][i:].ctypes.data, o["n_kept"][i:].ctypes.data,
                                       o["status"][i:].ctypes.data, o["res"][i:].ctypes.data, o["dig"][i:].ctypes.data,
                                       o["acc"][i:].ctypes.data, o["sent"][i:].ctypes.data)
            assert rc == 0, "script_host_run rc=%d" % rc
        return o
    rc = lib().script_host_run(C.addressof(c), rows.ctypes.data, n, depth, C.addressof(s) if s is not None else None,
                               o["rec"].ctypes.data if capacity else None, capacity, o["n_window"].ctypes.data,
                               o["n_kept"].ctypes.data, o["status"].ctypes.data, o["res"].ctypes.data,
                               o["dig"].ctypes.data, o["acc"].ctypes.data, o["sent"].ctypes.data)
    assert rc == 0, "script_host_run rc=%d" % rc
    return o


def host_runner(cfg, rows, depth):
    """pxb.shrink's runner over the host build."""
    o = host_run(cfg, rows, depth)
    return o["res"], o["status"], o["sent"]


def random_overrides(cfg, ids, depth, seed):
    """Explicit rows of `ids` with about 10 % of the link entries overridden
    (a quarter of those lost, the rest delays 1 .. delay_max + 3, so the clamp is
    exercised) and some skew, window and proposer-count overrides; a third of
    the rows start from all-keep rows instead, so that keep entries mix in."""
    rng = np.random.default_rng(seed)
    rows = build_rows(cfg, ids, depth)
    keep = pxb.scripts_empty(cfg, ids, depth)
    for i in range(len(ids)):
        if i % 3 == 2:
            rows[i] = keep[i]
    lk = pxb.script_links(cfg, rows, depth)
    m = rng.random(lk.shape) < 0.10
    v = np.where(rng.random(lk.shape) < 0.25, 0, rng.integers(1, cfg.delay_max + 4, lk.shape)).astype(np.uint8)
    lk[m] = v[m]
    for i in range(len(ids)):
        if rng.random() < 0.25:
            pxb.script_n_proposers(rows)[i] = rng.integers(1, cfg.n_proposers + 1)
        if rng.random() < 0.25:
            pxb.script_skews(rows)[i, rng.integers(0, 3)] = rng.integers(0, 6)
        if rng.random() < 0.25:
            c0 = int(rng.integers(0, 12))
            pxb.script_windows(cfg, rows)[i, rng.integers(0, cfg.n_acceptors)] = (c0, c0 + int(rng.integers(0, 10)))
    return rows
