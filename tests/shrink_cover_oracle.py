"""Test-side helpers for the shrinker over a coverage predicate
(docs/SEMANTICS.md §16).

* ``host_batch``: the host build of the shared logic
  (tests/native/shrink_cover_host.cpp), pxb_shrink_cover_batch's arguments and
  outputs.
* ``host_runner``: pxb.shrink_cover's runner over the host builds of the
  scripted lane (script_oracle) and of the coverage lane (cover_oracle).
* ``reference``: pxb.shrink_cover for one row as the batch reports it (a status
  where it raises), computed once per (config, row, arguments, runner).
* ``check``: one instance of a batch against its reference.
No tests here."""
import ctypes as C
import os
import subprocess

import numpy as np

import cover_oracle as CO
import pxb
import script_oracle as SO
import shrink_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "shrink_cover_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libshrink_cover_host.so")
DEPS = sorted(set(H.DEPS[1:] + CO.DEPS + [SRC] + [os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
                                                   for f in ("shrink_cover_core.h", "cover_core.h", "events_core.h")]))
KEYS = ("rows", "status", "n_faults", "launches", "sent", "res", "sig", "masks")
_lib = None
_refs = {}


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def lib():
    global _lib
    if _lib is None:
        if stale(OUT):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run([SO.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", tmp, SRC],
                           check=True, timeout=900)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
        vp = C.c_void_p
        _lib.shrink_cover_host_batch.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp] + [vp] * 7
    return _lib


def pred(query, flag_mask=0, max_launches=64):
    q = query if query is not None else pxb.CoverQuery()
    return pxb.pxb_shrink_pred(flag_mask, max_launches, (C.c_uint32 * 2)(0, 0), q.to_c())


def host_batch(cfg, instances, query, flag_mask=0, depth=64, max_launches=64):
    """shrink_cover_host_batch over ids (1-D) or rows (2-D): a dict of KEYS."""
    inst = np.asarray(instances)
    ids = None
    if inst.ndim == 2:
        rows = np.ascontiguousarray(inst, dtype=np.uint8).copy()
        assert rows.shape[1] == pxb.script_stride(cfg, depth)
    else:
        ids = np.ascontiguousarray(inst, dtype=np.uint64)
        rows = np.full((len(ids), pxb.script_stride(cfg, depth)), 0xA5, dtype=np.uint8)
    n, P, N = len(rows), cfg.n_proposers, cfg.n_acceptors
    o = {"rows": rows, "status": np.full(n, 99, np.uint32), "n_faults": np.full(n, 99, np.uint32),
         "launches": np.zeros(n, np.uint32), "sent": np.full((n, 2, P, N), 7, np.uint16),
         "res": np.zeros((n, 4), np.uint32), "sig": np.zeros(n, np.uint64), "masks": np.full(n, 0xABCD, np.uint32)}
    c = cfg.to_c(0, 1)
    pr = pred(query, flag_mask, max_launches)
    rc = lib().shrink_cover_host_batch(C.addressof(c), ids.ctypes.data if ids is not None else None, rows.ctypes.data,
                                       n, depth, C.addressof(pr), o["status"].ctypes.data, o["n_faults"].ctypes.data,
                                       o["launches"].ctypes.data, o["sent"].ctypes.data, o["res"].ctypes.data,
                                       o["sig"].ctypes.data, o["masks"].ctypes.data)
    assert rc == 0, "shrink_cover_host_batch rc=%d" % rc
    return o


def as_dict(out):
    """pxb.shrink_cover_batch's tuple as host_batch's dict."""
    return dict(zip(KEYS, out))


def host_runner(cfg, rows, depth):
    """pxb.shrink_cover's runner over the host builds: script_oracle.host_runner plus cover_oracle.host_cover."""
    res, status, sent = SO.host_runner(cfg, rows, depth)
    rc, masks, cst, _, _ = CO.host_cover(cfg, rows, depth)
    assert rc == 0 and (cst == status).all()
    return res, status, sent, masks


def gpu_cover(cfg, rows, depth):
    """The masks of rows as pxb.cover gives them (0 where the status is not OK)."""
    return pxb.cover(cfg, rows, depth)[0]


def reference(cfg, row, query, flag_mask=0, depth=64, max_launches=64, runner=None):
    """pxb.shrink_cover(cfg, row, ...) as the batch reports it: {"status", "row",
    "faults", "launches", "mask"}.  Where it raises for a row that is no input:
    NOT_INPUT, the row as given, launches 1, no faults, and the given row's mask
    by the runner (what pxb.cover gives: 0 unless the row ran OK)."""
    key = (repr(cfg), bytes(row), repr(query), flag_mask, depth, max_launches, runner)
    if key not in _refs:
        try:
            r, faults, launches, mask = pxb.shrink_cover(cfg, row, query, flag_mask, runner=runner,
                                                         max_launches=max_launches, depth=depth)
            st = pxb.SHRINK_BUDGET if (faults and launches % 2 == 1) else pxb.SHRINK_MINIMAL
            _refs[key] = {"status": st, "row": r.copy(), "faults": faults, "launches": launches, "mask": mask}
        except ValueError:
            given = np.array(row, dtype=np.uint8)
            run = runner or pxb._run_cover_runner
            _refs[key] = {"status": pxb.SHRINK_NOT_INPUT, "row": given, "faults": [], "launches": 1,
                          "mask": int(run(cfg, given[None, :], depth)[3][0])}
    return _refs[key]


def check(cfg, o, i, ref, depth):
    """Instance i of the batch outputs `o` equals the reference, bit for bit:
    shrink_oracle.check's fields (status, row, fault list, launches, signature) and the mask."""
    H.check(cfg, o, i, ref, depth)
    assert int(o["masks"][i]) == ref["mask"], (i, hex(int(o["masks"][i])), hex(ref["mask"]))


def one_minimal(cfg, o, query, flag_mask, depth, runner):
    """Every MINIMAL row of `o` holds the predicate by `runner` with the reported
    result, sent and mask, and every single neutralisation of it loses it."""
    q = query if query is not None else pxb.CoverQuery()

    def holds(res, status, sent, masks):
        return [bool(status[i] == pxb.TRACE_OK and (flag_mask == 0 or int(res[i][3]) & 0xFF & flag_mask)
                     and q.matches(int(masks[i])) and int(sent[i].max()) <= depth) for i in range(len(res))]
    keep = [i for i in range(len(o["status"])) if o["status"][i] == pxb.SHRINK_MINIMAL]
    assert keep
    res, status, sent, masks = runner(cfg, o["rows"][keep], depth)
    assert all(holds(res, status, sent, masks))
    assert (res == o["res"][keep]).all() and (np.asarray(sent) == o["sent"][keep]).all()
    assert (np.asarray(masks) == o["masks"][keep]).all()
    cand, owner = [], []
    for i in keep:
        for f in pxb.script_faults(cfg, o["rows"][i], depth, o["sent"][i]):
            r = o["rows"][i].copy()
            pxb.script_neutralise(cfg, r, depth, f)
            cand.append(r)
            owner.append(i)
    assert len(cand) == int(o["n_faults"][keep].sum())
    if cand:
        held = holds(*runner(cfg, np.array(cand), depth))
        assert not any(held), [owner[j] for j, h in enumerate(held) if h]
    return keep
