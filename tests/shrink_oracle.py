"""Test-side helpers for the batched shrinker (docs/SEMANTICS.md §11).

* ``host_batch``: the host build of the shrinker's shared logic
  (tests/native/shrink_host.cpp), pxb_shrink_batch's arguments and outputs.
* ``reference``: pxb.shrink for one row as the batch reports it (a status where
  it raises), computed once per (config, row, arguments, runner) and shared.
* ``check``: one instance of a batch against its reference.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import pxb
import script_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "shrink_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libshrink_host.so")
DEPS = [SRC, os.path.join(HERE, "native", "host_lane.h")] + [
    os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", f)
    for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "paxos_trace_core.h", "ev_layouts.h",
              "lane_shapes.h", "script_core.h", "script_lane.h", "shrink_core.h")] + [
                  os.path.join(ROOT, "include", "paxos_batch.h")]
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
        _lib.shrink_host_batch.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32] + [vp] * 6
    return _lib


def host_batch(cfg, instances, flag_mask, depth=64, max_launches=64):
    """shrink_host_batch over ids (1-D) or rows (2-D): a dict of rows, status,
    n_faults, launches, sent, res, sig."""
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
         "res": np.zeros((n, 4), np.uint32), "sig": np.zeros(n, np.uint64)}
    c = cfg.to_c(0, 1)
    rc = lib().shrink_host_batch(C.addressof(c), ids.ctypes.data if ids is not None else None, rows.ctypes.data, n,
                                 depth, flag_mask, max_launches, o["status"].ctypes.data, o["n_faults"].ctypes.data,
                                 o["launches"].ctypes.data, o["sent"].ctypes.data, o["res"].ctypes.data,
                                 o["sig"].ctypes.data)
    assert rc == 0, "shrink_host_batch rc=%d" % rc
    return o


def as_dict(out):
    """pxb.shrink_batch's tuple as host_batch's dict."""
    return dict(zip(("rows", "status", "n_faults", "launches", "sent", "res", "sig"), out))


def reference(cfg, row, flag_mask, depth=64, max_launches=64, runner=None):
    """pxb.shrink(cfg, row, ...) as the batch reports it: {"status", "row",
    "faults", "launches"}.  Where pxb.shrink raises for a row that is no input:
    NOT_INPUT, the row as given, launches 1, no faults.  It returns with faults
    left either before a round (launches odd: the budget) or after a singles
    launch in which none was removable (launches even: 1-minimal)."""
    key = (repr(cfg), bytes(row), flag_mask, depth, max_launches, runner)
    if key not in _refs:
        try:
            r, faults, launches = pxb.shrink(cfg, row, flag_mask, runner=runner, max_launches=max_launches, depth=depth)
            st = pxb.SHRINK_BUDGET if (faults and launches % 2 == 1) else pxb.SHRINK_MINIMAL
            _refs[key] = {"status": st, "row": r.copy(), "faults": faults, "launches": launches}
        except ValueError:
            _refs[key] = {"status": pxb.SHRINK_NOT_INPUT, "row": np.array(row, dtype=np.uint8), "faults": [],
                          "launches": 1}
    return _refs[key]


def check(cfg, o, i, ref, depth):
    """Instance i of the batch outputs `o` equals the reference, bit for bit:
    status, row, fault list, launches; and the signature is the Python one."""
    assert int(o["status"][i]) == ref["status"], (i, int(o["status"][i]), ref["status"])
    assert int(o["launches"][i]) == ref["launches"], (i, int(o["launches"][i]), ref["launches"])
    assert (o["rows"][i] == ref["row"]).all(), i
    assert int(o["n_faults"][i]) == len(ref["faults"]), (i, int(o["n_faults"][i]), len(ref["faults"]))
    if ref["status"] == pxb.SHRINK_NOT_INPUT:
        assert not o["sent"][i].any() and int(o["sig"][i]) == 0, i
        return
    assert pxb.script_faults(cfg, o["rows"][i], depth, o["sent"][i]) == ref["faults"], i
    assert int(o["sig"][i]) == pxb.script_signature(cfg, o["rows"][i], depth, o["sent"][i]), i
