"""CPU-side checks of the result queries (pxb_query_device, pxb_sweep): the
struct layout against the header, the argument validation (before any device
call, so on every host), the Python wrappers' buffer checks, and the chunk
arithmetic of a sweep (csrc/sweep_plan.h) through a stand-alone program."""
import ctypes as C
import os
import subprocess

import pytest

import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "paxos_batch.h")
PLAN_SRC = os.path.join(HERE, "native", "sweep_plan_host.cpp")
PLAN_HDR = os.path.join(ROOT, "cloud-haskell-paxos_amd", "csrc", "sweep_plan.h")
PLAN_BIN = os.path.join(HERE, "native", "_build", "sweep_plan_host")


def test_query_struct_layout_matches_header(tmp_path):
    fields = [f for f, _ in pxb.pxb_query._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "paxos_batch.h"\nint main(void) {\n'
           '  printf("%zu %d %u %u %u", sizeof(pxb_query), PXB_HIST_MAX_BINS, PXB_Q_ANY, PXB_Q_ALL, PXB_Q_NONE);\n'
           + "".join('  printf(" %%zu", offsetof(pxb_query, %s));\n' % f for f in fields)
           + "  return 0;\n}\n")
    tmp = str(tmp_path / "pxb_query_layout")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", tmp, tmp + ".c"], check=True)
    got = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32 == C.sizeof(pxb.pxb_query)
    assert got[1:5] == [pxb.HIST_MAX_BINS, pxb.Q_ANY, pxb.Q_ALL, pxb.Q_NONE] == [8194, 0, 1, 2]
    assert got[5:] == [getattr(pxb.pxb_query, f).offset for f in fields] == [4 * k for k in range(8)]
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY, steps_min=1, steps_max=2, rounds_min=3,
                  rounds_max=4, n_bins_steps=5, n_bins_rounds=6).to_c()
    assert list(C.cast(C.byref(q), C.POINTER(C.c_uint32))[:8]) == [4, 0, 1, 2, 3, 4, 5, 6]
    assert pxb.Query().to_c().steps_max == 0xFFFFFFFF and pxb.Query().flag_mode == pxb.Q_NONE


# The pointers are never followed: every case fails validation first.
P = C.c_void_p(0x1000)


def _query_rc(q, ids=P, capacity=4, n_matches=P, hs=None, hr=None, results=P, count=16):
    return pxb.load().pxb_query_device(results, 0, count, C.byref(q) if q is not None else None, ids, None, capacity,
                                       n_matches, hs, hr, None)


def _sweep_rc(q, ids=P, capacity=4, n_matches=P, hs=None, hr=None, cfg=None):
    c = (cfg or pxb.CONFIGS[3]).to_c(0, 64)
    return pxb.load().pxb_sweep(C.byref(c), C.byref(q) if q is not None else None, ids, None, capacity, n_matches,
                                hs, hr, None)


BAD = {
    "null q": dict(q=None),
    "flag_mode 3": dict(q=pxb.Query(flag_mode=3)),
    "flag_mask 0x100": dict(q=pxb.Query(flag_mask=0x100)),
    "steps bins above the maximum": dict(q=pxb.Query(n_bins_steps=pxb.HIST_MAX_BINS + 1), hs=P),
    "rounds bins above the maximum": dict(q=pxb.Query(n_bins_rounds=pxb.HIST_MAX_BINS + 1), hr=P),
    "null ids with capacity": dict(q=pxb.Query(), ids=None, capacity=1),
    "null steps histogram with bins": dict(q=pxb.Query(n_bins_steps=4), hs=None),
    "null rounds histogram with bins": dict(q=pxb.Query(n_bins_rounds=4), hr=None),
    "null n_matches": dict(q=pxb.Query(), n_matches=None),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_query_device_validation(case):
    kw = dict(BAD[case])
    q = kw.pop("q")
    assert _query_rc(q.to_c() if q is not None else None, **kw) == pxb.PXB_E_INVAL


@pytest.mark.parametrize("case", sorted(BAD))
def test_sweep_validation(case):
    kw = dict(BAD[case])
    q = kw.pop("q")
    assert _sweep_rc(q.to_c() if q is not None else None, **kw) == pxb.PXB_E_INVAL


def test_more_validation():
    q = pxb.Query().to_c()
    assert _query_rc(q, results=None, count=1) == pxb.PXB_E_INVAL           # results needed when count > 0
    assert _query_rc(q, results=C.c_void_p(0x1004)) == pxb.PXB_E_INVAL      # records move as 16-B words
    assert _query_rc(q, count=(1 << 40) + 1) == pxb.PXB_E_INVAL
    # count == 0 with legal arguments is a no-op, histogram-only (null ids) included
    assert _query_rc(q, count=0) == pxb.PXB_OK
    assert _query_rc(q, ids=None, capacity=0, count=0, results=None) == pxb.PXB_OK
    assert _sweep_rc(q, cfg=pxb.Config(seed=1, n_proposers=4)) == pxb.PXB_E_INVAL   # pxb_run's own rules
    assert pxb.load().pxb_sweep(None, C.byref(q), P, None, 4, P, None, None, None) == pxb.PXB_E_INVAL


def test_sweep_without_gpu_is_nodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    ids = np.zeros(4, np.uint64)
    nm = C.c_uint64(7)
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY).to_c()
    c = pxb.CONFIGS[3].to_c(0, 64)
    assert pxb.load().pxb_sweep(C.byref(c), C.byref(q), C.c_void_p(ids.ctypes.data), None, 4, C.byref(nm), None,
                                None, None) == pxb.PXB_E_NODEV
    with pytest.raises(pxb.PaxosError, match="no GPU"):
        pxb.sweep(pxb.CONFIGS[3], 0, 64, pxb.Query(), 4)


def test_query_device_checks_buffers_before_the_abi():
    import torch
    n, cap = 100, 10
    q = pxb.Query(n_bins_steps=16)
    with pytest.raises(ValueError, match="CUDA"):
        pxb.query_device(torch.zeros((n, 4), dtype=torch.int32), 0, n, pxb.Query(), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="required"):
        pxb.query_device(None, 0, 0, pxb.Query(), None)

    class Fake:   # a stand-in for a device tensor (no GPU here)
        def __init__(self, numel, size=4, contiguous=True):
            self.is_cuda, self._n, self._s, self._c = True, numel, size, contiguous
            self.dtype = torch.int32 if size == 4 else torch.int64

        def element_size(self):
            return self._s

        def is_contiguous(self):
            return self._c

        def numel(self):
            return self._n

    ok = dict(d_results=Fake(4 * n), first_instance=0, count=n, query=q, d_n_matches=Fake(1, 8), d_ids=Fake(cap, 8),
              d_matched=Fake(4 * cap), capacity=cap, d_hist_steps=Fake(16, 8))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            pxb.query_device(**{**ok, **kw})
    bad("needed", d_results=Fake(4 * n - 1))
    bad("integer", d_results=Fake(4 * n, 8))
    bad("integer", d_results=Fake(4 * n, 4, False))
    bad("CUDA", d_n_matches=torch.zeros(1, dtype=torch.int64))
    bad("integer", d_n_matches=Fake(1, 4))
    bad("needed", d_ids=Fake(cap - 1, 8))
    bad("integer", d_ids=Fake(cap, 4))
    bad("required", d_ids=None)
    bad("needed", d_matched=Fake(4 * cap - 1))
    bad("needed", d_hist_steps=Fake(15, 8))
    bad("integer", d_hist_steps=Fake(16, 4))
    bad("required", d_hist_steps=None)
    bad("required", query=pxb.Query(n_bins_steps=16, n_bins_rounds=8))


def _plan(first, n, chunk_value):
    if not os.path.exists(PLAN_BIN) or max(os.path.getmtime(PLAN_SRC), os.path.getmtime(PLAN_HDR)) > os.path.getmtime(PLAN_BIN):
        os.makedirs(os.path.dirname(PLAN_BIN), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", PLAN_BIN, PLAN_SRC], check=True)
    out = subprocess.run([PLAN_BIN, str(first), str(n), str(chunk_value)], capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return int(out[0]), [tuple(int(x) for x in line.split()) for line in out[1:] if line]


def _expected(first, n, chunk):
    return [(first + k, min(chunk, n - k)) for k in range(0, n, chunk)]


@pytest.mark.parametrize("chunk", [1, 4096, 1 << 24])
def test_sweep_chunk_plan(chunk):
    for first, n in ((0, 0), (7, 1), (0, chunk), (3, chunk + 1), ((1 << 32) - 5000, 20000)):
        got_chunk, chunks = _plan(first, n, chunk)
        assert got_chunk == chunk
        assert chunks == _expected(first, n, chunk), (first, n)
        # restated: contiguous from `first`, full chunks but for a ragged last one, n covered exactly
        assert sum(c for _, c in chunks) == n and len(chunks) == -(-n // chunk)
        assert all(c == chunk for _, c in chunks[:-1]) and all(0 < c <= chunk for _, c in chunks)
        at = first
        for f, c in chunks:
            assert f == at
            at += c
    if chunk == 4096:   # the GPU test's sweep: five chunks, the 2^32 crossing inside the second
        _, chunks = _plan((1 << 32) - 5000, 20000, chunk)
        assert chunks == [(4294962296, 4096), (4294966392, 4096), (4294970488, 4096), (4294974584, 4096),
                          (4294978680, 3616)]


def test_sweep_chunk_hook_is_clamped():
    assert _plan(0, 10, 0)[0] == 1 and _plan(0, 10, -5)[0] == 1
    assert _plan(0, 10, 1 << 30)[0] == (1 << 30) - 1 and _plan(0, 10, (1 << 30) - 1)[0] == (1 << 30) - 1
    # the hook goes through the library's hook mechanism (no GPU call)
    with pxb.hooks(PXB_SWEEP_CHUNK=4096):
        assert os.environ["PXB_SWEEP_CHUNK"] == "4096"
    assert "PXB_SWEEP_CHUNK" not in os.environ
