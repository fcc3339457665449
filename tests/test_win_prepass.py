"""The window pre-pass (csrc/paxos_win.hip): the per-lane kernels load their
instances' isolation windows from the launch's digest rows, where a dense
pre-pass kernel drew them, instead of drawing them in the refill.

Nothing a caller sees may change: results, digests, acceptor records and run
totals are bit-identical to the CPU oracle, and to the same run with
PXB_NO_WIN_PREPASS=1 (the in-kernel draws).  The CPU case checks the pre-pass's
words against EvLane::init's own draws on the host build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_c
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = min(16, os.cpu_count() or 1)
HIGH = (1 << 40) + 12345                     # (the Philox counter's high word set)


def _both(cfg, first, n):
    """GPU run with the pre-pass against the oracle and against the in-kernel draws."""
    got = pxb.run(cfg, first, n, want_acceptors=True)
    want = oracle_c.run_cpu(cfg, first, n, threads=THREADS, want_acceptors=True)
    with pxb.hooks(PXB_NO_WIN_PREPASS="1"):
        drawn = pxb.run(cfg, first, n, want_acceptors=True)
    for name, g, w, d in zip(("results", "digests", "acceptors"), got, want, drawn):
        assert np.array_equal(g, w), "%s differ from the oracle" % name
        assert np.array_equal(g, d), "%s differ from the in-kernel draws" % name
    assert got[3] == want[3] and got[3] == drawn[3]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, HIGH])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4097])
def test_config4_sizes(gpu_lib, n, first):
    """Config 4 (tight routing: layout 7 over the chunk, layout 6 over its
    hand-offs, which reads the rows the one pre-pass left): partial waves,
    partial pre-pass blocks, and the counter's high word."""
    _both(pxb.CONFIGS[4], first, n)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("N", [2, 9])
def test_topologies(gpu_lib, P, N):
    cfg = pxb.Config(seed=0x3170 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000, delay_max=4,
                     skew_max=2, crash_ppm=200000, crash_len_max=16, crash_start_max=8, step_cap=256)
    _both(cfg, 1000, 1025)


@pytest.mark.gpu
@pytest.mark.parametrize("ppm", [0, 200000, 1000000])
def test_crash_rates(gpu_lib, ppm):
    """No window at all (no pre-pass is launched), config 4's rate, every acceptor isolated."""
    c4 = pxb.CONFIGS[4]
    cfg = pxb.Config(seed=c4.seed, n_proposers=2, n_acceptors=7, delay_max=4, crash_ppm=ppm, crash_len_max=16,
                     crash_start_max=8, step_cap=256)
    _both(cfg, 5, 1025)


@pytest.mark.gpu
def test_window_clamp(gpu_lib):
    """crash_start_max 5,000: window starts past step 4095 are clamped to 4096."""
    cfg = pxb.Config(seed=0xC1A, n_proposers=2, n_acceptors=7, delay_max=4, crash_ppm=500000, crash_len_max=4096,
                     crash_start_max=5000, step_cap=256)
    _both(cfg, 9, 1025)


@pytest.mark.gpu
def test_config5_split_routing(gpu_lib):
    """Config 5's fuzzed parameters: every instance's own crash threshold, and
    the P = 3 launch reading the rows of the instances the first launch handed on."""
    pxb.handoff_counts(0)                                # (reset)
    _both(pxb.CONFIGS[5], 0, 2048)
    assert pxb.handoff_counts(0)[0] > 2 * 400            # (two runs; a third of each drew P = 3)


@pytest.mark.gpu
def test_faulty_log_mode(gpu_lib):
    _, _, _, cnt = _both(pxb.LOG_FAULTY_CONFIG, 321, 2048)
    assert cnt["executes"] >= cnt["decided"]


def _device_run(cfg, first, n, digests, stream=None):
    import torch
    N = cfg.n_acceptors
    res = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    dig = torch.zeros((n, N), dtype=torch.int32, device="cuda") if digests else None
    tot = torch.zeros(pxb.NCOUNTERS, dtype=torch.int64, device="cuda")
    pxb.run_device(cfg, first, n, d_results=res, d_digests=dig, d_totals=tot, stream=stream)
    return res, dig, tot


@pytest.mark.gpu
def test_totals_only_run_keeps_the_draws(gpu_lib):
    """Without a digest buffer there are no rows: the refill draws, and the
    results and totals equal those of the run with digests."""
    import torch
    cfg = pxb.CONFIGS[4]
    a = _device_run(cfg, 77, 4097, True)
    b = _device_run(cfg, 77, 4097, False)
    torch.cuda.synchronize()
    assert b[1] is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    _, edig, _, ecnt = oracle_c.run_cpu(cfg, 77, 4097, threads=THREADS)
    assert np.array_equal(a[1].cpu().numpy().view(np.uint32), edig)
    assert pxb.counters_dict(a[2].cpu().tolist()) == ecnt


@pytest.mark.gpu
def test_two_calls_in_flight(gpu_lib):
    """Two calls on two streams, each with its own buffers (so its own rows)."""
    import torch
    cfgs = (pxb.CONFIGS[4], pxb.CONFIGS[5])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for cfg, st in zip(cfgs, streams):
        with torch.cuda.stream(st):
            outs.append(_device_run(cfg, HIGH, 3000, True, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for cfg, (res, dig, tot) in zip(cfgs, outs):
        eres, edig, _, ecnt = oracle_c.run_cpu(cfg, HIGH, 3000, threads=THREADS)
        assert np.array_equal(res.cpu().numpy().view(np.uint32), eres)
        assert np.array_equal(dig.cpu().numpy().view(np.uint32), edig)
        assert pxb.counters_dict(tot.cpu().tolist()) == ecnt


# ---- CPU: the pre-pass's words against EvLane::init's draws (tests/native/win_host.cpp) ----
SRC = os.path.join(HERE, "native", "win_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libwin_host.so")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")]
_lib = None


def win_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            tmp = "%s.%d" % (OUT, os.getpid())          # (parallel workers: build, then rename)
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC",
                            "-shared", "-o", tmp, SRC], check=True)
            os.replace(tmp, OUT)
        _lib = C.CDLL(OUT)
    return _lib


@pytest.mark.parametrize("first", [0, HIGH])
@pytest.mark.parametrize("cfg", [
    pxb.CONFIGS[4],
    pxb.CONFIGS[5],
    pxb.LOG_FAULTY_CONFIG,
    pxb.Config(seed=3, n_proposers=1, n_acceptors=2, delay_max=2, crash_ppm=1000000, crash_len_max=4096,
               crash_start_max=5000),
    pxb.Config(seed=4, n_proposers=3, n_acceptors=9, delay_max=2, crash_ppm=0),
], ids=["config4", "config5", "log_faulty", "clamp", "no_crash"])
def test_prepass_words_equal_init_draws(cfg, first):
    n, N = 1000, cfg.n_acceptors
    rows = np.zeros((n, N), np.uint32)
    drawn = np.zeros((n, N), np.uint32)
    c = cfg.to_c(first, n)
    bad = win_lib().win_host_check(C.byref(c), C.c_void_p(rows.ctypes.data), C.c_void_p(drawn.ctypes.data))
    assert bad == 0
    assert np.array_equal(rows, drawn)
    c0, c1 = rows & 0xFFFF, rows >> 16
    assert (c0 <= 4096).all() and (c1 <= 4096).all()
    if cfg.crash_ppm == 0:
        assert not rows.any()
    else:
        assert rows.any()
        if cfg.crash_start_max > 4096:
            assert (c0 == 4096).any() and (c1 == 4096).any()      # (the clamp is exercised)
