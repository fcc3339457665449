"""Python host binding of the batched Paxos C ABI (include/paxos_batch.h).

This is the host side above the C-ABI for environments without GHC (the
reference's own host is Haskell: /root/reference/app/Main.hs; the Haskell
binding a maintainer would add lives in hs/ and INTEGRATION.md).  It mirrors
the reference's vocabulary (/root/reference/src/Common.hs:20-68): ``Ticket``,
``Command`` ("c<clientId>.<t>", Client.hs:202-203), ``Proposal``,
``ClientRequest`` / ``ServerResponse`` constructors.

The product path is ``libpaxos_batch.so`` (HIP kernels for gfx950).  There is
NO CPU fallback here: when the library (or a GPU) is missing every entry point
raises.  The CPU restatement used as test oracle lives in ``oracle/`` and is
never imported by this module.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import os
from dataclasses import dataclass
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PXB_LIB") or os.path.join(_HERE, "csrc", "libpaxos_batch.so")

# ---- constants (include/paxos_batch.h) ------------------------------------
PXB_OK, PXB_E_INVAL, PXB_E_HIP, PXB_E_OOM, PXB_E_NODEV, PXB_E_RCCL = 0, -1, -2, -3, -4, -5
MAX_PROPOSERS, MIN_ACCEPTORS, MAX_ACCEPTORS = 3, 2, 9
MAX_DELAY, MAX_STEP_CAP, QUEUE_DEPTH, LOG_TRACK, MAX_TICKS = 15, 8192, 8, 32, 4096
CFG_RANDOMIZE = 1
CFG_TRACE_PRODUCTION = 2         # pxb_trace_instance: the batch kernels' carry-over variant
TRACE_IN_FLIGHT_UNKNOWN = 0xFFFFFFFF

F_UNDECIDED, F_STUCK, F_PANIC, F_LOG_DIVERGENCE = 1, 2, 4, 8
F_STEP_CAP, F_QUEUE_OVERFLOW, F_TICKET_OVERFLOW, F_LOG_TRUNC = 16, 32, 64, 128
FLAG_NAMES = {F_UNDECIDED: "UNDECIDED", F_STUCK: "STUCK", F_PANIC: "PANIC",
              F_LOG_DIVERGENCE: "LOG_DIVERGENCE", F_STEP_CAP: "STEP_CAP",
              F_QUEUE_OVERFLOW: "QUEUE_OVERFLOW", F_TICKET_OVERFLOW: "TICKET_OVERFLOW",
              F_LOG_TRUNC: "LOG_TRUNC"}

NCOUNTERS = 16
COUNTER_NAMES = ["decided", "undecided", "stuck", "panic", "divergence", "step_cap",
                 "rounds", "messages", "queue_overflow", "ticket_overflow", "log_trunc",
                 "canon_bytes", "steps", "instances", "executes", "reserved15"]

# ClientRequest (Common.hs:41-45) / ServerResponse (Common.hs:49-53) tags
AskForTicket, Propose, Execute = 0, 1, 2
Round1OK, HaveTicket, Round2Success = 0, 1, 2
Tick = 3
MSG_NONE = 0xFFFFFFFF
Idle, Round1, Round2 = 0, 1, 2


class pxb_config(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_instance", C.c_uint64),
                ("n_instances", C.c_uint64), ("n_proposers", C.c_uint32),
                ("n_acceptors", C.c_uint32), ("loss_ppm", C.c_uint32),
                ("delay_max", C.c_uint32), ("crash_ppm", C.c_uint32),
                ("crash_len_max", C.c_uint32), ("crash_start_max", C.c_uint32),
                ("skew_max", C.c_uint32), ("step_cap", C.c_uint32), ("flags", C.c_uint32),
                ("n_ticks", C.c_uint32), ("tick_period", C.c_uint32)]


class pxb_result(C.Structure):
    _fields_ = [("decided_val", C.c_uint32), ("decided_ticket", C.c_int32),
                ("rounds", C.c_uint32), ("flags", C.c_uint32)]


class pxb_acceptor_rec(C.Structure):
    _fields_ = [("t_max", C.c_int32), ("t_store", C.c_int32), ("val", C.c_uint32),
                ("meta", C.c_uint32)]


class pxb_counters(C.Structure):
    _fields_ = [("c", C.c_int64 * NCOUNTERS)]


class pxb_msg(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("x", C.c_int32), ("y", C.c_int32), ("z", C.c_uint32)]


class pxb_proposer_rec(C.Structure):
    _fields_ = [("ticket", C.c_int32), ("cmd", C.c_uint32), ("acks", C.c_uint32),
                ("state", C.c_uint32), ("mr_t", C.c_int32), ("mr_v", C.c_uint32),
                ("r2_t", C.c_int32), ("r2_v", C.c_uint32), ("pending", C.c_uint32),
                ("client_id", C.c_uint32)]


class pxb_query(C.Structure):
    _fields_ = [("flag_mask", C.c_uint32), ("flag_mode", C.c_uint32),
                ("steps_min", C.c_uint32), ("steps_max", C.c_uint32),
                ("rounds_min", C.c_uint32), ("rounds_max", C.c_uint32),
                ("n_bins_steps", C.c_uint32), ("n_bins_rounds", C.c_uint32)]


class pxb_trace_sel(C.Structure):
    _fields_ = [("step_min", C.c_uint32), ("step_max", C.c_uint32), ("tail", C.c_uint32),
                ("reserved", C.c_uint32)]


class pxb_explore_space(C.Structure):
    _fields_ = [("site_depth", C.c_uint32), ("radius", C.c_uint32), ("flag_mask", C.c_uint32),
                ("flags", C.c_uint32)]


assert C.sizeof(pxb_explore_space) == 16
assert C.sizeof(pxb_config) == 72 and C.sizeof(pxb_result) == 16 and C.sizeof(pxb_trace_sel) == 16
assert C.sizeof(pxb_acceptor_rec) == 16 and C.sizeof(pxb_msg) == 16
assert C.sizeof(pxb_query) == 32

# pxb_query.flag_mode / histogram bound
Q_ANY, Q_ALL, Q_NONE = 0, 1, 2
HIST_MAX_BINS = 8194
U32_MAX = 0xFFFFFFFF


@dataclass
class Query:
    """pxb_query: the flag test (flags & flag_mask against Q_ANY / Q_ALL /
    Q_NONE), inclusive ranges on the steps and the rounds, and the number of
    bins of the two histograms (0 = none).  The default matches everything."""
    flag_mask: int = 0
    flag_mode: int = Q_NONE
    steps_min: int = 0
    steps_max: int = U32_MAX
    rounds_min: int = 0
    rounds_max: int = U32_MAX
    n_bins_steps: int = 0
    n_bins_rounds: int = 0

    def to_c(self) -> pxb_query:
        return pxb_query(self.flag_mask, self.flag_mode, self.steps_min, self.steps_max,
                         self.rounds_min, self.rounds_max, self.n_bins_steps, self.n_bins_rounds)

# ---- Common.hs vocabulary ------------------------------------------------


def command(client_id: int, t: int) -> int:
    """Encode the Command "c<clientId>.<t>" (Client.hs:202-203)."""
    return ((client_id & 0xFF) << 24) | (t & 0xFFFFFF)


def command_str(code: int) -> Optional[str]:
    """Decode a Command code back into the reference's String (None = Nothing)."""
    if code == 0:
        return None
    return "c%d.%d" % (code >> 24, code & 0xFFFFFF)


def flag_names(flags: int):
    return [n for b, n in FLAG_NAMES.items() if flags & b]


# ---- named configurations (BASELINE.json configs) -------
@dataclass
class Config:
    seed: int
    n_proposers: int = 1
    n_acceptors: int = 5
    loss_ppm: int = 0
    delay_max: int = 1
    crash_ppm: int = 0
    crash_len_max: int = 1
    crash_start_max: int = 0
    skew_max: int = 0
    step_cap: int = 256
    randomize: bool = False
    n_ticks: int = 1          # log mode when > 1: Ticks per proposer (Client.hs:96-100)
    tick_period: int = 1      # steps between Ticks

    def to_c(self, first_instance: int, n_instances: int) -> pxb_config:
        return pxb_config(self.seed, first_instance, n_instances, self.n_proposers,
                          self.n_acceptors, self.loss_ppm, self.delay_max, self.crash_ppm,
                          self.crash_len_max, self.crash_start_max, self.skew_max,
                          self.step_cap, CFG_RANDOMIZE if self.randomize else 0,
                          self.n_ticks, self.tick_period)


CONFIGS = {
    1: Config(seed=0x5EED0001, n_proposers=1, n_acceptors=3),
    2: Config(seed=0x5EED0002, n_proposers=1, n_acceptors=5),
    3: Config(seed=0x5EED0003, n_proposers=2, n_acceptors=5, loss_ppm=100000,
              delay_max=4, skew_max=3, step_cap=256),
    4: Config(seed=0x5EED0004, n_proposers=2, n_acceptors=7, delay_max=4,
              crash_ppm=200000, crash_len_max=16, crash_start_max=8, step_cap=256),
    5: Config(seed=0x5EED0005, n_proposers=3, n_acceptors=9, loss_ppm=300000,
              delay_max=8, crash_ppm=200000, crash_len_max=16, crash_start_max=16,
              skew_max=3, step_cap=512, randomize=True),
}
CONFIG_INSTANCES = {1: 1 << 10, 2: 1 << 20, 3: 1 << 24, 4: 1 << 26, 5: 1 << 28, 6: 1 << 20, 7: 1 << 20}

# Log mode (docs/SEMANTICS.md §9): the stock app/Main.hs
# topology (2 proposers, 2 acceptors, Main.hs:41-46) with the ticker running
# (Client.hs:96-100): 16 Ticks per proposer, 8 steps apart.
LOG_CONFIG = Config(seed=0x5EED0006, n_proposers=2, n_acceptors=2, step_cap=1024,
                    n_ticks=16, tick_period=8)
CONFIGS[6] = LOG_CONFIG
# Faulty log mode: config 3's duel and loss with crash windows, 16 Ticks per
# proposer (the per-lane kernel's log-mode shape; bench.py extra.log_mode_faulty)
LOG_FAULTY_CONFIG = Config(seed=0x5EED0007, n_proposers=2, n_acceptors=5, loss_ppm=100000, delay_max=4,
                           skew_max=3, crash_ppm=200000, crash_len_max=16, crash_start_max=64, step_cap=1024,
                           n_ticks=16, tick_period=8)
CONFIGS[7] = LOG_FAULTY_CONFIG


def canonical_bytes_nofault(n_acceptors: int) -> int:
    """B = 196 N + 160 for a fault-free P = 1 instance."""
    return 196 * n_acceptors + 160


# ---- library loading --------------------------------------------------------
_lib = None
ABI_VERSION = 5          # PXB_ABI_VERSION of include/paxos_batch.h this mirror binds


class PaxosError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load libpaxos_batch.so.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise PaxosError("libpaxos_batch.so not built at %s — run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.pxb_run.argtypes = [C.POINTER(pxb_config), vp, vp, vp, vp]
    lib.pxb_run.restype = C.c_int
    lib.pxb_run_device.argtypes = [C.POINTER(pxb_config), vp, vp, vp, vp, vp]
    lib.pxb_run_device.restype = C.c_int
    lib.pxb_run_multi.argtypes = [C.POINTER(pxb_config), C.c_int, vp, vp, vp, vp]
    lib.pxb_run_multi.restype = C.c_int
    lib.pxb_acceptor_handle.argtypes = [vp, vp, vp, C.c_uint32]
    lib.pxb_acceptor_handle.restype = C.c_int
    lib.pxb_proposer_handle.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32]
    lib.pxb_proposer_handle.restype = C.c_int
    lib.pxb_strerror.argtypes = [C.c_int]
    lib.pxb_strerror.restype = C.c_char_p
    lib.pxb_last_hip_error.restype = C.c_int
    lib.pxb_abi_version.restype = C.c_int
    lib.pxb_canonical_bytes_nofault.argtypes = [C.c_uint32]
    lib.pxb_canonical_bytes_nofault.restype = C.c_uint64
    for name, args in (("pxb_wire_size", [vp, C.c_uint64, C.c_uint32, vp, vp]),
                       ("pxb_wire_encode", [vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
                       ("pxb_wire_encode_all", [vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
                       ("pxb_wire_decode", [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
                       ("pxb_wire_encode_host", [vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
                       ("pxb_wire_decode_host", [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp]),
                       ("pxb_init", [C.c_int]), ("pxb_shutdown", []),
                       ("pxb_trace_instance", [vp, C.c_uint64, vp, C.c_uint32, vp, vp]),
                       ("pxb_query_device", [vp, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_sweep", [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_trace_batch_device", [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_trace_batch", [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_schedule_extract_device", [vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
                       ("pxb_schedule_extract", [vp, vp, C.c_uint64, C.c_uint32, vp]),
                       ("pxb_run_scripted_device", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp]),
                       ("pxb_run_scripted", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]),
                       ("pxb_trace_scripted_device",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_trace_scripted",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_trace_events_device",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_trace_events",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_cover_device", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]),
                       ("pxb_cover", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
                       ("pxb_cover_range", [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint64, vp]),
                       ("pxb_shrink_batch_device",
                        [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
                       ("pxb_shrink_batch",
                        [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]),
                       ("pxb_explore_row", [vp, C.c_uint32, vp, vp, C.c_uint64, vp]),
                       ("pxb_explore_device",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_explore", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp]),
                       ("pxb_explore_cover_device",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp]),
                       ("pxb_explore_cover", [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
                       ("pxb_shrink_cover_batch_device",
                        [vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("pxb_shrink_cover_batch",
                        [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    lib.pxb_explore_total.argtypes = [C.c_uint32] * 5
    lib.pxb_explore_total.restype = C.c_uint64
    lib.pxb_script_stride.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.pxb_script_stride.restype = C.c_uint64
    lib.pxb_stream_release.argtypes = [C.c_int, vp]
    lib.pxb_stream_release.restype = None
    lib.pxb_handoff_counts.argtypes = [C.c_int, vp, C.c_int]
    lib.pxb_handoff_counts.restype = C.c_int
    lib.pxb_reload_hooks.argtypes = []
    lib.pxb_reload_hooks.restype = None
    if lib.pxb_abi_version() != ABI_VERSION:          # (a stale build: its struct layouts may differ)
        raise PaxosError("libpaxos_batch.so has ABI %d, this binding expects %d — rebuild it"
                         % (lib.pxb_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int):
    if rc != PXB_OK:
        lib = load()
        raise PaxosError("pxb error %d: %s (hip %d)" % (rc, lib.pxb_strerror(rc).decode(),
                                                         lib.pxb_last_hip_error()))


def _ptr(a):
    """Address of a numpy array / torch tensor / None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def run(cfg: Config, first_instance: int, n_instances: int, want_results=True,
        want_digests=True, want_acceptors=False):
    """Host-buffer batch run (pxb_run).  Returns numpy arrays + counters dict."""
    import numpy as np
    lib = load()
    N = cfg.n_acceptors
    res = np.zeros((n_instances, 4), dtype=np.uint32) if want_results else None
    dig = np.zeros((n_instances, N), dtype=np.uint32) if want_digests else None
    acc = np.zeros((n_instances, N, 4), dtype=np.uint32) if want_acceptors else None
    tot = pxb_counters()
    c = cfg.to_c(first_instance, n_instances)
    check(lib.pxb_run(C.byref(c), _ptr(res), _ptr(dig), _ptr(acc), C.cast(C.byref(tot), C.c_void_p)))
    return res, dig, acc, counters_dict(tot.c)


def run_multi(cfg: Config, first_instance: int, n_instances: int, n_devices: int = 0,
              want_results=True, want_digests=True):
    """Host-buffer batch sharded over devices 0..n_devices-1 (pxb_run_multi):
    one thread per GPU, one RCCL all-reduce of the run totals."""
    import numpy as np
    lib = load()
    N = cfg.n_acceptors
    res = np.zeros((n_instances, 4), dtype=np.uint32) if want_results else None
    dig = np.zeros((n_instances, N), dtype=np.uint32) if want_digests else None
    tot = pxb_counters()
    c = cfg.to_c(first_instance, n_instances)
    check(lib.pxb_run_multi(C.byref(c), n_devices, _ptr(res), _ptr(dig), None,
                            C.cast(C.byref(tot), C.c_void_p)))
    return res, dig, counters_dict(tot.c)


def _check_buf(name, t, words, itemsize):
    """A device output buffer must be a contiguous GPU tensor of 4-byte (or, for
    the totals, 8-byte) integers holding at least `words` elements: the kernels
    write through its raw address."""
    if t is None:
        return
    if not getattr(t, "is_cuda", False):
        raise ValueError("%s: a CUDA (HIP) tensor is required" % name)
    if t.element_size() != itemsize or t.dtype.is_floating_point or not t.is_contiguous():
        raise ValueError("%s: contiguous %d-byte integer tensor required" % (name, itemsize))
    if t.numel() < words:
        raise ValueError("%s: %d elements, %d needed" % (name, t.numel(), words))


def _check_bytes(name, t, nbytes):
    """A device byte buffer: contiguous GPU uint8 tensor of at least nbytes
    (its element count is the byte bound handed to the C ABI)."""
    import torch
    if not getattr(t, "is_cuda", False):
        raise ValueError("%s: a CUDA (HIP) tensor is required" % name)
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError("%s: contiguous uint8 tensor required" % name)
    if t.numel() < nbytes:
        raise ValueError("%s: %d bytes, %d needed" % (name, t.numel(), nbytes))


def run_device(cfg: Config, first_instance: int, n_instances: int, d_results=None,
               d_digests=None, d_acceptors=None, d_totals=None, stream=None):
    """Device-buffer, asynchronous batch run (pxb_run_device) on torch tensors
    (sizes and dtypes checked here: the C ABI takes raw pointers)."""
    N = cfg.n_acceptors
    _check_buf("d_results", d_results, 4 * n_instances, 4)
    _check_buf("d_digests", d_digests, N * n_instances, 4)
    _check_buf("d_acceptors", d_acceptors, 4 * N * n_instances, 4)
    if d_totals is None:
        raise ValueError("d_totals is required")
    _check_buf("d_totals", d_totals, NCOUNTERS, 8)
    lib = load()
    c = cfg.to_c(first_instance, n_instances)
    s = C.c_void_p(stream) if stream else None
    check(lib.pxb_run_device(C.byref(c), _ptr(d_results), _ptr(d_digests), _ptr(d_acceptors),
                             _ptr(d_totals), s))


def query_device(d_results, first_instance: int, count: int, query: Query, d_n_matches, d_ids=None,
                 d_matched=None, capacity: int = 0, d_hist_steps=None, d_hist_rounds=None, stream=None):
    """pxb_query_device on torch tensors, asynchronous on `stream`: applies
    `query` to d_results[:count] (int32 (count, 4), the results of instances
    first_instance..).  Matching global ids go to d_ids (int64, `capacity`
    entries) and their records to d_matched (int32 (capacity, 4), optional) in
    ascending order from the cursor d_n_matches (int64, one entry), which then
    has the call's full match count added; the histograms (int64, n_bins
    entries) are added to.  Sizes and dtypes are checked here: the C ABI takes
    raw pointers."""
    if d_n_matches is None:
        raise ValueError("d_n_matches is required")
    if count and d_results is None:
        raise ValueError("d_results is required")
    if capacity and d_ids is None:
        raise ValueError("d_ids is required when capacity > 0")
    if (query.n_bins_steps and d_hist_steps is None) or (query.n_bins_rounds and d_hist_rounds is None):
        raise ValueError("a histogram buffer is required when its n_bins > 0")
    _check_buf("d_results", d_results, 4 * count, 4)
    _check_buf("d_n_matches", d_n_matches, 1, 8)
    _check_buf("d_ids", d_ids, capacity, 8)
    _check_buf("d_matched", d_matched, 4 * capacity, 4)
    _check_buf("d_hist_steps", d_hist_steps, query.n_bins_steps, 8)
    _check_buf("d_hist_rounds", d_hist_rounds, query.n_bins_rounds, 8)
    lib = load()
    q = query.to_c()
    s = C.c_void_p(stream) if stream else None
    check(lib.pxb_query_device(_ptr(d_results), first_instance, count, C.byref(q), _ptr(d_ids), _ptr(d_matched),
                               capacity, _ptr(d_n_matches), _ptr(d_hist_steps), _ptr(d_hist_rounds), s))


def sweep(cfg: Config, first_instance: int, n_instances: int, query: Query, capacity: int):
    """pxb_sweep: run n_instances instances chunk by chunk and query every
    chunk on the device; only the match list, the bins and the totals come
    back.  Returns (ids uint64 (k,), matched uint32 (k, 4), n_matches,
    hist_steps int64 (n_bins_steps,), hist_rounds int64 (n_bins_rounds,),
    counters dict) with k = min(n_matches, capacity): the k smallest matching
    ids; n_matches is the full count."""
    import numpy as np
    lib = load()
    ids = np.zeros(capacity, dtype=np.uint64)
    matched = np.zeros((capacity, 4), dtype=np.uint32)
    hs = np.zeros(query.n_bins_steps, dtype=np.int64)
    hr = np.zeros(query.n_bins_rounds, dtype=np.int64)
    nm = C.c_uint64(0)
    tot = pxb_counters()
    c = cfg.to_c(first_instance, n_instances)
    q = query.to_c()
    check(lib.pxb_sweep(C.byref(c), C.byref(q), _ptr(ids) if capacity else None, _ptr(matched) if capacity else None,
                        capacity, C.byref(nm), _ptr(hs) if len(hs) else None, _ptr(hr) if len(hr) else None,
                        C.cast(C.byref(tot), C.c_void_p)))
    k = min(nm.value, capacity)
    return ids[:k], matched[:k], nm.value, hs, hr, counters_dict(tot.c)


def counters_dict(c) -> dict:
    return {COUNTER_NAMES[i]: int(c[i]) for i in range(NCOUNTERS)}


def acceptor_handle(states, msgs):
    """GPU hook: handleClientRequest (Server.hs:51-78) on arrays of
    pxb_acceptor_rec / pxb_msg (numpy uint32 views, shape (n, 4))."""
    import numpy as np
    lib = load()
    n = len(states)
    reply = np.zeros((n, 4), dtype=np.uint32)
    check(lib.pxb_acceptor_handle(_ptr(states), _ptr(msgs), _ptr(reply), n))
    return reply


def proposer_handle(states, n_acceptors, msgs):
    """GPU hook: handleServerResponse / handleTick (Client.hs:125-207) on
    arrays of pxb_proposer_rec (uint32 (n,10)) / pxb_msg (uint32 (n,4))."""
    import numpy as np
    lib = load()
    n = len(states)
    bc = np.zeros((n, 2, 4), dtype=np.uint32)
    nb = np.zeros(n, dtype=np.uint32)
    check(lib.pxb_proposer_handle(_ptr(states), n_acceptors, _ptr(msgs), _ptr(bc), _ptr(nb), n))
    return bc, nb


# ---- wire format (include/paxos_batch.h) ------------------
WIRE_REQUEST, WIRE_RESPONSE, WIRE_MAX_BYTES = 0, 1, 39
WIRE_OK, WIRE_E_LENGTH, WIRE_E_TAG, WIRE_E_STRING, WIRE_E_RANGE = 0, 1, 2, 3, 4


def wire_encode(msgs, wire_type):
    """Data.Binary encoding (Common.hs:24,47,55) of pxb_msg records
    (numpy uint32 (n, 4)) on the GPU.  Returns (bytes, offsets[n + 1])."""
    import numpy as np
    lib = load()
    msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
    n = len(msgs)
    out = np.zeros(max(1, n * WIRE_MAX_BYTES), dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    nb = C.c_uint64(0)
    check(lib.pxb_wire_encode_host(_ptr(msgs), n, wire_type, _ptr(out), _ptr(offs), C.byref(nb)))
    return out[:nb.value].tobytes(), offs


def wire_encode_device(d_msgs, wire_type, d_offsets, d_bytes, stream=None):
    """Fused size + encode on device tensors (pxb_wire_encode_all): d_msgs
    int32 (n, 4), d_offsets int64 (n + 1), d_bytes uint8 (n * WIRE_MAX_BYTES),
    asynchronous on `stream` (a raw hipStream_t handle, default stream if None)."""
    n = d_msgs.shape[0]
    _check_buf("d_msgs", d_msgs, 4 * n, 4)
    _check_bytes("d_bytes", d_bytes, max(1, n * WIRE_MAX_BYTES))
    _check_buf("d_offsets", d_offsets, n + 1, 8)
    lib = load()
    check(lib.pxb_wire_encode_all(C.c_void_p(d_msgs.data_ptr()), n, wire_type, C.c_void_p(d_offsets.data_ptr()),
                                  C.c_void_p(d_bytes.data_ptr()), C.c_void_p(stream or 0)))


def wire_decode_device(d_bytes, d_offsets, n, wire_type, d_msgs, d_status=None, stream=None):
    """pxb_wire_decode on device tensors: d_bytes uint8 (its whole length is the
    buffer bound), d_offsets int64 (n + 1), d_msgs int32 (n, 4), d_status int32
    (n,) or None; asynchronous on `stream` (raw hipStream_t, default if None)."""
    _check_bytes("d_bytes", d_bytes, 1)
    _check_buf("d_offsets", d_offsets, n + 1, 8)
    _check_buf("d_msgs", d_msgs, 4 * n, 4)
    _check_buf("d_status", d_status, n, 4)
    lib = load()
    check(lib.pxb_wire_decode(C.c_void_p(d_bytes.data_ptr()), d_bytes.numel(), C.c_void_p(d_offsets.data_ptr()), n,
                              wire_type, C.c_void_p(d_msgs.data_ptr()),
                              C.c_void_p(d_status.data_ptr() if d_status is not None else 0), C.c_void_p(stream or 0)))


TRACE_WORDS = 4 + 9 * 4 + 9 + 3 * 8      # pxb_trace_step, uint32 words


def trace_instance(cfg: Config, instance: int, max_records: int = 8192, production: bool = False):
    """pxb_trace_instance: the state at the end of every visited step of one
    instance, as a list of dicts (step, in_flight, acc (N, 4), digest (N,),
    prop (P, 8): ticket, cmd, acks, state, mr_t, mr_v, r2_v, pending), and its
    pxb_result.  production=True traces the batch kernels' carry-over variant
    (PXB_CFG_TRACE_PRODUCTION; in_flight may be TRACE_IN_FLIGHT_UNKNOWN)."""
    import numpy as np
    lib = load()
    buf = np.zeros((max_records, TRACE_WORDS), dtype=np.uint32)
    nrec = C.c_uint32(0)
    res = np.zeros(4, dtype=np.uint32)
    c = cfg.to_c(instance, 1)
    if production:
        c.flags |= CFG_TRACE_PRODUCTION
    check(lib.pxb_trace_instance(C.byref(c), instance, _ptr(buf), max_records, C.byref(nrec), _ptr(res)))
    return trace_records(buf[:nrec.value]), res


def trace_records(records):
    """Decode pxb_trace_step rows (uint32 (k, TRACE_WORDS), as trace_batch returns
    them) into the dicts trace_instance returns."""
    out = []
    for r in records:
        N, P = int(r[2]), int(r[3])
        out.append({"step": int(r[0]), "in_flight": int(r[1]),
                    "acc": r[4:4 + 36].reshape(9, 4)[:N].copy(), "digest": r[40:49][:N].copy(),
                    "prop": r[49:49 + 24].reshape(3, 8)[:P].copy()})
    return out


TRACE_OK, TRACE_BAILED = 0, 1
TRACE_BATCH_MAX = 1 << 30


def _trace_cfg(cfg: Config, production: bool) -> pxb_config:
    c = cfg.to_c(0, 1)
    if production:
        c.flags |= CFG_TRACE_PRODUCTION
    return c


def trace_batch(cfg: Config, ids, step_min: int = 0, step_max: int = U32_MAX, tail: int = 0, capacity=None,
                production: bool = False):
    """pxb_trace_batch: the instances `ids` (any order, repeats allowed) traced
    in one launch.  Of every instance's per-step records (trace_instance's), those
    with step_min <= step <= step_max are kept, cut to the last `tail` when tail
    != 0.  Returns (records uint32 (k, TRACE_WORDS), offsets uint64 (n + 1,),
    status uint32 (n,), results uint32 (n, 4)): instance i's records are
    records[offsets[i]:offsets[i + 1]] (decode them with trace_records), status
    TRACE_OK or TRACE_BAILED (beyond the state machine's link capacities, where
    trace_instance raises: no records, a zeroed result).  capacity=None sizes the
    record buffer with a count-only call first; with a capacity, k =
    min(offsets[n], capacity) and the offsets stay the full ones."""
    import numpy as np
    lib = load()
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    n = len(ids)
    offs = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    res = np.zeros((n, 4), dtype=np.uint32)
    c = _trace_cfg(cfg, production)
    sel = pxb_trace_sel(step_min, step_max, tail, 0)
    total = C.c_uint64(0)
    args = (_ptr(offs), _ptr(status) if n else None, _ptr(res) if n else None, C.byref(total))
    if capacity is None:
        check(lib.pxb_trace_batch(C.byref(c), _ptr(ids) if n else None, n, C.byref(sel), None, 0, *args))
        capacity = total.value
        if capacity == 0:
            return np.zeros((0, TRACE_WORDS), dtype=np.uint32), offs, status, res
    rec =np.zeros((capacity, TRACE_WORDS), dtype=np.uint32)
    check(lib.pxb_trace_batch(C.byref(c), _ptr(ids) if n else None, n, C.byref(sel), _ptr(rec) if capacity else None,
                              capacity, *args))
    return rec[:min(total.value, capacity)], offs, status, res


def trace_batch_device(cfg: Config, d_ids, count: int, d_offsets, d_records=None, capacity: int = 0, d_status=None,
                       d_results=None, step_min: int = 0, step_max: int = U32_MAX, tail: int = 0,
                       production: bool = False, stream=None):
    """pxb_trace_batch_device on torch tensors, asynchronous on `stream`: d_ids
    int64 (count,), d_offsets int64 (count + 1,), d_records int32 (capacity,
    TRACE_WORDS) or None with capacity 0 (the sizing call), d_status int32
    (count,) and d_results int32 (count, 4) optional.  Records at or past
    `capacity` are counted in the offsets and not written.  Sizes and dtypes
    are checked here: the C ABI takes raw pointers."""
    if d_offsets is None:
        raise ValueError("d_offsets is required")
    if count and d_ids is None:
        raise ValueError("d_ids is required")
    if capacity and d_records is None:
        raise ValueError("d_records is required when capacity > 0")
    if count > TRACE_BATCH_MAX:
        raise ValueError("count: at most 2^30 instances a call")
    _check_buf("d_ids", d_ids, count, 8)
    _check_buf("d_offsets", d_offsets, count + 1, 8)
    _check_buf("d_records", d_records, TRACE_WORDS * capacity, 4)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_results", d_results, 4 * count, 4)
    lib = load()
    c = _trace_cfg(cfg, production)
    sel = pxb_trace_sel(step_min, step_max, tail, 0)
    s = C.c_void_p(stream) if stream else None
    check(lib.pxb_trace_batch_device(C.byref(c), _ptr(d_ids), count, C.byref(sel), _ptr(d_records) if capacity else None,
                                     capacity, _ptr(d_offsets), _ptr(d_status), _ptr(d_results), s))


# ---- scripted schedules (include/paxos_batch.h, docs/SEMANTICS.md §10) --------
SCRIPT_MAX_DEPTH = 4096
SCRIPT_BAD = 2                   # status of a malformed row
SCRIPT_KEEP8, SCRIPT_KEEP16 = 0xFF, 0xFFFF
SCRIPT_HDR = 16


def script_links_off(cfg: Config) -> int:
    return SCRIPT_HDR + 4 * cfg.n_acceptors


def script_stride(cfg: Config, depth: int) -> int:
    """pxb_script_stride: bytes between the rows of a call (a multiple of 8)."""
    return (script_links_off(cfg) + 2 * cfg.n_proposers * cfg.n_acceptors * depth + 7) & ~7


def scripts_empty(cfg: Config, ids, depth: int):
    """All-keep rows, uint8 (n, stride): row i is the instance ids[i]."""
    import numpy as np
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    rows = np.zeros((len(ids), script_stride(cfg, depth)), dtype=np.uint8)
    rows[:, 10:script_links_off(cfg) + 2 * cfg.n_proposers * cfg.n_acceptors * depth] = SCRIPT_KEEP8
    script_base(rows)[:] = ids
    return rows


def _script_view(rows, off, dtype, tail):
    """A numpy view (no copy) of a field of every row: shape (n,) + tail."""
    import numpy as np
    if rows.dtype != np.uint8 or rows.ndim != 2 or not rows.flags["C_CONTIGUOUS"]:
        raise ValueError("rows: C-contiguous uint8 (n, stride) required")
    size = np.dtype(dtype).itemsize
    strides, s = [], size
    for d in reversed(tail):
        strides.insert(0, s)
        s *= d
    return np.ndarray((rows.shape[0],) + tuple(tail), dtype=dtype, buffer=rows, offset=off,
                      strides=(rows.shape[1],) + tuple(strides))


def script_base(rows):
    """uint64 (n,): the Philox base ids."""
    import numpy as np
    return _script_view(rows, 0, np.uint64, ())


def script_n_proposers(rows):
    """uint8 (n,): 0 = keep, else the proposer count."""
    import numpy as np
    return _script_view(rows, 8, np.uint8, ())


def script_skews(rows):
    """uint16 (n, 3): the Tick steps, 0xFFFF = keep."""
    import numpy as np
    return _script_view(rows, 10, np.uint16, (3,))


def script_windows(cfg: Config, rows):
    """uint16 (n, N, 2): the isolation windows [c0, c1); both 0xFFFF = keep."""
    import numpy as np
    return _script_view(rows, SCRIPT_HDR, np.uint16, (cfg.n_acceptors, 2))


def script_links(cfg: Config, rows, depth: int):
    """uint8 (n, 2, P, N, depth): [dirn][p][a][k]; 0xFF keep, 0 lost, else the delay."""
    import numpy as np
    if rows.shape[1] != script_stride(cfg, depth):
        raise ValueError("rows: stride %d, %d expected at depth %d" % (rows.shape[1], script_stride(cfg, depth), depth))
    return _script_view(rows, script_links_off(cfg), np.uint8, (2, cfg.n_proposers, cfg.n_acceptors, depth))


def _script_rows(cfg, rows, depth):
    import numpy as np
    if not 0 <= depth <= SCRIPT_MAX_DEPTH:
        raise ValueError("depth: 0..%d" % SCRIPT_MAX_DEPTH)
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim == 1:
        rows = rows[None, :]
    if rows.ndim != 2 or rows.shape[1] != script_stride(cfg, depth):
        raise ValueError("rows: uint8 (n, %d) expected at depth %d" % (script_stride(cfg, depth), depth))
    return rows


def extract_schedule(cfg: Config, ids, depth: int):
    """pxb_schedule_extract: the fully explicit rows (no keep anywhere) of the
    schedule Philox gives (cfg.seed, ids[i]); uint8 (n, stride)."""
    import numpy as np
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    rows = np.zeros((len(ids), script_stride(cfg, depth)), dtype=np.uint8)
    c = cfg.to_c(0, 1)
    n = len(ids)
    check(load().pxb_schedule_extract(C.byref(c), _ptr(ids) if n else None, n, depth, _ptr(rows) if n else None))
    return rows


def run_scripted(cfg: Config, rows, depth: int, want_digests=True, want_acceptors=False):
    """pxb_run_scripted: the rows through the per-lane state machine.  Returns
    (results uint32 (n, 4), digests (n, N), acceptor records (n, N, 4), status
    (n,), sent uint16 (n, 2, P, N)): pxb.run's outputs row by row, status
    TRACE_OK / TRACE_BAILED / SCRIPT_BAD (not OK: zeroed outputs), and the
    messages sent on every link (the entries of the row the run consumed)."""
    import numpy as np
    rows = _script_rows(cfg, rows, depth)
    n, P, N = len(rows), cfg.n_proposers, cfg.n_acceptors
    res = np.zeros((n, 4), dtype=np.uint32)
    dig = np.zeros((n, N), dtype=np.uint32) if want_digests else None
    acc = np.zeros((n, N, 4), dtype=np.uint32) if want_acceptors else None
    status = np.zeros(n, dtype=np.uint32)
    sent = np.zeros((n, 2, P, N), dtype=np.uint16)
    c = cfg.to_c(0, 1)
    if n:
        check(load().pxb_run_scripted(C.byref(c), _ptr(rows), n, depth, _ptr(res), _ptr(dig), _ptr(acc), _ptr(status),
                                      _ptr(sent)))
    return res, dig, acc, status, sent


def trace_scripted(cfg: Config, rows, depth: int, step_min: int = 0, step_max: int = U32_MAX, tail: int = 0,
                   capacity=None):
    """pxb_trace_scripted: trace_batch with script rows in place of ids (the
    default variant only); the same returns."""
    import numpy as np
    lib = load()
    rows = _script_rows(cfg, rows, depth)
    n = len(rows)
    offs = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    res = np.zeros((n, 4), dtype=np.uint32)
    c = cfg.to_c(0, 1)
    sel = pxb_trace_sel(step_min, step_max, tail, 0)
    total = C.c_uint64(0)
    head = (C.byref(c), _ptr(rows) if n else None, n, depth, C.byref(sel))
    args = (_ptr(offs), _ptr(status) if n else None, _ptr(res) if n else None, C.byref(total))
    if capacity is None:
        check(lib.pxb_trace_scripted(*head, None, 0, *args))
        capacity = total.value
        if capacity == 0:
            return np.zeros((0, TRACE_WORDS), dtype=np.uint32), offs, status, res
    rec = np.zeros((capacity, TRACE_WORDS), dtype=np.uint32)
    check(lib.pxb_trace_scripted(*head, _ptr(rec) if capacity else None, capacity, *args))
    return rec[:min(total.value, capacity)], offs, status, res


def _check_script_call(cfg, d_rows, count, depth):
    if not 0 <= depth <= SCRIPT_MAX_DEPTH:
        raise ValueError("depth: 0..%d" % SCRIPT_MAX_DEPTH)
    if count > TRACE_BATCH_MAX:
        raise ValueError("count: at most 2^30 rows a call")
    if count and d_rows is None:
        raise ValueError("d_rows is required")
    if d_rows is not None:
        _check_bytes("d_rows", d_rows, count * script_stride(cfg, depth))


def extract_schedule_device(cfg: Config, d_ids, count: int, depth: int, d_rows, stream=None):
    """pxb_schedule_extract_device on torch tensors, asynchronous on `stream`:
    d_ids int64 (count,), d_rows uint8 (count * stride)."""
    if count and d_ids is None:
        raise ValueError("d_ids is required")
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_ids", d_ids, count, 8)
    c = cfg.to_c(0, 1)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_schedule_extract_device(C.byref(c), _ptr(d_ids), count, depth, _ptr(d_rows), s))


def run_scripted_device(cfg: Config, d_rows, count: int, depth: int, d_results=None, d_digests=None,
                        d_acceptors=None, d_status=None, d_sent=None, stream=None):
    """pxb_run_scripted_device on torch tensors, asynchronous on `stream`: d_rows
    uint8, d_results int32 (count, 4), d_digests int32 (count, N), d_acceptors
    int32 (count, N, 4), d_status int32 (count,), d_sent int16 (count, 2, P, N);
    every output optional.  Sizes and dtypes are checked here."""
    N, P = cfg.n_acceptors, cfg.n_proposers
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_results", d_results, 4 * count, 4)
    _check_buf("d_digests", d_digests, N * count, 4)
    _check_buf("d_acceptors", d_acceptors, 4 * N * count, 4)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_sent", d_sent, 2 * P * N * count, 2)
    c = cfg.to_c(0, 1)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_run_scripted_device(C.byref(c), _ptr(d_rows), count, depth, _ptr(d_results), _ptr(d_digests),
                                         _ptr(d_acceptors), _ptr(d_status), _ptr(d_sent), s))


def trace_scripted_device(cfg: Config, d_rows, count: int, depth: int, d_offsets, d_records=None, capacity: int = 0,
                          d_status=None, d_results=None, step_min: int = 0, step_max: int = U32_MAX, tail: int = 0,
                          stream=None):
    """pxb_trace_scripted_device on torch tensors: trace_batch_device with d_rows
    (uint8) and depth in place of d_ids."""
    if d_offsets is None:
        raise ValueError("d_offsets is required")
    if capacity and d_records is None:
        raise ValueError("d_records is required when capacity > 0")
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_offsets", d_offsets, count + 1, 8)
    _check_buf("d_records", d_records, TRACE_WORDS * capacity, 4)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_results", d_results, 4 * count, 4)
    c = cfg.to_c(0, 1)
    sel = pxb_trace_sel(step_min, step_max, tail, 0)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_trace_scripted_device(C.byref(c), _ptr(d_rows), count, depth, C.byref(sel),
                                           _ptr(d_records) if capacity else None, capacity, _ptr(d_offsets),
                                           _ptr(d_status), _ptr(d_results), s))


# ---- handler events of scripted rows (docs/SEMANTICS.md §13) ---------------------
EVT_ACCEPTOR, EVT_PROPOSER = 0, 1
EVT_HANDLED, EVT_DISCARDED_DEAD, EVT_DISCARDED_ISOL = 0, 1, 2
EVT_PEER_TICK = 0xFF
EVENT_BYTES = 96


class pxb_trace_prop(C.Structure):
    _fields_ = [("ticket", C.c_int32), ("cmd", C.c_uint32), ("acks", C.c_uint32), ("state", C.c_uint32),
                ("mr_t", C.c_int32), ("mr_v", C.c_uint32), ("r2_v", C.c_uint32), ("pending", C.c_uint32)]


class _pxb_event_acc(C.Structure):
    _fields_ = [("rec", pxb_acceptor_rec), ("log_digest", C.c_uint32)]


class _pxb_event_after(C.Union):
    _fields_ = [("acc", _pxb_event_acc), ("prop", pxb_trace_prop)]


class pxb_trace_event(C.Structure):
    _fields_ = [("step", C.c_uint32), ("actor", C.c_uint8), ("index", C.c_uint8), ("peer", C.c_uint8),
                ("fate", C.c_uint8), ("n_out", C.c_uint32), ("reserved", C.c_uint32), ("in_", pxb_msg),
                ("out", pxb_msg * 2), ("after", _pxb_event_after)]


assert C.sizeof(pxb_trace_event) == EVENT_BYTES and C.sizeof(pxb_trace_prop) == 32
_event_dtype = None


def event_dtype():
    """The numpy structured dtype of pxb_trace_event (96 bytes): step, actor,
    index, peer, fate, n_out, reserved, in and out[2] as (kind, x, y, z), and
    after as its 8 words (event_after_acc / event_after_prop name them)."""
    global _event_dtype
    if _event_dtype is None:
        import numpy as np
        msg = np.dtype([("kind", "<u4"), ("x", "<i4"), ("y", "<i4"), ("z", "<u4")])
        _event_dtype = np.dtype([("step", "<u4"), ("actor", "u1"), ("index", "u1"), ("peer", "u1"), ("fate", "u1"),
                                 ("n_out", "<u4"), ("reserved", "<u4"), ("in", msg), ("out", msg, (2,)),
                                 ("after", "<u4", (8,))])
        assert _event_dtype.itemsize == EVENT_BYTES
    return _event_dtype


def event_after_acc(ev):
    """after.acc of an acceptor event: (t_max, t_store, val, meta, log_digest)."""
    return tuple(int(x) for x in ev["after"][:5])


def event_after_prop(ev):
    """after.prop of a proposer event, in pxb_trace_prop's order: (ticket, cmd,
    acks, state, mr_t, mr_v, r2_v, pending)."""
    return tuple(int(x) for x in ev["after"])


def trace_events(cfg: Config, rows, depth: int, step_min: int = 0, step_max: int = U32_MAX, capacity=None):
    """pxb_trace_events: one record per handler invocation of every script row,
    in the reference model's order.  Returns (events, offsets, status, results):
    a structured array of event_dtype() holding min(total, capacity) events
    (capacity None: all, after a sizing call), offsets uint64 (n + 1,) with
    row i's events at [offsets[i], offsets[i + 1]), status uint32 (n,) TRACE_OK /
    TRACE_BAILED / SCRIPT_BAD (not OK: no events, a zeroed result), results
    uint32 (n, 4)."""
    import numpy as np
    lib = load()
    rows = _script_rows(cfg, rows, depth)
    n = len(rows)
    offs = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    res = np.zeros((n, 4), dtype=np.uint32)
    c = cfg.to_c(0, 1)
    sel = pxb_trace_sel(step_min, step_max, 0, 0)
    total = C.c_uint64(0)
    head = (C.byref(c), _ptr(rows) if n else None, n, depth, C.byref(sel))
    args = (_ptr(offs), _ptr(status) if n else None, _ptr(res) if n else None, C.byref(total))
    if capacity is None:
        check(lib.pxb_trace_events(*head, None, 0, *args))
        capacity = total.value
        if capacity == 0:
            return np.zeros(0, dtype=event_dtype()), offs, status, res
    ev = np.zeros(capacity, dtype=event_dtype())
    check(lib.pxb_trace_events(*head, _ptr(ev) if capacity else None, capacity, *args))
    return ev[:min(total.value, capacity)], offs, status, res


def trace_events_ids(cfg: Config, ids, **kw):
    """trace_events of the plain instances `ids`: all-keep rows at depth 0."""
    return trace_events(cfg, scripts_empty(cfg, ids, 0), 0, **kw)


def trace_events_device(cfg: Config, d_rows, count: int, depth: int, d_offsets, d_events=None, capacity: int = 0,
                        d_status=None, d_results=None, step_min: int = 0, step_max: int = U32_MAX, stream=None):
    """pxb_trace_events_device on torch tensors, asynchronous on `stream`: d_rows
    uint8, d_offsets int64 (count + 1,), d_events uint8 (96 * capacity, 16-byte
    aligned; None with capacity 0 is the sizing call), d_status int32 (count,),
    d_results int32 (count, 4)."""
    if d_offsets is None:
        raise ValueError("d_offsets is required")
    if capacity and d_events is None:
        raise ValueError("d_events is required when capacity > 0")
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_offsets", d_offsets, count + 1, 8)
    if d_events is not None:
        _check_bytes("d_events", d_events, EVENT_BYTES * capacity)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_results", d_results, 4 * count, 4)
    c = cfg.to_c(0, 1)
    sel = pxb_trace_sel(step_min, step_max, 0, 0)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_trace_events_device(C.byref(c), _ptr(d_rows), count, depth, C.byref(sel),
                                         _ptr(d_events) if capacity else None, capacity, _ptr(d_offsets),
                                         _ptr(d_status), _ptr(d_results), s))


# ---- handler-path coverage (include/paxos_batch.h, docs/SEMANTICS.md §14) ----------
COVER_NAMES = ("ASK_GRANT_EMPTY", "ASK_GRANT_STORED", "ASK_NACK", "PROPOSE_ACCEPT", "PROPOSE_NACK", "EXEC_APPLY",
               "EXEC_IGNORED", "EXEC_PANIC", "DISCARD_DEAD", "DISCARD_ISOLATED", "Q1_FOREIGN_ACCEPT", "Q7_STALE_EXEC",
               "TICK_START", "TICK_BUSY", "HAVE_IDLE", "HAVE_BELOW", "HAVE_RESTART_R1", "HAVE_ABORT_R2", "R1OK_STALE",
               "R1OK_ACK", "R1OK_PROPOSE_OWN", "R1OK_PROPOSE_ADOPTED", "Q5_ADOPTED_OWN", "Q4_TIE", "R2S_DROPPED",
               "R2S_ACK", "R2S_DONE", "R2S_RESTART", "R2S_REPEAT")
COVER_CLASSES = len(COVER_NAMES)                     # PXB_COVER_CLASSES
COVER_ALL = (1 << COVER_CLASSES) - 1
COVER_BIT = {n: i for i, n in enumerate(COVER_NAMES)}    # name -> bit index (the index into a summary's lists)
for _n, _i in COVER_BIT.items():                     # COVER_<NAME>: the mask, as PXB_COVER_<NAME>
    globals()["COVER_" + _n] = 1 << _i
# the quirk classes by their number in docs/SEMANTICS.md §9, as BIT INDICES: summary.witness[pxb.COVER_Q1]
COVER_Q1, COVER_Q7, COVER_Q10, COVER_Q5, COVER_Q4, COVER_Q2 = 10, 11, 17, 22, 23, 28
COVER_NONE = (1 << 64) - 1                           # a summary's witness of a class no row has
COVER_RANGE_CHUNK = 1 << 20


class pxb_cover_summary(C.Structure):
    _fields_ = [("rows_ok", C.c_uint64), ("rows_bailed", C.c_uint64), ("rows_bad", C.c_uint64),
                ("n_matches", C.c_uint64), ("count", C.c_uint64 * 32), ("witness", C.c_uint64 * 32),
                ("witness_steps", C.c_uint32 * 32), ("union_mask", C.c_uint32), ("reserved", C.c_uint32)]


class pxb_cover_query(C.Structure):
    _fields_ = [("all_mask", C.c_uint32), ("any_mask", C.c_uint32), ("none_mask", C.c_uint32),
                ("reserved", C.c_uint32)]


COVER_SUMMARY_BYTES = 680
assert C.sizeof(pxb_cover_summary) == COVER_SUMMARY_BYTES and C.sizeof(pxb_cover_query) == 16


@dataclasses.dataclass
class CoverQuery:
    """A row matches when it is TRACE_OK, has every class of all_mask, one of
    any_mask (0: no such condition) and none of none_mask."""
    all_mask: int = 0
    any_mask: int = 0
    none_mask: int = 0

    def to_c(self):
        return pxb_cover_query(self.all_mask, self.any_mask, self.none_mask, 0)

    def matches(self, mask: int) -> bool:
        return (mask & self.all_mask) == self.all_mask and (not self.any_mask or bool(mask & self.any_mask)) and \
            not mask & self.none_mask


class CoverSummary:
    """pxb_cover_summary as Python values: rows_ok / rows_bailed / rows_bad /
    n_matches, and per class (lists of COVER_CLASSES entries, indexed by bit)
    `counts`, `witness` (row index or id of the OK row with the fewest steps,
    ties to the lowest i; COVER_NONE when no row has the class) and
    `witness_steps` (0xFFFFFFFF then); `union`, the classes some row has."""

    def __init__(self, c):
        self.rows_ok, self.rows_bailed, self.rows_bad = int(c.rows_ok), int(c.rows_bailed), int(c.rows_bad)
        self.n_matches = int(c.n_matches)
        self.counts = [int(c.count[b]) for b in range(COVER_CLASSES)]
        self.witness = [int(c.witness[b]) for b in range(COVER_CLASSES)]
        self.witness_steps = [int(c.witness_steps[b]) for b in range(COVER_CLASSES)]
        self.union = int(c.union_mask)
        self.tail = [(int(c.count[b]), int(c.witness[b]), int(c.witness_steps[b])) for b in range(COVER_CLASSES, 32)] + \
            [int(c.reserved)]

    def key(self):
        return (self.rows_ok, self.rows_bailed, self.rows_bad, self.n_matches, self.counts, self.witness,
                self.witness_steps, self.union, self.tail)

    def __eq__(self, other):
        return isinstance(other, CoverSummary) and self.key() == other.key()

    def __repr__(self):
        per = ", ".join("%s=%d" % (COVER_NAMES[b], n) for b, n in enumerate(self.counts) if n)
        return "CoverSummary(ok=%d bailed=%d bad=%d matches=%d: %s)" % (self.rows_ok, self.rows_bailed, self.rows_bad,
                                                                       self.n_matches, per)


def cover_summary_from(buf) -> CoverSummary:
    """A CoverSummary of the 680 bytes of a pxb_cover_summary (bytes, a numpy
    array, or a CPU torch tensor)."""
    if hasattr(buf, "numpy"):
        buf = buf.numpy()
    raw = bytes(buf if isinstance(buf, (bytes, bytearray)) else buf.tobytes())
    if len(raw) != COVER_SUMMARY_BYTES:
        raise ValueError("a pxb_cover_summary is %d bytes" % COVER_SUMMARY_BYTES)
    return CoverSummary(pxb_cover_summary.from_buffer_copy(raw))


def cover_names(mask: int):
    """The names of the classes of a coverage mask, in bit order."""
    return [n for i, n in enumerate(COVER_NAMES) if (int(mask) >> i) & 1]


def cover_of_events(events, n_acceptors: int, per_event: bool = False):
    """The coverage mask of ONE row's events (a structured array of
    event_dtype(), all of the row's events in trace_events' order): the
    specification of docs/SEMANTICS.md §14.  per_event: one mask per event."""
    granted = [None] * n_acceptors
    fresh = [False] * n_acceptors
    log_len = [0] * n_acceptors
    before, seen = {}, {}
    out = []
    for e in events:
        i, peer, n_out, kind = int(e["index"]), int(e["peer"]), int(e["n_out"]), int(e["in"]["kind"])
        m = 0
        if e["actor"] == EVT_ACCEPTOR:
            fate = int(e["fate"])
            if fate == EVT_DISCARDED_DEAD:
                m |= COVER_DISCARD_DEAD
            elif fate == EVT_DISCARDED_ISOL:
                m |= COVER_DISCARD_ISOLATED
            else:
                t_max, t_store, val, meta, _ = event_after_acc(e)
                rk = int(e["out"][0]["kind"]) if n_out else None
                if kind == 0:                           # AskForTicket
                    if rk == 0:
                        m |= COVER_ASK_GRANT_STORED if int(e["out"][0]["z"]) else COVER_ASK_GRANT_EMPTY
                        granted[i] = peer
                    else:
                        m |= COVER_ASK_NACK
                elif kind == 1:                         # Propose
                    if rk == 2:
                        m |= COVER_PROPOSE_ACCEPT
                        if granted[i] != peer:
                            m |= COVER_Q1_FOREIGN_ACCEPT
                    else:
                        m |= COVER_PROPOSE_NACK
                else:                                   # Execute
                    grew, dead = (meta & 0x7FFFFFFF) > log_len[i], bool(meta >> 31)
                    if grew:
                        m |= COVER_EXEC_APPLY
                        if not fresh[i]:
                            m |= COVER_Q7_STALE_EXEC
                    if dead:
                        m |= COVER_EXEC_PANIC
                    if not grew and not dead:
                        m |= COVER_EXEC_IGNORED
                fresh[i] = val != 0 and t_store == t_max
                log_len[i] = meta & 0x7FFFFFFF
        else:
            after = event_after_prop(e)
            b_ticket, _, _, b_state, b_mr_t, b_mr_v, _, _ = before.get(i, (0,) * 8)
            ticket, cmd, acks, state, mr_t, mr_v, r2_v, pending = after
            if peer == EVT_PEER_TICK:
                m |= COVER_TICK_START if n_out else COVER_TICK_BUSY
            elif kind == 1:                             # HaveTicket
                if b_state == 0:
                    m |= COVER_HAVE_IDLE
                elif not n_out:
                    m |= COVER_HAVE_BELOW
                else:
                    m |= COVER_HAVE_RESTART_R1 if b_state == 1 else COVER_HAVE_ABORT_R2
            elif kind == 0:                             # Round1OK
                if b_state != 1 or b_ticket != int(e["in"]["x"]):
                    m |= COVER_R1OK_STALE
                else:
                    if not n_out:
                        m |= COVER_R1OK_ACK
                    elif not pending:
                        m |= COVER_R1OK_PROPOSE_OWN
                    else:
                        m |= COVER_R1OK_PROPOSE_ADOPTED
                        if r2_v == cmd:
                            m |= COVER_Q5_ADOPTED_OWN
                    if int(e["in"]["z"]) and b_mr_v and b_mr_t == int(e["in"]["y"]):
                        m |= COVER_Q4_TIE
            else:                                       # Round2Success
                if b_state != 2:
                    m |= COVER_R2S_DROPPED
                else:
                    m |= (COVER_R2S_ACK, COVER_R2S_DONE, COVER_R2S_RESTART)[n_out]
                    s = seen.setdefault(i, set())
                    if peer in s:
                        m |= COVER_R2S_REPEAT
                    s.add(peer)
            if any(int(e["out"][j]["kind"]) == 1 for j in range(n_out)):      # a Propose goes out: a new Round 2
                seen[i] = set()
            before[i] = after
        out.append(m)
    if per_event:
        return out
    total = 0
    for m in out:
        total |= m
    return total


def cover(cfg: Config, rows, depth: int):
    """pxb_cover: the coverage mask of every script row.  Returns (masks uint32
    (n,), status uint32 (n,), results uint32 (n, 4), summary CoverSummary); a row
    that is not TRACE_OK has mask 0 and a zeroed result; summary.witness holds
    row indices."""
    import numpy as np
    rows = _script_rows(cfg, rows, depth)
    n = len(rows)
    masks = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    res = np.zeros((n, 4), dtype=np.uint32)
    c = cfg.to_c(0, 1)
    s = pxb_cover_summary()
    check(load().pxb_cover(C.byref(c), _ptr(rows) if n else None, n, depth, _ptr(masks) if n else None,
                           _ptr(status) if n else None, _ptr(res) if n else None, C.byref(s)))
    return masks, status, res, CoverSummary(s)


def cover_ids(cfg: Config, ids):
    """cover of the plain instances `ids`: all-keep rows at depth 0."""
    return cover(cfg, scripts_empty(cfg, ids, 0), 0)


def cover_device(cfg: Config, d_rows, count: int, depth: int, d_masks=None, d_status=None, d_results=None,
                 d_summary=None, stream=None):
    """pxb_cover_device on torch tensors, asynchronous on `stream`: d_rows uint8,
    d_masks int32 (count,), d_status int32 (count,), d_results int32 (count, 4),
    d_summary uint8 (680,) (8-byte aligned; read it back with
    cover_summary_from after a synchronise); every output optional."""
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_masks", d_masks, count, 4)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_results", d_results, 4 * count, 4)
    if d_summary is not None:
        _check_bytes("d_summary", d_summary, COVER_SUMMARY_BYTES)
    c = cfg.to_c(0, 1)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_cover_device(C.byref(c), _ptr(d_rows), count, depth, _ptr(d_masks), _ptr(d_status),
                                  _ptr(d_results), _ptr(d_summary), s))


CoverRange = collections.namedtuple("CoverRange", "summary match_ids match_masks")


def cover_range(cfg: Config, first: int, count: int, query: Optional[CoverQuery] = None, max_matches: int = 0,
                chunk: int = 0):
    """pxb_cover_range: the coverage of the plain instances first .. first + count
    - 1 (ids wrap modulo 2^64), `chunk` ids at a time on the device (0: 2^20).
    Returns CoverRange(summary, match_ids uint64, match_masks uint32): the
    summary's witnesses are instance ids; with a query, summary.n_matches counts
    every matching id and the lists hold the first max_matches in ascending
    order of i.  No output depends on `chunk`."""
    import numpy as np
    ids = np.zeros(max_matches if query is not None else 0, dtype=np.uint64)
    mm = np.zeros(len(ids), dtype=np.uint32)
    c = cfg.to_c(0, 1)
    s = pxb_cover_summary()
    q = query.to_c() if query is not None else None
    check(load().pxb_cover_range(C.byref(c), first & ((1 << 64) - 1), count, chunk, C.byref(q) if q is not None else None,
                                 _ptr(ids) if len(ids) else None, _ptr(mm) if len(ids) else None, len(ids),
                                 C.byref(s)))
    m = min(int(s.n_matches), len(ids))
    return CoverRange(CoverSummary(s), ids[:m], mm[:m])


_REQ_NAMES = ("AskForTicket", "Propose", "Execute")
_RSP_NAMES = ("Round1OK", "HaveTicket", "Round2Success")
_STATE_NAMES = ("Idle", "Round1", "Round2")


def _cmd(code):
    return command_str(int(code)) or "-"


def request_str(m) -> str:
    k, x, z = int(m["kind"]), int(m["x"]), int(m["z"])
    return "Propose(%d,%s)" % (x, _cmd(z)) if k == 1 else "%s(%d)" % (_REQ_NAMES[k], x)


def response_str(m) -> str:
    k, x, y, z = int(m["kind"]), int(m["x"]), int(m["y"]), int(m["z"])
    if k == 0:
        return "Round1OK(%d,%s)" % (x, "(%d,%s)" % (y, _cmd(z)) if z else "-")
    return "HaveTicket(%d)" % x if k == 1 else "Round2Success"


def event_lines(events):
    """One readable line per event, e.g.
    `s=3 acc1 <- p0 Propose(1,c1.1) -> Round2Success | t_max=1 store=(1,c1.1) log=0`."""
    out = []
    for e in events:
        s, i, peer, n_out = int(e["step"]), int(e["index"]), int(e["peer"]), int(e["n_out"])
        if e["actor"] == EVT_ACCEPTOR:
            t_max, t_store, val, meta, _ = event_after_acc(e)
            fate = int(e["fate"])
            made = (response_str(e["out"][0]) if n_out else "-") if fate == EVT_HANDLED else \
                "discarded (dead)" if fate == EVT_DISCARDED_DEAD else "discarded (isolated)"
            out.append("s=%d acc%d <- p%d %s -> %s | t_max=%d store=%s log=%d%s" % (
                s, i, peer, request_str(e["in"]), made, t_max, "(%d,%s)" % (t_store, _cmd(val)) if val else "-",
                meta & 0x7FFFFFFF, " DEAD" if meta >> 31 else ""))
        else:
            ticket, cmd, acks, state, mr_t, mr_v, r2_v, pending = event_after_prop(e)
            src = "Tick" if peer == EVT_PEER_TICK else "a%d %s" % (peer, response_str(e["in"]))
            made = ", ".join(request_str(e["out"][j]) for j in range(n_out)) or "-"
            out.append("s=%d prop%d <- %s -> %s | %s ticket=%d acks=%d cmd=%s%s" % (
                s, i, src, made, _STATE_NAMES[state], ticket, acks, _cmd(cmd), " pending" if pending else ""))
    return out


CHART_LOST, CHART_HANDLED, CHART_DISCARDED, CHART_IN_FLIGHT = 0, 1, 2, 3
_chart_dtype = None


def message_chart(cfg: Config, row, depth: int, events):
    """The per-message view of one row's events (all of them: no step window).
    Every event's out[] is expanded into sends: a proposer broadcast is N sends,
    to a = 0 .. N - 1, an acceptor reply is one.  The sends of a link are
    numbered in order (the seq), and each send's loss is read from the row's link
    byte; a keep byte (or a seq past `depth`) is a ValueError: extract the
    schedule first.  The j-th non-lost send of a link is the j-th delivery event
    on that link (discards count as deliveries).  Returns a structured array,
    one record per message in send order: dirn (0: p -> a, 1: a -> p), p, a, seq,
    kind, x, y, z, sent_step, fate (CHART_LOST / _HANDLED / _DISCARDED /
    _IN_FLIGHT: not delivered when the run ended), delivered_step (-1: none)."""
    global _chart_dtype
    import numpy as np
    if _chart_dtype is None:
        _chart_dtype = np.dtype([("dirn", "u1"), ("p", "u1"), ("a", "u1"), ("seq", "<u4"), ("kind", "<u4"),
                                 ("x", "<i4"), ("y", "<i4"), ("z", "<u4"), ("sent_step", "<u4"), ("fate", "u1"),
                                 ("delivered_step", "<i4")])
    row = _script_rows(cfg, row, depth)
    if len(row) != 1:
        raise ValueError("row: one script row")
    N = cfg.n_acceptors
    lk = script_links(cfg, row, depth)[0]
    sends = []                                        # (dirn, p, a, msg, step)
    deliveries = {}                                   # link -> [(step, handled, msg)]
    for e in events:
        i, peer, s = int(e["index"]), int(e["peer"]), int(e["step"])
        if e["actor"] == EVT_ACCEPTOR:
            deliveries.setdefault((0, peer, i), []).append((s, e["fate"] == EVT_HANDLED, e["in"]))
            if e["n_out"]:
                sends.append((1, peer, i, e["out"][0], s))
        else:
            if peer != EVT_PEER_TICK:
                deliveries.setdefault((1, i, peer), []).append((s, True, e["in"]))
            for j in range(int(e["n_out"])):
                sends.extend((0, i, a, e["out"][j], s) for a in range(N))
    chart = np.zeros(len(sends), dtype=_chart_dtype)
    seqs, arrived = {}, {}
    for r, (dirn, p, a, m, s) in zip(chart, sends):
        link = (dirn, p, a)
        k = seqs.get(link, 0)
        seqs[link] = k + 1
        b = int(lk[dirn, p, a, k]) if k < depth else SCRIPT_KEEP8
        if b == SCRIPT_KEEP8:
            raise ValueError("link (%d, %d, %d) seq %d is a keep entry: extract the schedule first" % (dirn, p, a, k))
        r["dirn"], r["p"], r["a"], r["seq"], r["sent_step"] = dirn, p, a, k, s
        r["kind"], r["x"], r["y"], r["z"] = m["kind"], m["x"], m["y"], m["z"]
        r["delivered_step"] = -1
        if b == 0:
            r["fate"] = CHART_LOST
            continue
        j = arrived.get(link, 0)
        arrived[link] = j + 1
        got = deliveries.get(link, [])
        if j < len(got):
            r["fate"] = CHART_HANDLED if got[j][1] else CHART_DISCARDED
            r["delivered_step"] = got[j][0]
        else:
            r["fate"] = CHART_IN_FLIGHT
    return chart


# ---- the shrinker -------------------------------------------------------------
def script_faults(cfg: Config, row, depth: int, sent):
    """The faults of one explicit row given its run's send counts `sent`
    (2, P, N): consumed link entries (k < sent) that are lost or delayed by more
    than one step, ("link", dirn, p, a, k); non-zero skews of the proposers it
    has, ("skew", p); non-empty windows, ("win", a)."""
    row = _script_rows(cfg, row, depth)
    P = int(script_n_proposers(row)[0]) or cfg.n_proposers
    lk = script_links(cfg, row, depth)[0]
    out = []
    for p in range(P):
        if script_skews(row)[0, p] not in (0, SCRIPT_KEEP16):
            out.append(("skew", p))
    for a in range(cfg.n_acceptors):
        c0, c1 = (min(int(x), 4096) for x in script_windows(cfg, row)[0, a])
        if c0 < c1:
            out.append(("win", a))
    for dirn in range(2):
        for p in range(P):
            for a in range(cfg.n_acceptors):
                for k in range(min(int(sent[dirn, p, a]), depth)):
                    b = int(lk[dirn, p, a, k])
                    if b == 0 or (b != SCRIPT_KEEP8 and min(b, cfg.delay_max) > 1):
                        out.append(("link", dirn, p, a, k))
    return out


def script_neutralise(cfg: Config, row, depth: int, fault):
    """Neutralises one fault in place: a link entry := 1 (delivered next step),
    a skew := 0, a window := none."""
    row = row if row.ndim == 2 else row[None, :]
    if fault[0] == "skew":
        script_skews(row)[0, fault[1]] = 0
    elif fault[0] == "win":
        script_windows(cfg, row)[0, fault[1]] = 0
    else:
        script_links(cfg, row, depth)[(0,) + tuple(fault[1:])] = 1


def _run_scripted_runner(cfg, rows, depth):
    res, _, _, status, sent = run_scripted(cfg, rows, depth, want_digests=False)
    return res, status, sent


def shrink(cfg: Config, instance, flag_mask: int, runner=None, max_launches: int = 64, depth: int = 64):
    """Reduces a failing instance to a 1-minimal set of faults.

    `instance` is an instance id (its schedule is extracted on the GPU at
    `depth`) or a fully explicit row (extract_schedule's).  The predicate is
    (result.flags & flag_mask) != 0 with status TRACE_OK.  A fault is a consumed
    link entry that is lost or delayed by more than one step, a non-zero skew or
    a non-empty window (script_faults); neutralising sets it to 1, 0 or none.
    Returns (row, faults, launches): the row is fully explicit with benign 1s
    past what its run consumes, keeps the predicate under any seed and base, and
    is 1-minimal (neutralising any one of `faults` loses the predicate) unless
    the budget ran out first (launches + 2 > max_launches before a round).
    A candidate whose run consumes more than `depth` entries on a link is
    rejected like one that loses the predicate.  Rounds of two launches: every
    single neutralisation of the current row, then every prefix of the
    individually removable ones; the longest prefix that keeps the predicate is
    taken.  `runner(cfg, rows, depth) -> (results, status, sent)` defaults to
    run_scripted."""
    runner = runner or _run_scripted_runner

    def run(rows):
        res, status, sent = runner(cfg, rows, depth)
        ok = [bool(status[i] == TRACE_OK and (int(res[i][3]) & 0xFF & flag_mask) and int(sent[i].max()) <= depth)
              for i in range(len(res))]
        return ok, sent, [None] * len(ok)
    return _shrink_rounds(cfg, instance, run, max_launches, depth)[:3]


def _shrink_rounds(cfg: Config, instance, run, max_launches: int, depth: int):
    """The rounds pxb.shrink and pxb.shrink_cover share (docs/SEMANTICS.md §10,
    §16).  `run(rows) -> (holds, sent, extra)`: per candidate row whether its run
    holds the predicate, its send counts, and anything of the run to hand back.
    Returns (row, faults, launches, extra of the accepted run)."""
    import numpy as np
    if isinstance(instance, (int, np.integer)):
        row = extract_schedule(cfg, [int(instance)], depth)
    else:
        row = _script_rows(cfg, instance, depth).copy()
    if len(row) != 1:
        raise ValueError("instance: one id or one row")

    def settle(r, sent):
        # benign 1s past what the run consumed (entries it never read)
        lk = script_links(cfg, r, depth)[0]
        k = np.arange(depth)[None, None, None, :]
        lk[k >= np.asarray(sent, dtype=np.int64)[..., None]] = 1
        nz = (lk != 0) & (lk != SCRIPT_KEEP8)
        lk[nz] = np.minimum(lk[nz], cfg.delay_max)

    ok, sent, extra = run(row)
    launches = 1
    if not ok[0]:
        raise ValueError("shrink: the instance does not satisfy the predicate within depth %d" % depth)
    sent, extra = np.array(sent[0]), extra[0]
    settle(row, sent)
    while True:
        faults = script_faults(cfg, row, depth, sent)
        if not faults or launches + 2 > max_launches:
            return row[0], faults, launches, extra
        cand = np.repeat(row, len(faults), axis=0)
        for i, f in enumerate(faults):
            script_neutralise(cfg, cand[i:i + 1], depth, f)
        ok = run(cand)[0]
        launches += 1
        removable = [f for f, o in zip(faults, ok) if o]
        if not removable:
            return row[0], faults, launches, extra      # 1-minimal: this launch is the proof
        cand = np.repeat(row, len(removable), axis=0)
        for i in range(len(removable)):
            for f in removable[:i + 1]:
                script_neutralise(cfg, cand[i:i + 1], depth, f)
        ok, sent_c, extra_c = run(cand)
        launches += 1
        best = max((i for i, o in enumerate(ok) if o), default=None)
        if best is None:                                # (prefix 1 is launch 1's candidate: deterministic runs keep it)
            raise PaxosError("shrink: a candidate that held did not hold again")
        row = cand[best:best + 1].copy()
        sent, extra = np.array(sent_c[best]), extra_c[best]
        settle(row, sent)


def _run_cover_runner(cfg, rows, depth):
    res, _, _, status, sent = run_scripted(cfg, rows, depth, want_digests=False)
    return res, status, sent, cover(cfg, rows, depth)[0]


def shrink_cover(cfg: Config, instance, query: Optional["CoverQuery"], flag_mask: int = 0, runner=None,
                 max_launches: int = 64, depth: int = 64):
    """pxb.shrink over a coverage predicate (docs/SEMANTICS.md §16; this function
    is the specification of pxb_shrink_cover_batch).

    The predicate of a run: status TRACE_OK; flag_mask == 0 or (result.flags &
    0xFF & flag_mask) != 0; the run's coverage mask (pxb.cover's) matches
    `query` (None: the all-zero query) by CoverQuery.matches; and no link
    consumed more than `depth` entries.  Everything else is pxb.shrink's.
    Returns (row, faults, launches, mask): mask is the coverage mask of the
    returned row's accepted run.  `runner(cfg, rows, depth) -> (results, status,
    sent, masks)` defaults to run_scripted for the first three and cover for the
    masks; `launches` counts rounds as pxb.shrink does, not device calls."""
    q = query if query is not None else CoverQuery()
    for name, m in (("all_mask", q.all_mask), ("any_mask", q.any_mask), ("none_mask", q.none_mask)):
        if m & ~((1 << COVER_CLASSES) - 1):
            raise ValueError("query.%s: bits 0..%d" % (name, COVER_CLASSES - 1))
    if flag_mask & ~0xFF:
        raise ValueError("flag_mask: the eight outcome flags")
    runner = runner or _run_cover_runner

    def run(rows):
        res, status, sent, masks = runner(cfg, rows, depth)
        ok = [bool(status[i] == TRACE_OK and (flag_mask == 0 or int(res[i][3]) & 0xFF & flag_mask)
                   and q.matches(int(masks[i])) and int(sent[i].max()) <= depth) for i in range(len(res))]
        return ok, sent, [int(m) for m in masks]
    return _shrink_rounds(cfg, instance, run, max_launches, depth)


# ---- the batched shrinker (include/paxos_batch.h, docs/SEMANTICS.md §11) --------
SHRINK_MINIMAL, SHRINK_BUDGET, SHRINK_NOT_INPUT, SHRINK_TOO_MANY, SHRINK_UNSTABLE = 0, 1, 2, 3, 4
FNV64_BASIS, FNV64_PRIME = 0xCBF29CE484222325, 0x100000001B3


def script_signature(cfg: Config, row, depth: int, sent) -> int:
    """The signature pxb_shrink_batch gives a row: FNV-1a-64 over the row's
    n_proposers byte, then 8 little-endian bytes per fault of script_faults(cfg,
    row, depth, sent), in its order: skew (0, 0, p, 0, skew u16, 0 u16), window
    (1, 0, 0, a, c0 u16, c1 u16; clamped to 4096), link (2, dirn, p, a, k u16,
    byte u16)."""
    import struct
    row = _script_rows(cfg, row, depth)
    data = bytes([int(script_n_proposers(row)[0])])
    for f in script_faults(cfg, row, depth, sent):
        if f[0] == "skew":
            data += struct.pack("<4B2H", 0, 0, f[1], 0, int(script_skews(row)[0, f[1]]), 0)
        elif f[0] == "win":
            c0, c1 = (min(int(x), 4096) for x in script_windows(cfg, row)[0, f[1]])
            data += struct.pack("<4B2H", 1, 0, 0, f[1], c0, c1)
        else:
            _, dirn, p, a, k = f
            data += struct.pack("<4B2H", 2, dirn, p, a, k, int(script_links(cfg, row, depth)[0, dirn, p, a, k]))
    h = FNV64_BASIS
    for b in data:
        h = ((h ^ b) * FNV64_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def shrink_batch(cfg: Config, instances, flag_mask: int, depth: int = 64, max_launches: int = 64, chunk: int = 4096):
    """pxb_shrink_batch: pxb.shrink for many instances at once, on the device.

    `instances`: instance ids (1-D; their schedules are extracted on the GPU at
    `depth`) or fully explicit rows (uint8 (n, stride)).  Runs in chunks of
    `chunk` parents, so that the device scratch stays bounded.  Returns (rows
    uint8 (n, stride), status (n,) SHRINK_*, n_faults (n,), launches (n,), sent
    uint16 (n, 2, P, N), results uint32 (n, 4), signature uint64 (n,)): per
    instance what shrink(cfg, instance, flag_mask, depth=depth,
    max_launches=max_launches) returns, with a status where it raises."""
    ids, rows, out = _shrink_batch_buffers(cfg, instances, depth, chunk)
    c = cfg.to_c(0, 1)
    lib = load()
    for a in range(0, len(rows), chunk):
        m = min(chunk, len(rows) - a)
        check(lib.pxb_shrink_batch(C.byref(c), _ptr(ids[a:]) if ids is not None else None, _ptr(rows[a:]), m, depth,
                                   flag_mask, max_launches, *(_ptr(o[a:]) for o in out)))
    return (rows, *out)


def _shrink_batch_buffers(cfg, instances, depth, chunk):
    """What shrink_batch and shrink_cover_batch share: the argument checks, and
    (ids or None, rows, (status, n_faults, launches, sent, results, signature))."""
    import numpy as np
    if chunk < 1:
        raise ValueError("chunk: at least 1")
    if not 0 <= depth <= SCRIPT_MAX_DEPTH:
        raise ValueError("depth: 0..%d" % SCRIPT_MAX_DEPTH)
    inst = np.asarray(instances)
    ids = None
    if inst.ndim == 2:
        rows = _script_rows(cfg, inst, depth).copy()
    else:
        ids = np.ascontiguousarray(inst, dtype=np.uint64).reshape(-1)
        rows = np.zeros((len(ids), script_stride(cfg, depth)), dtype=np.uint8)
    n, P, N = len(rows), cfg.n_proposers, cfg.n_acceptors
    return ids, rows, (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                       np.zeros((n, 2, P, N), dtype=np.uint16), np.zeros((n, 4), dtype=np.uint32),
                       np.zeros(n, dtype=np.uint64))


def shrink_batch_device(cfg: Config, d_rows, count: int, depth: int, flag_mask: int, max_launches: int = 64,
                        d_status=None, d_n_faults=None, d_launches=None, d_sent=None, d_results=None,
                        d_signature=None, stream=None):
    """pxb_shrink_batch_device on torch tensors: d_rows uint8 (count * stride),
    shrunk in place; d_status, d_n_faults, d_launches int32 (count,), d_sent
    int16 (count, 2, P, N), d_results int32 (count, 4), d_signature int64
    (count,), every output optional.  Ordered on `stream`, which the call
    synchronises once per launch."""
    N, P = cfg.n_acceptors, cfg.n_proposers
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_n_faults", d_n_faults, count, 4)
    _check_buf("d_launches", d_launches, count, 4)
    _check_buf("d_sent", d_sent, 2 * P * N * count, 2)
    _check_buf("d_results", d_results, 4 * count, 4)
    _check_buf("d_signature", d_signature, count, 8)
    c = cfg.to_c(0, 1)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_shrink_batch_device(C.byref(c), _ptr(d_rows), count, depth, flag_mask, max_launches,
                                         _ptr(d_status), _ptr(d_n_faults), _ptr(d_launches), _ptr(d_sent),
                                         _ptr(d_results), _ptr(d_signature), s))


# ---- shrinking over a coverage predicate (include/paxos_batch.h, docs/SEMANTICS.md §16) ----
class pxb_shrink_pred(C.Structure):
    _fields_ = [("flag_mask", C.c_uint32), ("max_launches", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("q", pxb_cover_query)]


assert C.sizeof(pxb_shrink_pred) == 32


def _shrink_pred(query, flag_mask, max_launches):
    q = query if query is not None else CoverQuery()
    return pxb_shrink_pred(flag_mask, max_launches, (C.c_uint32 * 2)(0, 0), q.to_c())


def shrink_cover_batch(cfg: Config, instances, query: Optional[CoverQuery], flag_mask: int = 0, depth: int = 64,
                       max_launches: int = 64, chunk: int = 4096):
    """pxb_shrink_cover_batch: pxb.shrink_cover for many instances at once, on
    the device.  `instances`, `chunk` and the first seven returned arrays as
    shrink_batch; returns (rows, status, n_faults, launches, sent, results,
    signature, masks uint32 (n,)): masks[i] is the coverage mask of the returned
    row's accepted run (NOT_INPUT / TOO_MANY: the given row's, as pxb.cover)."""
    import numpy as np
    ids, rows, out = _shrink_batch_buffers(cfg, instances, depth, chunk)
    out += (np.zeros(len(rows), dtype=np.uint32),)
    c = cfg.to_c(0, 1)
    pred = _shrink_pred(query, flag_mask, max_launches)
    lib = load()
    for a in range(0, len(rows), chunk):
        m = min(chunk, len(rows) - a)
        check(lib.pxb_shrink_cover_batch(C.byref(c), _ptr(ids[a:]) if ids is not None else None, _ptr(rows[a:]), m,
                                         depth, C.byref(pred), *(_ptr(o[a:]) for o in out)))
    return (rows, *out)


def shrink_cover_batch_device(cfg: Config, d_rows, count: int, depth: int, query: Optional[CoverQuery],
                              flag_mask: int = 0, max_launches: int = 64, d_status=None, d_n_faults=None,
                              d_launches=None, d_sent=None, d_results=None, d_signature=None, d_masks=None,
                              stream=None):
    """pxb_shrink_cover_batch_device on torch tensors: shrink_batch_device's
    arguments with the predicate of shrink_cover, and d_masks int32 (count,);
    every output optional.  Ordered on `stream`, which the call synchronises
    once per launch."""
    N, P = cfg.n_acceptors, cfg.n_proposers
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_status", d_status, count, 4)
    _check_buf("d_n_faults", d_n_faults, count, 4)
    _check_buf("d_launches", d_launches, count, 4)
    _check_buf("d_sent", d_sent, 2 * P * N * count, 2)
    _check_buf("d_results", d_results, 4 * count, 4)
    _check_buf("d_signature", d_signature, count, 8)
    _check_buf("d_masks", d_masks, count, 4)
    c = cfg.to_c(0, 1)
    pred = _shrink_pred(query, flag_mask, max_launches)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_shrink_cover_batch_device(C.byref(c), _ptr(d_rows), count, depth, C.byref(pred), _ptr(d_status),
                                               _ptr(d_n_faults), _ptr(d_launches), _ptr(d_sent), _ptr(d_results),
                                               _ptr(d_signature), _ptr(d_masks), s))


def shrink_clusters(signature, status):
    """The distinct minimal schedules of a shrink_batch: (signatures, counts)
    over the rows with status MINIMAL or BUDGET, the largest cluster first."""
    import numpy as np
    signature, status = np.asarray(signature, dtype=np.uint64), np.asarray(status)
    sig, cnt = np.unique(signature[(status == SHRINK_MINIMAL) | (status == SHRINK_BUDGET)], return_counts=True)
    order = np.argsort(-cnt.astype(np.int64), kind="stable")
    return sig[order], cnt[order]


# ---- exploration (include/paxos_batch.h, docs/SEMANTICS.md §12) ----------------
EXPLORE_MAX_RADIUS = 3
EXPLORE_MINIMAL = 1              # pxb_explore_space.flags: list only minimal candidates
EXPLORE_MAX_TOTAL = 1 << 30


def _explore_bases(S: int, A: int, radius: int):
    """[base_0, .., base_(radius + 1)] of S sites with A alternatives each:
    base_r = sum of C(S, q) A^q over q < r; the last is T."""
    import math
    base = [0]
    for r in range(radius + 1):
        base.append(base[-1] + math.comb(S, r) * A ** r)
    return base


def explore_total(cfg: Config, site_depth: int, radius: int) -> int:
    """pxb_explore_total: the candidates per parent, or 0 for a space that is
    invalid or larger than 2^30."""
    P, N, A = cfg.n_proposers, cfg.n_acceptors, cfg.delay_max
    if not (1 <= P <= 3 and 1 <= N <= 9 and 1 <= A <= 15 and 1 <= site_depth <= SCRIPT_MAX_DEPTH
            and 0 <= radius <= EXPLORE_MAX_RADIUS):
        return 0
    T = _explore_bases(2 * P * N * site_depth, A, radius)[-1]
    return T if T <= EXPLORE_MAX_TOTAL else 0


def explore_unrank(S: int, A: int, radius: int, c: int):
    """Candidate c of S sites with A alternatives within `radius`: (sites,
    digits), the sites ascending.  With base_r <= c < base_(r+1) and x = c -
    base_r, the sites satisfy x // A^r = sum of C(s_i, i) over i = 1..r (the
    combinatorial number system) and site s_i takes digit (x % A^r // A^(i-1)) % A."""
    import math
    base = _explore_bases(S, A, radius)
    if not 0 <= c < base[-1]:
        raise ValueError("c: 0..%d" % (base[-1] - 1))
    r = next(q for q in range(radius + 1) if c < base[q + 1])
    m, v = divmod(c - base[r], A ** r)
    sites, hi = [], S
    for i in range(r, 0, -1):
        lo, up = i - 1, hi                             # the largest s < hi with C(s, i) <= m
        while up - lo > 1:
            mid = (lo + up) // 2
            lo, up = (mid, up) if math.comb(mid, i) <= m else (lo, mid)
        sites.insert(0, lo)
        m -= math.comb(lo, i)
        hi = lo
    return sites, [(v // A ** i) % A for i in range(r)]


def explore_changes(cfg: Config, site_depth: int, radius: int, c: int):
    """The changes of candidate c: [(dirn, p, a, k, digit)] in ascending site
    order.  Site s is seq s % site_depth of link s // site_depth = (dirn P + p) N
    + a; digit j of a site whose parent byte is b reads as (min(b, delay_max) + 1
    + j) mod (delay_max + 1)."""
    P, N = cfg.n_proposers, cfg.n_acceptors
    if not explore_total(cfg, site_depth, radius):
        raise ValueError("no such space (or more than 2^30 candidates)")
    sites, digits = explore_unrank(2 * P * N * site_depth, cfg.delay_max, radius, c)
    out = []
    for s, j in zip(sites, digits):
        link, k = divmod(s, site_depth)
        out.append((link // N // P, link // N % P, link % N, k, j))
    return out


def _explore_unrank_many(S: int, A: int, radius: int, c):
    """explore_unrank over an array: (r (n,), sites (n, 3), digits (n, 3)),
    unused columns 0."""
    import numpy as np
    c = np.asarray(c, dtype=np.int64)
    base = np.array(_explore_bases(S, A, radius), dtype=np.int64)
    if len(c) and (c.min() < 0 or c.max() >= base[-1]):
        raise ValueError("c: 0..%d" % (base[-1] - 1))
    r = np.zeros(len(c), dtype=np.int64)
    for q in range(1, radius + 1):
        r[c >= base[q]] = q
    apow = np.array([A ** q for q in range(4)], dtype=np.int64)
    x = c - base[r]
    m, v = x // apow[r], x % apow[r]
    s = np.arange(S + 1, dtype=np.int64)
    comb = [None, s, s * (s - 1) // 2, s * (s - 1) * (s - 2) // 6]
    sites = np.zeros((len(c), 3), dtype=np.int64)
    digits = np.zeros((len(c), 3), dtype=np.int64)
    for q in range(1, radius + 1):                     # the candidates of radius q
        w = np.nonzero(r == q)[0]
        mq, hi = m[w], np.full(len(w), S, dtype=np.int64)
        for i in range(q, 0, -1):
            # the largest s < hi with C(s, i) <= m (C(., i) ascends; C(hi, i) > m by the recursion)
            si = np.minimum(np.searchsorted(comb[i], mq, side="right") - 1, hi - 1)
            sites[w, i - 1] = si
            mq = mq - comb[i][si]
            hi = si
            digits[w, i - 1] = v[w] // apow[i - 1] % A
    return r, sites, digits


def _explore_apply(cfg, parents, depth, site_depth, radius, ids):
    """(parent index, changed (n, 3) bool, link-table index (n, 3), new byte (n, 3),
    keep (n, 3) bool) of the global candidate ids over `parents`."""
    import numpy as np
    parents = _script_rows(cfg, parents, depth)
    if not 1 <= site_depth <= depth:
        raise ValueError("site_depth: 1..depth")
    T = explore_total(cfg, site_depth, radius)
    if not T:
        raise ValueError("no such space (or more than 2^30 candidates)")
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1).astype(np.int64)
    i, c = ids // T, ids % T
    if len(ids) and i.max() >= len(parents):
        raise ValueError("ids: beyond the last parent")
    A = cfg.delay_max
    r, sites, digits = _explore_unrank_many(2 * cfg.n_proposers * cfg.n_acceptors * site_depth, A, radius, c)
    changed = np.arange(3)[None, :] < r[:, None]
    idx = sites // site_depth * depth + sites % site_depth
    b = parents[i[:, None], script_links_off(cfg) + idx].astype(np.int64)
    new = (np.minimum(b, A) + 1 + digits) % (A + 1)
    return parents, i, changed, idx, new, changed & (b == SCRIPT_KEEP8)


def explore_skipped(cfg: Config, parents, depth: int, site_depth: int, radius: int, ids):
    """bool (n,): the candidates that change a keep site (byte 0xFF) of their
    parent.  They are skipped: not run, never "ran OK", never held."""
    return _explore_apply(cfg, parents, depth, site_depth, radius, ids)[5].any(axis=1)


def explore_rows(cfg: Config, parents, depth: int, site_depth: int, radius: int, ids):
    """The candidates `ids` (global: parent index * T + c, as explore lists them)
    of `parents` (one row or uint8 (n, stride)) materialised: uint8 (len(ids),
    stride), what pxb_explore_row writes.  A candidate that changes a keep site
    has no row: ValueError."""
    import numpy as np
    parents, i, changed, idx, new, keep = _explore_apply(cfg, parents, depth, site_depth, radius, ids)
    if keep.any():
        raise ValueError("ids: candidate %d changes a keep site" % int(np.asarray(ids).reshape(-1)[keep.any(axis=1)][0]))
    rows = parents[i]
    n, off = np.arange(len(rows)), script_links_off(cfg)
    for j in range(3):
        w = changed[:, j]
        rows[n[w], off + idx[w, j]] = new[w, j]
    return rows


def _explore_two_call(call, nm, capacity):
    """The listing protocol of the exploring host forms: call(ids pointer,
    capacity) runs the form, which leaves the match count in `nm`.  capacity
    None: a sizing call first, and no second call when nothing matches.
    Returns the listed ids."""
    import numpy as np
    if capacity is None:
        call(None, 0)
        capacity = nm.value
        if capacity == 0:
            return np.zeros(0, dtype=np.uint64)
    ids = np.zeros(capacity, dtype=np.uint64)
    call(_ptr(ids) if capacity else None, capacity)
    return ids[:min(nm.value, capacity)]


def _check_explore_device(cfg, d_rows, count, depth, d_n_matches, d_ids, capacity, d_counts, d_status, cnt_words=12):
    """The checks the exploring device forms share (cnt_words: the words of a parent's counts)."""
    if d_n_matches is None:
        raise ValueError("d_n_matches is required")
    if capacity and d_ids is None:
        raise ValueError("d_ids is required when capacity > 0")
    _check_script_call(cfg, d_rows, count, depth)
    _check_buf("d_n_matches", d_n_matches, 1, 8)
    _check_buf("d_ids", d_ids, capacity, 8)
    _check_buf("d_counts", d_counts, cnt_words * count, 4)
    _check_buf("d_status", d_status, count, 4)


def explore(cfg: Config, parents, depth: int, site_depth: int, radius: int, flag_mask: int, minimal: bool = True,
            capacity=None):
    """pxb_explore: every schedule within `radius` changed sites of each parent
    (the first site_depth entries of every link), run on the device.  Returns
    (ids uint64 (k,), n_matches, counts uint32 (n, 4, 3), status uint32 (n,)):
    the candidates that hold the predicate (`minimal`: those of which no proper
    subset of the changes holds) as parent index * T + c, ascending, the first
    `capacity` of them (None: all, at the price of a sizing run first);
    counts[i, r] = (ran OK, held, minimal) of parent i at radius r; status
    TRACE_OK or SCRIPT_BAD."""
    import numpy as np
    lib = load()
    rows = _script_rows(cfg, parents, depth)
    n = len(rows)
    counts = np.zeros((n, 4, 3), dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    c = cfg.to_c(0, 1)
    sp = pxb_explore_space(site_depth, radius, flag_mask, EXPLORE_MINIMAL if minimal else 0)
    nm = C.c_uint64(0)
    head = (C.byref(c), _ptr(rows) if n else None, n, depth, C.byref(sp))
    tail = (C.byref(nm), _ptr(counts) if n else None, _ptr(status) if n else None)
    ids = _explore_two_call(lambda p, cap: check(lib.pxb_explore(*head, p, cap, *tail)), nm, capacity)
    return ids, nm.value, counts, status


def explore_device(cfg: Config, d_rows, count: int, depth: int, site_depth: int, radius: int, flag_mask: int,
                   d_n_matches, d_ids=None, capacity: int = 0, d_counts=None, d_status=None, first_parent: int = 0,
                   minimal: bool = True, stream=None):
    """pxb_explore_device on torch tensors, asynchronous on `stream`, no
    synchronisation: d_rows uint8 (count * stride); d_n_matches int64 (1,), the
    write cursor, which has the call's full count added; d_ids int64 (capacity,)
    takes (first_parent + i) * T + c, ascending; d_counts int32 (count, 4, 3)
    and d_status int32 (count,) optional.  Sizes and dtypes are checked here."""
    _check_explore_device(cfg, d_rows, count, depth, d_n_matches, d_ids, capacity, d_counts, d_status)
    c = cfg.to_c(0, 1)
    sp = pxb_explore_space(site_depth, radius, flag_mask, EXPLORE_MINIMAL if minimal else 0)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_explore_device(C.byref(c), _ptr(d_rows), count, depth, C.byref(sp), first_parent,
                                    _ptr(d_ids) if capacity else None, capacity, _ptr(d_n_matches), _ptr(d_counts),
                                    _ptr(d_status), s))


# ---- coverage of an exploration (include/paxos_batch.h, docs/SEMANTICS.md §15) ----
class pxb_explore_reach(C.Structure):
    _fields_ = [("count", (C.c_uint32 * 32) * 4), ("first", C.c_uint32 * 32), ("parent_mask", C.c_uint32),
                ("union_mask", C.c_uint32)]


class pxb_explore_cover_space(C.Structure):
    _fields_ = [("site_depth", C.c_uint32), ("radius", C.c_uint32), ("flag_mask", C.c_uint32), ("flags", C.c_uint32),
                ("q", pxb_cover_query)]


EXPLORE_REACH_BYTES = 648
REACH_NONE = 0xFFFFFFFF                              # a record's `first` of a class no candidate has
assert C.sizeof(pxb_explore_reach) == EXPLORE_REACH_BYTES and C.sizeof(pxb_explore_cover_space) == 32


def reach_dtype():
    """A pxb_explore_reach as a numpy structured dtype (648 bytes)."""
    import numpy as np
    return np.dtype([("count", np.uint32, (4, 32)), ("first", np.uint32, (32,)), ("parent_mask", np.uint32),
                     ("union_mask", np.uint32)])


@dataclasses.dataclass
class ExploreReach:
    """pxb_explore_reach as Python values: counts[r][b], the candidates of radius
    r that ran OK and have class b (bit index b, as COVER_BIT); first[b], the
    lowest such candidate c or REACH_NONE; parent_mask, candidate 0's mask;
    union, the classes with any count.  `tail`: what lies at b >= COVER_CLASSES
    (zero counts, REACH_NONE firsts)."""
    counts: list
    first: list
    parent_mask: int
    union: int
    tail: list

    @classmethod
    def from_record(cls, rec):
        cnt, fst = rec["count"], rec["first"]
        return cls([[int(cnt[r][b]) for b in range(COVER_CLASSES)] for r in range(4)],
                   [int(fst[b]) for b in range(COVER_CLASSES)], int(rec["parent_mask"]), int(rec["union_mask"]),
                   [[int(cnt[r][b]) for r in range(4)] + [int(fst[b])] for b in range(COVER_CLASSES, 32)])

    def by_name(self):
        """{class name: (first, [count per radius])} of the reached classes."""
        return {n: (self.first[b], [self.counts[r][b] for r in range(4)]) for b, n in enumerate(COVER_NAMES)
                if (self.union >> b) & 1}


def explore_reach_of(masks, ran, S: int, A: int, radius: int):
    """The reach record of ONE parent from its T candidates' coverage masks and
    "ran OK" bits, in numpy: the specification of docs/SEMANTICS.md §15.  The
    mask of a candidate that did not run OK counts as 0.  Returns a 0-d array of
    reach_dtype()."""
    import numpy as np
    base = _explore_bases(S, A, radius)
    masks = np.where(np.asarray(ran, dtype=bool), np.asarray(masks, dtype=np.uint32), np.uint32(0))
    if masks.shape != (base[-1],):
        raise ValueError("masks: one per candidate (%d)" % base[-1])
    rec = np.zeros((), dtype=reach_dtype())
    rec["first"][:] = REACH_NONE
    for b in range(COVER_CLASSES):
        has = ((masks >> np.uint32(b)) & np.uint32(1)) != 0
        for r in range(radius + 1):
            rec["count"][r, b] = int(has[base[r]:base[r + 1]].sum())
        if has.any():
            rec["first"][b] = int(np.argmax(has))
            rec["union_mask"] |= np.uint32(1 << b)
    rec["parent_mask"] = masks[0]
    return rec


def reach_distance(reach):
    """The reach distance of every class from a record (an ExploreReach or a
    reach_dtype() record): a list of COVER_CLASSES entries, the smallest radius
    at which some candidate has the class, or None."""
    if not isinstance(reach, ExploreReach):
        reach = ExploreReach.from_record(reach)
    return [next((r for r in range(4) if reach.counts[r][b]), None) for b in range(COVER_CLASSES)]


def _explore_cover_space(site_depth, radius, query, flag_mask, minimal):
    q = query.to_c() if query is not None else pxb_cover_query(0, 0, 0, 0)
    return pxb_explore_cover_space(site_depth, radius, flag_mask, EXPLORE_MINIMAL if minimal else 0, q)


def explore_cover(cfg: Config, parents, depth: int, site_depth: int, radius: int, query: Optional[CoverQuery] = None,
                  flag_mask: int = 0, minimal: bool = True, capacity=None):
    """pxb_explore_cover: pxb.explore's space with pxb.cover's classes.  A
    candidate holds when it ran OK, has one of the outcome flags of `flag_mask`
    (0: no such condition) and its coverage mask matches `query` (None: any).
    Returns (ids, n_matches, counts, reach, status) with ids, n_matches, counts
    and status as pxb.explore and reach a list of ExploreReach, one per parent:
    reach_distance(reach[i]) says how many changed link entries away from
    parent i each handler class lies."""
    import numpy as np
    lib = load()
    rows = _script_rows(cfg, parents, depth)
    n = len(rows)
    counts = np.zeros((n, 4, 3), dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    reach = np.zeros(n, dtype=reach_dtype())
    c = cfg.to_c(0, 1)
    sp = _explore_cover_space(site_depth, radius, query, flag_mask, minimal)
    nm = C.c_uint64(0)
    head = (C.byref(c), _ptr(rows) if n else None, n, depth, C.byref(sp))
    tail = (C.byref(nm), _ptr(counts) if n else None, _ptr(reach) if n else None, _ptr(status) if n else None)
    ids = _explore_two_call(lambda p, cap: check(lib.pxb_explore_cover(*head, p, cap, *tail)), nm, capacity)
    return ids, nm.value, counts, [ExploreReach.from_record(r) for r in reach], status


def explore_cover_device(cfg: Config, d_rows, count: int, depth: int, site_depth: int, radius: int, d_n_matches,
                         query: Optional[CoverQuery] = None, flag_mask: int = 0, d_ids=None, capacity: int = 0,
                         d_counts=None, d_reach=None, d_status=None, first_parent: int = 0, minimal: bool = True,
                         stream=None):
    """pxb_explore_cover_device on torch tensors, asynchronous on `stream`, no
    synchronisation: the buffers of explore_device, and d_reach uint8 (count *
    648,) (8-byte aligned; after a synchronise, d_reach.cpu().numpy().view(
    reach_dtype()) gives the records).  Sizes and dtypes are checked here."""
    _check_explore_device(cfg, d_rows, count, depth, d_n_matches, d_ids, capacity, d_counts, d_status)
    if d_reach is not None:
        _check_bytes("d_reach", d_reach, EXPLORE_REACH_BYTES * count)
    c = cfg.to_c(0, 1)
    sp = _explore_cover_space(site_depth, radius, query, flag_mask, minimal)
    s = C.c_void_p(stream) if stream else None
    check(load().pxb_explore_cover_device(C.byref(c), _ptr(d_rows), count, depth, C.byref(sp), first_parent,
                                          _ptr(d_ids) if capacity else None, capacity, _ptr(d_n_matches),
                                          _ptr(d_counts), _ptr(d_reach), _ptr(d_status), s))


# ---- isolation windows as sites of the exploration (include/paxos_batch.h, docs/SEMANTICS.md §17) ----
EXPLORE_WIN_MAX_RADIUS = 2
EXPLORE_WIN_OPEN = 2             # pxb_explore_win_space.flags: one more length alternative, "to the end"
WIN_END = 4096                   # c1 of the open alternative


class pxb_explore_win_space(C.Structure):
    _fields_ = [("site_depth", C.c_uint32), ("radius", C.c_uint32), ("flag_mask", C.c_uint32), ("flags", C.c_uint32),
                ("q", pxb_cover_query), ("win_radius", C.c_uint32), ("win_first", C.c_uint32),
                ("win_starts", C.c_uint32), ("win_lens", C.c_uint32)]


class pxb_explore_win_reach(C.Structure):
    _fields_ = [("count", ((C.c_uint32 * 32) * 4) * 3), ("first", ((C.c_uint32 * 32) * 4) * 3),
                ("parent_mask", C.c_uint32), ("union_mask", C.c_uint32)]


EXPLORE_WIN_REACH_BYTES = 3080
assert C.sizeof(pxb_explore_win_reach) == EXPLORE_WIN_REACH_BYTES and C.sizeof(pxb_explore_win_space) == 48


@dataclasses.dataclass(frozen=True)
class WinGrid:
    """The window alternatives of an acceptor: starts first .. first + starts -
    1, lengths 1 .. lens and, with `open`, one more that lasts to the end (c1 =
    4096); `radius`: how many acceptors' windows a candidate may replace (0..2).
    Digit d is start d // L and length index d % L, L = lens + open."""
    first: int
    starts: int
    lens: int
    open: bool = False
    radius: int = 1

    @property
    def L(self) -> int:
        return self.lens + (1 if self.open else 0)

    @property
    def W(self) -> int:
        return self.starts * self.L

    def valid(self) -> bool:
        return (0 <= self.radius <= EXPLORE_WIN_MAX_RADIUS and self.starts >= 1 and self.first >= 0 and self.lens >= 0
                and self.L >= 1 and self.first + self.starts - 1 + self.lens <= WIN_END)

    def window(self, d: int):
        """(c0, c1) of digit d."""
        i, j = divmod(d, self.L)
        c0 = self.first + i
        return c0, (c0 + 1 + j if j < self.lens else WIN_END)


def _win_bases(N: int, W: int, radius: int):
    """[base_0, .., base_(radius + 1)] of the window choices: base_r = sum of
    C(N, q) W^q over q < r; the last is H."""
    import math
    base = [0]
    for r in range(radius + 1):
        base.append(base[-1] + math.comb(N, r) * W ** r)
    return base


def _win_split(cfg, site_depth, radius, grid):
    """(T, H) of a valid joint space, or (0, 0)."""
    T = explore_total(cfg, site_depth, radius)
    if not T or not grid.valid():
        return 0, 0
    H = _win_bases(cfg.n_acceptors, grid.W, grid.radius)[-1]
    return (T, H) if H * T <= EXPLORE_MAX_TOTAL else (0, 0)


def explore_win_total(cfg: Config, site_depth: int, radius: int, grid: WinGrid) -> int:
    """pxb_explore_win_total: T_w = H T candidates per parent, or 0 for a space
    that is invalid or larger than 2^30."""
    T, H = _win_split(cfg, site_depth, radius, grid)
    return T * H


def _win_unrank_many(N: int, grid: WinGrid, h):
    """The window choices h as arrays: (r (n,), acceptors (n, 2), digits (n, 2)),
    unused columns 0.  §12's order over N sites with W alternatives."""
    import numpy as np
    h = np.asarray(h, dtype=np.int64)
    W = grid.W
    base = np.array(_win_bases(N, W, grid.radius) + [0, 0], dtype=np.int64)
    H = int(base[grid.radius + 1])
    if len(h) and (h.min() < 0 or h.max() >= H):
        raise ValueError("h: 0..%d" % (H - 1))
    r = np.zeros(len(h), dtype=np.int64)
    for q in range(1, grid.radius + 1):
        r[h >= base[q]] = q
    x = h - base[r]
    acc, dig = np.zeros((len(h), 2), dtype=np.int64), np.zeros((len(h), 2), dtype=np.int64)
    one, two = r == 1, r == 2
    acc[one, 0], dig[one, 0] = x[one] // W, x[one] % W
    m, v = x[two] // (W * W), x[two] % (W * W)
    s = np.arange(10, dtype=np.int64)
    a2 = np.searchsorted(s * (s - 1) // 2, m, side="right") - 1      # the largest s with C(s, 2) <= m
    acc[two, 1], acc[two, 0] = a2, m - a2 * (a2 - 1) // 2
    dig[two, 0], dig[two, 1] = v % W, v // W
    return r, acc, dig


def explore_win_unrank(cfg: Config, site_depth: int, radius: int, grid: WinGrid, c: int):
    """Candidate c (c' = h T + c of §17) as ((acceptors, window digits), (sites,
    link digits)): the window choice h = c // T in §12's order over N acceptors
    with W alternatives, and explore_unrank of the link part c % T."""
    T, H = _win_split(cfg, site_depth, radius, grid)
    if not T:
        raise ValueError("no such space (or more than 2^30 candidates)")
    if not 0 <= c < T * H:
        raise ValueError("c: 0..%d" % (T * H - 1))
    r, acc, dig = _win_unrank_many(cfg.n_acceptors, grid, [c // T])
    q = int(r[0])
    links = explore_unrank(2 * cfg.n_proposers * cfg.n_acceptors * site_depth, cfg.delay_max, radius, c % T)
    return ([int(a) for a in acc[0, :q]], [int(d) for d in dig[0, :q]]), links


def explore_win_changes(cfg: Config, site_depth: int, radius: int, grid: WinGrid, c: int):
    """The changes of candidate c: ([(a, c0, c1)] in ascending acceptor order,
    explore_changes' [(dirn, p, a, k, digit)] of the link part)."""
    (accs, digs), _ = explore_win_unrank(cfg, site_depth, radius, grid, c)
    T = explore_total(cfg, site_depth, radius)
    return [(a, *grid.window(d)) for a, d in zip(accs, digs)], explore_changes(cfg, site_depth, radius, c % T)


def _explore_win_split_ids(cfg, parents, depth, site_depth, radius, grid, ids):
    import numpy as np
    parents = _script_rows(cfg, parents, depth)
    T, H = _win_split(cfg, site_depth, radius, grid)
    if not T:
        raise ValueError("no such space (or more than 2^30 candidates)")
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1).astype(np.int64)
    i, cw = ids // (T * H), ids % (T * H)
    if len(ids) and i.max() >= len(parents):
        raise ValueError("ids: beyond the last parent")
    return parents, T, i, cw // T, cw % T


def explore_win_skipped(cfg: Config, parents, depth: int, site_depth: int, radius: int, grid: WinGrid, ids):
    """bool (n,): the candidates whose link part changes a keep site of their
    parent (explore_skipped).  A changed window never skips."""
    parents, T, i, h, c = _explore_win_split_ids(cfg, parents, depth, site_depth, radius, grid, ids)
    return explore_skipped(cfg, parents, depth, site_depth, radius, i * T + c)


def explore_win_rows(cfg: Config, parents, depth: int, site_depth: int, radius: int, grid: WinGrid, ids):
    """The candidates `ids` (global: parent index * T_w + c', as explore_win
    lists them) materialised: uint8 (len(ids), stride), what pxb_explore_win_row
    writes: explore_rows of the link part, and the changed acceptors' windows as
    explicit (c0, c1) pairs in place of whatever the parent has there."""
    import numpy as np
    parents, T, i, h, c = _explore_win_split_ids(cfg, parents, depth, site_depth, radius, grid, ids)
    rows = explore_rows(cfg, parents, depth, site_depth, radius, i * T + c)
    r, acc, dig = _win_unrank_many(cfg.n_acceptors, grid, h)
    win = script_windows(cfg, rows)
    st, j = dig // grid.L, dig % grid.L
    c0 = grid.first + st
    c1 = np.where(j < grid.lens, c0 + 1 + j, WIN_END)
    for q in range(2):
        w = np.nonzero(r > q)[0]
        win[w, acc[w, q], 0], win[w, acc[w, q], 1] = c0[w, q], c1[w, q]
    return rows


def win_reach_dtype():
    """A pxb_explore_win_reach as a numpy structured dtype (3,080 bytes)."""
    import numpy as np
    return np.dtype([("count", np.uint32, (3, 4, 32)), ("first", np.uint32, (3, 4, 32)), ("parent_mask", np.uint32),
                     ("union_mask", np.uint32)])


@dataclasses.dataclass
class ExploreWinReach:
    """pxb_explore_win_reach as Python values: counts[r_w][r_l][b], the
    candidates of the cell that ran OK and have class b; first[r_w][r_l][b], the
    lowest such c' or REACH_NONE; parent_mask, candidate 0's mask; union, the
    classes with any count.  `tail_ok`: the words at b >= COVER_CLASSES are
    zero counts and REACH_NONE firsts."""
    counts: list
    first: list
    parent_mask: int
    union: int
    tail_ok: bool

    @classmethod
    def from_record(cls, rec):
        cnt, fst = rec["count"], rec["first"]
        n = COVER_CLASSES
        return cls([[[int(x) for x in cnt[a][b][:n]] for b in range(4)] for a in range(3)],
                   [[[int(x) for x in fst[a][b][:n]] for b in range(4)] for a in range(3)],
                   int(rec["parent_mask"]), int(rec["union_mask"]),
                   bool((cnt[:, :, n:] == 0).all() and (fst[:, :, n:] == REACH_NONE).all()))

    def by_name(self):
        """{class name: {(r_w, r_l): (first, count)}} of the reached classes, the populated cells only."""
        return {name: {(a, b): (self.first[a][b][k], self.counts[a][b][k]) for a in range(3) for b in range(4)
                       if self.counts[a][b][k]}
                for k, name in enumerate(COVER_NAMES) if (self.union >> k) & 1}


def explore_win_reach_of(masks, ran, r_w, r_l):
    """The reach record of ONE parent from its T_w candidates' coverage masks,
    "ran OK" bits and radii (arrays over c'), in numpy: the specification of
    docs/SEMANTICS.md §17.  Returns a 0-d array of win_reach_dtype()."""
    import numpy as np
    masks = np.where(np.asarray(ran, dtype=bool), np.asarray(masks, dtype=np.uint32), np.uint32(0))
    r_w, r_l = np.asarray(r_w), np.asarray(r_l)
    if not masks.shape == r_w.shape == r_l.shape or masks.ndim != 1:
        raise ValueError("masks, ran, r_w, r_l: one per candidate")
    rec = np.zeros((), dtype=win_reach_dtype())
    rec["first"][:] = REACH_NONE
    for b in range(COVER_CLASSES):
        has = ((masks >> np.uint32(b)) & np.uint32(1)) != 0
        for a in range(3):
            for l in range(4):
                w = np.nonzero(has & (r_w == a) & (r_l == l))[0]
                if len(w):
                    rec["count"][a, l, b], rec["first"][a, l, b] = len(w), int(w[0])
                    rec["union_mask"] |= np.uint32(1 << b)
    rec["parent_mask"] = masks[0]
    return rec


def reach_distance_win(reach):
    """The reach distance of every class from a record (an ExploreWinReach or a
    win_reach_dtype() record): a list of COVER_CLASSES entries, the least r_w +
    r_l of a cell with a non-zero count, or None."""
    if not isinstance(reach, ExploreWinReach):
        reach = ExploreWinReach.from_record(reach)
    return [min((a + l for a in range(3) for l in range(4) if reach.counts[a][l][b]), default=None)
            for b in range(COVER_CLASSES)]


def _explore_win_space(site_depth, radius, grid, query, flag_mask, minimal):
    q = query.to_c() if query is not None else pxb_cover_query(0, 0, 0, 0)
    flags = (EXPLORE_MINIMAL if minimal else 0) | (EXPLORE_WIN_OPEN if grid.open else 0)
    return pxb_explore_win_space(site_depth, radius, flag_mask, flags, q, grid.radius, grid.first, grid.starts, grid.lens)


_WIN_ARGS = {"pxb_explore_win_row": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p],
             "pxb_explore_win_device": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_uint64] + [C.c_void_p] * 5,
             "pxb_explore_win": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] +
                                [C.c_void_p] * 4}


def _win_fn(name):
    """An entry point of this family, found by symbol: a library without it is an error."""
    lib = load()
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise PaxosError("libpaxos_batch.so has no %s — rebuild it" % name)
    if name == "pxb_explore_win_total":
        fn.argtypes, fn.restype = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p], C.c_uint64
    else:
        fn.argtypes, fn.restype = _WIN_ARGS[name], C.c_int
    return fn


def explore_win(cfg: Config, parents, depth: int, site_depth: int, radius: int, grid: WinGrid,
                query: Optional[CoverQuery] = None, flag_mask: int = 0, minimal: bool = True, capacity=None):
    """pxb_explore_win: explore_cover over link changes AND isolation windows.  A
    candidate changes at most `radius` link entries and replaces the window of
    at most grid.radius acceptors by one of the grid's.  Returns (ids,
    n_matches, counts uint32 (n, 3, 4, 3), reach, status): ids as parent index *
    T_w + c' ascending; counts[i, r_w, r_l] = (ran OK, held, minimal); reach a
    list of ExploreWinReach; reach_distance_win(reach[i]) says how many changes
    (windows plus link entries) away from parent i each handler class lies."""
    import numpy as np
    fn = _win_fn("pxb_explore_win")
    rows = _script_rows(cfg, parents, depth)
    n = len(rows)
    counts = np.zeros((n, 3, 4, 3), dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    reach = np.zeros(n, dtype=win_reach_dtype())
    c = cfg.to_c(0, 1)
    sp = _explore_win_space(site_depth, radius, grid, query, flag_mask, minimal)
    nm = C.c_uint64(0)
    head = (C.byref(c), _ptr(rows) if n else None, n, depth, C.byref(sp))
    tail = (C.byref(nm), _ptr(counts) if n else None, _ptr(reach) if n else None, _ptr(status) if n else None)
    ids = _explore_two_call(lambda p, cap: check(fn(*head, p, cap, *tail)), nm, capacity)
    return ids, nm.value, counts, [ExploreWinReach.from_record(r) for r in reach], status


def explore_win_device(cfg: Config, d_rows, count: int, depth: int, site_depth: int, radius: int, grid: WinGrid,
                       d_n_matches, query: Optional[CoverQuery] = None, flag_mask: int = 0, d_ids=None,
                       capacity: int = 0, d_counts=None, d_reach=None, d_status=None, first_parent: int = 0,
                       minimal: bool = True, stream=None):
    """pxb_explore_win_device on torch tensors, asynchronous on `stream`, no
    synchronisation: the buffers of explore_cover_device with d_counts int32
    (count, 3, 4, 3) and d_reach uint8 (count * 3080,) (8-byte aligned; after a
    synchronise, d_reach.cpu().numpy().view(win_reach_dtype()) gives the
    records).  Sizes and dtypes are checked here."""
    _check_explore_device(cfg, d_rows, count, depth, d_n_matches, d_ids, capacity, d_counts, d_status, cnt_words=36)
    if d_reach is not None:
        _check_bytes("d_reach", d_reach, EXPLORE_WIN_REACH_BYTES * count)
    c = cfg.to_c(0, 1)
    sp = _explore_win_space(site_depth, radius, grid, query, flag_mask, minimal)
    s = C.c_void_p(stream) if stream else None
    check(_win_fn("pxb_explore_win_device")(C.byref(c), _ptr(d_rows), count, depth, C.byref(sp), first_parent,
                                            _ptr(d_ids) if capacity else None, capacity, _ptr(d_n_matches),
                                            _ptr(d_counts), _ptr(d_reach), _ptr(d_status), s))


def init(n_devices: int = 0):
    """pxb_init: allocate the per-device scratch of devices 0..n-1 up front."""
    check(load().pxb_init(n_devices))


def stream_release(dev: int, stream: int):
    """pxb_stream_release: a stream used with run_device is about to be
    destroyed; its bailed-id lists go back to the library."""
    load().pxb_stream_release(dev, C.c_void_p(stream))


def handoff_counts(dev: int = 0, reset: bool = True):
    """pxb_handoff_counts: (first per-lane kernel, second per-lane kernel)
    hand-off counts of device dev since its scratch was created or last reset."""
    out = (C.c_uint64 * 2)()
    check(load().pxb_handoff_counts(dev, C.cast(out, C.c_void_p), 1 if reset else 0))
    return int(out[0]), int(out[1])


def reload_hooks():
    """pxb_reload_hooks: re-read the library's test / A-B hooks (PXB_NO_EV,
    PXB_NO_TIGHT, PXB_EV_BAIL_CAP, ...) from the environment."""
    load().pxb_reload_hooks()


class hooks:
    """Context manager for tests and A/B runs: sets the given PXB_* hooks in
    the environment, has the library re-read them, and restores both on exit.

        with pxb.hooks(PXB_NO_EV="1"):
            pxb.run(cfg, 0, n)
    """

    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}
        self.old = {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        reload_hooks()
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reload_hooks()
        return False


def shutdown():
    """pxb_shutdown: free every per-device scratch buffer and the cached RCCL
    communicators (the next call allocates them again)."""
    check(load().pxb_shutdown())


def wire_decode(data: bytes, offsets, wire_type):
    """Inverse of wire_encode: (msgs (n, 4) uint32, status (n,) uint32)."""
    import numpy as np
    lib = load()
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offs) - 1
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    buf = np.ascontiguousarray(buf)
    msgs = np.zeros((max(n, 0), 4), dtype=np.uint32)
    st = np.zeros(max(n, 0), dtype=np.uint32)
    check(lib.pxb_wire_decode_host(_ptr(buf), len(data), _ptr(offs), n, wire_type, _ptr(msgs), _ptr(st)))
    return msgs, st
