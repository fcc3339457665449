"""The lane-kernel families accept exactly the same shapes (csrc/lane_shapes.h):
pxb_trace_instance, pxb_trace_batch_device, pxb_run_scripted_device,
pxb_trace_scripted_device, pxb_shrink_batch_device, pxb_explore_device,
pxb_trace_events_device, pxb_cover_device, pxb_explore_cover_device,
pxb_explore_win_device and pxb_shrink_cover_batch_device are called with an
otherwise valid, empty job over a sweep of proposer counts, acceptor counts, delays and Tick counts.  A shape with a kernel passes
validation (PXB_E_NODEV without a GPU, PXB_OK with one), a shape without one is
PXB_E_INVAL, and every family agrees with the table written out here."""
import ctypes as C

import numpy as np

import pxb

PROPOSERS = range(0, 5)
ACCEPTORS = range(1, 11)
DELAYS = (1, 8, 9, 15, 16)
TICKS = (1, 2)


def has_kernel(P, N, delay_max, n_ticks):
    """The table: P in 1..3, N in 2..9, delays up to 15 on the 8-step (<= 8) or
    the 16-step wheel, log mode (n_ticks > 1) on the 8-step wheel only."""
    if P not in (1, 2, 3) or N not in (2, 3, 4, 5, 6, 7, 8, 9):
        return False
    return delay_max in ((1, 8) if n_ticks > 1 else (1, 8, 9, 15))


def test_every_family_accepts_the_same_shapes():
    import torch
    L = pxb.load()
    gpu = torch.cuda.is_available()
    passes = pxb.PXB_OK if gpu else pxb.PXB_E_NODEV
    if gpu:                                            # (the traces' and the events' empty jobs write offsets[0])
        d_off = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        off_p = C.c_void_p(d_off.data_ptr())
    else:
        off_p = C.c_void_p(np.zeros(1, np.uint64).ctypes.data)
    nm = np.zeros(1, np.uint64)
    rec = np.zeros((64, pxb.TRACE_WORDS), np.uint32)
    n_rec = C.c_uint32(0)
    sp = pxb.pxb_explore_space(1, 1, 0xFE, 0)
    csp = pxb.pxb_explore_cover_space(1, 1, 0xFE, 0, pxb.pxb_cover_query(0, 0, 0, 0))
    wsp = pxb.pxb_explore_win_space(1, 1, 0xFE, 0, pxb.pxb_cover_query(0, 0, 0, 0), 1, 0, 1, 1)
    win_device = pxb._win_fn("pxb_explore_win_device")
    pred = pxb.pxb_shrink_pred(0xFE, 8, (C.c_uint32 * 2)(0, 0), pxb.pxb_cover_query(0, 0, 0, 0))
    families = {
        "pxb_trace_instance": lambda c: L.pxb_trace_instance(c, 0, C.c_void_p(rec.ctypes.data), len(rec),
                                                             C.byref(n_rec), None),
        "pxb_trace_batch_device": lambda c: L.pxb_trace_batch_device(c, None, 0, None, None, 0, off_p, None, None, None),
        "pxb_run_scripted_device": lambda c: L.pxb_run_scripted_device(c, None, 0, 1, None, None, None, None, None, None),
        "pxb_trace_scripted_device": lambda c: L.pxb_trace_scripted_device(c, None, 0, 1, None, None, 0, off_p, None,
                                                                           None, None),
        "pxb_shrink_batch_device": lambda c: L.pxb_shrink_batch_device(c, None, 0, 1, 0xFE, 8, None, None, None, None,
                                                                       None, None, None),
        "pxb_explore_device": lambda c: L.pxb_explore_device(c, None, 0, 1, C.byref(sp), 0, None, 0,
                                                             C.c_void_p(nm.ctypes.data), None, None, None),
        "pxb_trace_events_device": lambda c: L.pxb_trace_events_device(c, None, 0, 1, None, None, 0, off_p, None, None,
                                                                       None),
        "pxb_cover_device": lambda c: L.pxb_cover_device(c, None, 0, 1, None, None, None, None, None),
        "pxb_explore_cover_device": lambda c: L.pxb_explore_cover_device(c, None, 0, 1, C.byref(csp), 0, None, 0,
                                                                         C.c_void_p(nm.ctypes.data), None, None, None,
                                                                         None),
        "pxb_explore_win_device": lambda c: win_device(c, None, 0, 1, C.byref(wsp), 0, None, 0,
                                                       C.c_void_p(nm.ctypes.data), None, None, None, None),
        "pxb_shrink_cover_batch_device": lambda c: L.pxb_shrink_cover_batch_device(c, None, 0, 1, C.byref(pred), None,
                                                                                   None, None, None, None, None, None,
                                                                                   None),
    }
    wrong = []
    for P in PROPOSERS:
        for N in ACCEPTORS:
            for delay_max in DELAYS:
                for n_ticks in TICKS:
                    cfg = pxb.Config(seed=0x5A, n_proposers=P, n_acceptors=N, delay_max=delay_max, step_cap=16,
                                     n_ticks=n_ticks, tick_period=4)
                    c = cfg.to_c(0, 1)
                    want = passes if has_kernel(P, N, delay_max, n_ticks) else pxb.PXB_E_INVAL
                    for name, call in families.items():
                        rc = call(C.byref(c))
                        if rc != want:
                            wrong.append((name, P, N, delay_max, n_ticks, rc, want))
    assert not wrong, wrong[:20]
