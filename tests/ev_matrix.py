"""The per-lane kernel's test matrix: every layout the routing takes
(csrc/ev_layouts.h, csrc/route_plan.h) at every topology it takes it for.

A cell is (family, P, N, config, first-stage layout, second-stage layout or
None).  A family is one fixed set of schedule knobs, chosen from the rules of
ev::layout_for and route_plan so that the whole family lands on one layout;
tests/test_ev_matrix.py checks that against the routing itself, so the table
cannot drift from it.  The seed of a cell is 0x5EED0200 + 16 P + N.

  L3   compact, 4-step wheel: lossy, skewed, delays <= 4, P N <= 16
  L6   the same for simple schedules (no loss, no skew); P = 2 with N = 6, 7
       is routed tight: layout 7 over the batch, layout 6 over its hand-offs
  L5   slim, 8-step wheel, at its last delay (8), step cap <= 512
  L0   8-step wheel, step cap above 512
  L1   16-step wheel
  LG4  log mode, delays above 4; P N <= 10 in two stages (layout 4, then 8)
  LG9  log mode, delays <= 4, P N <= 10 (layout 9, then 8)

Every cell runs N_INST instances from FIRST; one cell per family runs a second
time from FIRST_HI, across 2^32.  A cell must keep at least 7/8 of its
instances on the layout under test (HANDOFF_CAP).

This is a plain module (no test, no fixture): tests/test_ev_matrix.py runs the
cells on the host build of the lane, tests/test_ev_matrix_gpu.py on the GPU.
Below the cells: the 72 shapes of the lane-kernel families, which
tests/test_script_gpu.py and tests/test_trace_batch_gpu.py sweep.
"""
import collections
import functools
import os

import oracle_c
import pxb

N_INST = 4096
FIRST = 1000
FIRST_HI = (1 << 32) - 1000            # just below 2^32: the batch crosses it
HANDOFF_CAP = N_INST // 8

TOPOLOGIES = [(P, N) for P in (1, 2, 3) for N in range(2, 10)]

Cell = collections.namedtuple("Cell", "family P N cfg first layout1 layout2")


def _cfg(P, N, **kw):
    return pxb.Config(seed=0x5EED0200 + 16 * P + N, n_proposers=P, n_acceptors=N, **kw)


_LOSSY = dict(loss_ppm=100000, skew_max=2, crash_ppm=150000, crash_len_max=8, crash_start_max=6)
_LOG = dict(loss_ppm=50000, skew_max=2, crash_ppm=100000, crash_len_max=12, crash_start_max=30, step_cap=1024,
            n_ticks=6, tick_period=9)
# LG4 at P = 3, N = 9: on the family's schedule the layout-4 lane hands 567 of
# 4096 instances on (host build), above HANDOFF_CAP.  Its hand-offs are pool
# overflows, three proposers' responses over 27 links in flight at once: fewer
# Ticks change nothing (2 Ticks: 563) and less loss makes it worse (2 %: 870,
# none: 1172), so this one cell is eased with more loss, the other families'
# 10 %: 151 (the counts of every cell: tests/test_ev_matrix.py)
_LG4_EASED = {(3, 9): dict(loss_ppm=100000)}


def _tight(P, N):
    return P == 2 and N in (6, 7)


# family -> (topologies, schedule of (P, N), (first-stage layout, second-stage layout or None) of (P, N))
FAMILIES = {
    "L3": (lambda P, N: P * N <= 16,
           lambda P, N: dict(_LOSSY, delay_max=4, step_cap=256),
           lambda P, N: (3, None)),
    "L6": (lambda P, N: P * N <= 16,
           lambda P, N: dict(delay_max=4, crash_ppm=200000, crash_len_max=16, crash_start_max=8, step_cap=256),
           lambda P, N: (7, 6) if _tight(P, N) else (6, None)),
    "L5": (lambda P, N: True,
           lambda P, N: dict(_LOSSY, delay_max=8, step_cap=400),
           lambda P, N: (5, None)),
    "L0": (lambda P, N: True,
           lambda P, N: dict(_LOSSY, delay_max=6, step_cap=1024),
           lambda P, N: (0, None)),
    "L1": (lambda P, N: True,
           lambda P, N: dict(_LOSSY, delay_max=12, step_cap=600),
           lambda P, N: (1, None)),
    "LG4": (lambda P, N: True,
            lambda P, N: {**_LOG, "delay_max": 6, **_LG4_EASED.get((P, N), {})},
            lambda P, N: (4, 8) if P * N <= 10 else (4, None)),
    "LG9": (lambda P, N: P * N <= 10,
            lambda P, N: dict(_LOG, delay_max=3),
            lambda P, N: (9, 8)),
}

# the cell of each family that also runs from FIRST_HI: a two-stage one where the
# family has one, else one whose lane hands some instances on
HIGH_FIRST = {"L3": (3, 5), "L6": (2, 7), "L5": (2, 9), "L0": (3, 8), "L1": (3, 6), "LG4": (3, 3), "LG9": (2, 5)}


def _cells():
    out = []
    for fam, (has, sched, layouts) in FAMILIES.items():
        for P, N in TOPOLOGIES:
            if not has(P, N):
                continue
            l1, l2 = layouts(P, N)
            for first in (FIRST, FIRST_HI) if HIGH_FIRST[fam] == (P, N) else (FIRST,):
                out.append(Cell(fam, P, N, _cfg(P, N, **sched(P, N)), first, l1, l2))
    return out


CELLS = _cells()


def cell_id(cell):
    return "%s-p%dn%d%s" % (cell.family, cell.P, cell.N, "" if cell.first == FIRST else "-hi")


IDS = [cell_id(c) for c in CELLS]


# ---- the lane-kernel families' shapes (csrc/lane_shapes.h): 3 proposer counts x
# 8 acceptor counts x {8-step wheel, 16-step wheel, log mode}, on the lossy
# schedule of test_script_gpu.py's test_g8_every_kernel_unit_launches.  A shape
# runs LANE_IDS; at most LANE_CAP of them may end with a status other than OK
# (tests/test_ev_matrix.py checks that on the host build of the lane).
LANE_MODES = {"w8": dict(delay_max=4), "w16": dict(delay_max=12),
              "log": dict(delay_max=4, n_ticks=6, tick_period=9)}
LANE_SHAPES = [(P, N, mode) for P, N in TOPOLOGIES for mode in LANE_MODES]
LANE_SHAPE_IDS = ["p%dn%d-%s" % s for s in LANE_SHAPES]
LANE_IDS = list(range(FIRST, FIRST + 128))
LANE_DEPTH = 64
LANE_CAP = len(LANE_IDS) // 8


def lane_cfg(P, N, mode):
    return pxb.Config(seed=0x5EED0100 + 16 * P + N, n_proposers=P, n_acceptors=N, loss_ppm=100000, skew_max=3,
                      crash_ppm=100000, crash_len_max=8, crash_start_max=8, step_cap=256, **LANE_MODES[mode])


@functools.lru_cache(maxsize=None)
def lane_oracle(P, N, mode):
    """The oracle's (results, digests, acceptor records) of a shape's LANE_IDS:
    computed once, read-only."""
    out = oracle_c.run_cpu(lane_cfg(P, N, mode), LANE_IDS[0], len(LANE_IDS), threads=min(16, os.cpu_count() or 1),
                           want_acceptors=True)[:3]
    for a in out:
        a.setflags(write=False)
    return out
