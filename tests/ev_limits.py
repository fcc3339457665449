"""The per-lane kernel at the limits of its packed fields: the cells that
tests/test_ev_limits.py runs on the host build of the lane and
tests/test_ev_limits_gpu.py on the GPU.

The lane (csrc/paxos_ev.h) hands an instance to the next stage the moment a
narrow field would overflow.  Four of the six causes have pinned instances in
tests/test_ev_rare_paths.py and tests/test_ev_masked_store.py; these cells sit
on the other two, and on the 4,095-step runs that the shared words are sized
for (ev_layouts.h MAX_STEP_CAP):

  EVB_RSEQ  a link's reply seq at the top of its field: 255 on the slim layouts
            5 and 9, 511 on the compact layouts 2 / 3 / 6 / 7, 65,535 elsewhere
  EVB_LOG   an acceptor's log length at A_LEN_MAX: 31 outside log mode

  A511, A512  three duelling proposers over six acceptors with delay_max = 1
              never decide, and every link carries one reply every two steps:
              the 256th reply of a link is sent at step 511.  Layout 5 (18
              links).  At step_cap = 511 nothing is handed on and the reply
              seqs stand at 255; at 512 nearly every instance is handed on.
  S512        the straddle: A512's topology with 2 % loss and no windows.  A
              lost message costs its link a reply, so some instances end at
              255 replies or fewer and some send the 256th.  The issue asked
              for a straddle at delay_max 2 .. 8: no routed layout-5 config
              has one.  Searched on the host lane, 300 ids each: P, N = (2, 9),
              (3, 6), (3, 7) and, with delays above 4, (2, 5); delay_max 2 and
              5; loss 0, 0.1, 2, 10 %; with and without windows; step_cap 512:
              the largest reply seq is 241 (3, 7 at delay_max = 2), and two
              proposers with delay_max = 1 decide at once (reply seq <= 7).
  B, BHI      log mode over ten links, 100 Ticks per proposer in 2,048 steps:
              layout 9 (byte reply seqs) hands on the instances a link of which
              carries a 256th reply, layout 8 (16-bit) runs them.  BHI: the
              same from FIRST_HI, across 2^32.
  C, C0       one proposer, 200 Ticks, 4,095 steps: layout 9 then 8.  Its reply
              seqs end just under the byte: of the 4,096 instances from FIRST
              none sends a 256th reply (the largest seq is 242), so C0 runs
              the same config from id 0, where instance 90 does.
  D           two proposers, 0.1 % loss, 4,095 steps, layout 0: an instance that
              never decides for good keeps executing, and an acceptor's 32nd
              log entry does not fit the 5-bit length (EVB_LOG).
  E           config 4's schedule at P = 2, N = 7, 16 times longer (layout 0):
              most instances run all 4,095 steps, none is handed on.
  F           three proposers over nine acceptors, 10 % loss, 4,095 steps
              (layout 0): the FIFO hand-offs of the longest runs.

The 9-bit compact limit is out of the routing's reach: the compact layouts
get step_cap <= 512 only (ev_layouts.h layout_for), and a link carries at most
one reply every two steps, 256 in all (searched: layouts 3, 6 and 7, P = 2, 3,
delay_max 1 and 2: reply seq <= 256).  HOST_ONLY pins it on the host lane with
the layout forced: K1023 and K1024, layout 3 at step caps the routing gives to
layout 0.

Every cell runs ev_matrix.N_INST = 4096 instances; 4,096 hand-offs fit the
hand-off lists (route_plan.h EV_BAIL_CAP = 2^22 ids whatever the batch size),
so A512 does not take the list-overflow path.

T512, T512HI: config 4 at step_cap = 512, the largest cap the compact layouts
are routed for, on the tight routing (layout 7, then 6), from id 0 and across
2^32.  Not a limit of a field: the longest run of the two-stage compact path.

LANE_D_IDS: 128 ids of cell D for the lane-kernel families (pxb.trace_batch,
pxb.run_scripted), which have no next stage and answer PXB_TRACE_BAILED at a
limit: every id the host lane hands on among D's first 1,000, and the lowest
other ids (with 47 and 74, which end with 31 and 30 log entries).

A plain module (no test, no fixture), like tests/ev_matrix.py, whose Cell it
reuses so that test_ev_matrix.expected_handoffs works on these cells.
"""
import ev_matrix as M
import pxb

N_INST = M.N_INST
FIRST, FIRST_HI = M.FIRST, M.FIRST_HI

_A = dict(seed=1, n_proposers=3, n_acceptors=6, delay_max=1, crash_ppm=100000, crash_len_max=8, crash_start_max=6)
_B = dict(seed=1, n_proposers=2, n_acceptors=5, delay_max=3, loss_ppm=50000, step_cap=2048, n_ticks=100, tick_period=5)
_C = dict(seed=1, n_proposers=1, n_acceptors=5, delay_max=2, loss_ppm=20000, step_cap=4095, n_ticks=200, tick_period=8)
_K = dict(seed=1, n_proposers=3, n_acceptors=5, delay_max=1, loss_ppm=1000, crash_ppm=100000, crash_len_max=8,
          crash_start_max=6)


def _cell(name, first, l1, l2, **kw):
    cfg = pxb.Config(**kw)
    return M.Cell(name, cfg.n_proposers, cfg.n_acceptors, cfg, first, l1, l2)


CELLS = [
    _cell("A511", FIRST, 5, None, step_cap=511, **_A),
    _cell("A512", FIRST, 5, None, step_cap=512, **_A),
    _cell("S512", FIRST, 5, None, seed=1, n_proposers=3, n_acceptors=6, delay_max=1, loss_ppm=20000, step_cap=512),
    _cell("B", FIRST, 9, 8, **_B),
    _cell("BHI", FIRST_HI, 9, 8, **_B),
    _cell("C", FIRST, 9, 8, **_C),
    _cell("C0", 0, 9, 8, **_C),
    _cell("D", FIRST, 0, None, seed=1, n_proposers=2, n_acceptors=5, delay_max=2, loss_ppm=1000, step_cap=4095),
    _cell("E", FIRST, 0, None, seed=5, n_proposers=2, n_acceptors=7, delay_max=4, crash_ppm=200000, crash_len_max=16,
          crash_start_max=8, step_cap=4095),
    _cell("F", FIRST, 0, None, seed=1, n_proposers=3, n_acceptors=9, delay_max=6, loss_ppm=100000, step_cap=4095),
]
# the compact layout's 9-bit reply seq, which no routed config reaches: layout 3
# forced on the host lane (the routing gives these configs layout 0)
HOST_ONLY = [
    _cell("K1023", FIRST, 3, None, step_cap=1023, **_K),
    _cell("K1024", FIRST, 3, None, step_cap=1024, **_K),
]


_T = dict(pxb.CONFIGS[4].__dict__, step_cap=512)
TIGHT = [_cell("T512", 0, 7, 6, **_T), _cell("T512HI", FIRST_HI, 7, 6, **_T)]

# offsets from D's first: its hand-offs below 1,000 (tests/test_ev_limits.py holds
# the list to the host lane), filled up from 0
LANE_D_HANDED_ON = [175, 267, 323, 334, 530, 633, 720, 907]
LANE_D_IDS = sorted(LANE_D_HANDED_ON + list(range(128 - len(LANE_D_HANDED_ON))))
LANE_DEPTH = 64


def cell_id(cell):
    return cell.family


IDS = [cell_id(c) for c in CELLS]
BY_ID = {cell_id(c): c for c in CELLS + HOST_ONLY + TIGHT}
# the cause every hand-off of a cell's first stage must show (EVB_* names); the
# other cells' hand-offs are counted per cause and not constrained
CAUSE = {"A512": "RSEQ", "S512": "RSEQ", "B": "RSEQ", "BHI": "RSEQ", "C": "RSEQ", "C0": "RSEQ", "D": "LOG",
         "K1024": "RSEQ"}
# (first hand-offs, second hand-offs) of the host lane, cell by cell:
# tests/test_ev_limits.py holds them to test_ev_matrix.expected_handoffs, and
# tests/test_ev_limits_gpu.py the device to them, so that the GPU test does not
# run 4,096 instances of 4,095 steps through the host lane again
HANDOFFS = {"A511": (0, 0), "A512": (4053, 0), "S512": (180, 0), "B": (133, 0), "BHI": (127, 0), "C": (0, 0),
            "C0": (1, 0), "D": (37, 0), "E": (0, 0), "F": (200, 0), "T512": (59, 2), "T512HI": (53, 3),
            "K1023": (0, 0), "K1024": (4063, 0)}
# the cells whose first stage hands nothing on
NONE = ["A511", "C", "E", "K1023"]
# the 4,095-step cells whose high-water marks must stay inside their fields
LONG = ["D", "E", "F"]
