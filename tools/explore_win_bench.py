"""pxb_explore_win measurements ("Isolation windows as sites"):
writes profiles/explore_win_bench.json.

The space: tools/explore_bench.py's benign row of P = 2, N = 5, delay_max = 4
at depth 32, site_depth 4, at link radius 2 (S = 80 sites, T = 50,881) with
the window grid (0, 8, 3, open), one window: W = 32, H = 161, T_w = 8,191,841
candidates.  The query: EXEC_PANIC.

The yardstick of the candidate kernel is pxb_explore_cover_device over the H
window variants materialised as H parents: the same candidates on the same
lanes, in the same order.

  (a) end to end      one pxb.explore_win call (capacity given, so no sizing
                      run) against the composed host path: the H rows built by
                      pxb.explore_win_rows and staged, pxb.explore_cover over
                      them (held listing), then the joint minimality in numpy.
                      Host clock around blocking calls, WARM untimed and REPS
                      timed repeats, median [min, max].
  (b) device calls    pxb.explore_win_device and pxb.explore_cover_device over
                      the H parents in the same session, RUNS runs in which the
                      two calls alternate, each timed by device events.
  (c) per kernel      --kernels: the same alternating device calls, to be run
                      under rocprofv3 --kernel-trace --stats in a run of its own;
                      --merge DIR then reads that run's kernel trace: both
                      candidate kernels' medians and min-max spreads, their
                      ratio, the allowance (the yardstick's median plus three of
                      its own spreads) and whether the new kernel is within it,
                      VGPRs and scratch, and the other kernels of the call.

python tools/explore_win_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/explore_win_bench.py --kernels
python tools/explore_win_bench.py --merge DIR [--out PATH]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "cloud-haskell-paxos_amd"))
sys.path.insert(0, HERE)
from explore_bench import DEPTH, SITE_DEPTH, space, stats, timed  # noqa: E402

RADIUS, RUNS, CAPACITY = 2, 3, 1 << 22
GRID = dict(first=0, starts=8, lens=3, open=True, radius=1)


def setup(pxb):
    cfg, row, _ = space(pxb)
    grid = pxb.WinGrid(**GRID)
    T = pxb.explore_total(cfg, SITE_DEPTH, RADIUS)
    Tw = pxb.explore_win_total(cfg, SITE_DEPTH, RADIUS, grid)
    return cfg, row, grid, T, Tw // T, Tw


def query(pxb):
    return pxb.CoverQuery(all_mask=1 << pxb.COVER_BIT["EXEC_PANIC"])


def variants(pxb, np, cfg, row, grid, T, H):
    """The H window variants of the parent as H rows."""
    return pxb.explore_win_rows(cfg, row, DEPTH, SITE_DEPTH, RADIUS, grid, np.arange(H, dtype=np.uint64) * np.uint64(T))


def composed(pxb, np, cfg, row, grid, T, H, q, tables):
    """The joint minimal list without pxb.explore_win: one parent per window
    variant through pxb.explore_cover, then the two-axis subset rule in numpy."""
    rows = variants(pxb, np, cfg, row, grid, T, H)
    ids, n, _, _, _ = pxb.explore_cover(cfg, rows, DEPTH, SITE_DEPTH, RADIUS, q, minimal=False, capacity=CAPACITY)
    assert n <= CAPACITY
    held = np.zeros(H * T, bool)
    held[ids.astype(np.int64)] = True
    held = held.reshape(H, T)
    (lrank, lvalid), (rw_of, wrank, wvalid) = tables
    smaller = np.zeros((H, T), bool)
    for sw in range(4):
        sub_w = held[wrank[sw]]
        for sl in range(7):
            smaller |= wvalid[sw][:, None] & lvalid[sl][None, :] & sub_w[:, lrank[sl]]
        smaller |= (wvalid[sw] & (sw < (1 << rw_of) - 1))[:, None] & sub_w
    return np.nonzero((held & ~smaller).reshape(-1))[0].astype(np.uint64), n


class DeviceCalls:
    """The two device calls with their buffers: the joint space over the one
    parent, and the link space over the H materialised parents."""

    def __init__(self, pxb, torch, np, cfg, row, grid, T, H):
        dev = torch.device("cuda:0")
        self.pxb, self.cfg, self.grid, self.H = pxb, cfg, grid, H
        self.d_row = torch.from_numpy(row.copy()).to(dev)
        self.d_rows = torch.from_numpy(variants(pxb, np, cfg, row, grid, T, H).reshape(-1).copy()).to(dev)
        self.d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_ids = torch.zeros(CAPACITY, dtype=torch.int64, device=dev)
        self.d_wcounts = torch.zeros(36, dtype=torch.int32, device=dev)
        self.d_wreach = torch.zeros(pxb.EXPLORE_WIN_REACH_BYTES, dtype=torch.uint8, device=dev)
        self.d_counts = torch.zeros(H * 12, dtype=torch.int32, device=dev)
        self.d_reach = torch.zeros(H * pxb.EXPLORE_REACH_BYTES, dtype=torch.uint8, device=dev)

    def win(self):
        self.d_n.zero_()
        self.pxb.explore_win_device(self.cfg, self.d_row, 1, DEPTH, SITE_DEPTH, RADIUS, self.grid, self.d_n,
                                    query=query(self.pxb), d_ids=self.d_ids, capacity=CAPACITY, d_counts=self.d_wcounts,
                                    d_reach=self.d_wreach)

    def cover(self):
        self.d_n.zero_()
        self.pxb.explore_cover_device(self.cfg, self.d_rows, self.H, DEPTH, SITE_DEPTH, RADIUS, self.d_n,
                                      query=query(self.pxb), d_ids=self.d_ids, capacity=CAPACITY, d_counts=self.d_counts,
                                      d_reach=self.d_reach)


def kernels_only():
    """(c): RUNS alternating pairs of device calls behind one warm pair."""
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "explore_win_bench needs a GPU"
    cfg, row, grid, T, H, Tw = setup(pxb)
    d = DeviceCalls(pxb, torch, np, cfg, row, grid, T, H)
    for _ in range(1 + RUNS):
        d.win()
        d.cover()
        torch.cuda.synchronize()
    print(json.dumps({"candidates": Tw, "runs": RUNS}))


def merge(path, prof_dir):
    rows = []
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731

    def timed_runs(name):                            # (the first dispatch is the warm one)
        hit = [r for r in rows if name in r["Kernel_Name"]]
        assert len(hit) == 1 + RUNS, "kernel trace: %d dispatches of %s" % (len(hit), name)
        return hit[1:]
    win, cov = timed_runs("paxos_explore_win_kernel"), timed_runs("paxos_explore_cover_kernel")
    w_ms, c_ms = [ms(r) for r in win], [ms(r) for r in cov]
    spread = max(c_ms) - min(c_ms)
    allowance = statistics.median(c_ms) + 3.0 * spread
    with open(path) as fh:
        out = json.load(fh)
    out["per_kernel"] = {
        "method": "rocprofv3 --kernel-trace --stats, a run of its own; %d alternating pairs of device calls behind a warm "
                  "pair" % RUNS,
        "explore_win_kernel_ms": w_ms, "explore_win_kernel_median_ms": statistics.median(w_ms),
        "explore_win_kernel_spread_ms": max(w_ms) - min(w_ms),
        "explore_win_kernel_vgprs": int(win[0]["VGPR_Count"]), "explore_win_kernel_scratch": int(win[0]["Scratch_Size"]),
        "yardstick": "paxos_explore_cover_kernel over the H window variants materialised as H parents",
        "explore_cover_kernel_ms": c_ms, "explore_cover_kernel_median_ms": statistics.median(c_ms),
        "explore_cover_kernel_spread_ms": spread,
        "explore_cover_kernel_vgprs": int(cov[0]["VGPR_Count"]), "explore_cover_kernel_scratch": int(cov[0]["Scratch_Size"]),
        "win_over_cover_median": statistics.median(w_ms) / statistics.median(c_ms),
        "allowance_ms": allowance, "within_allowance": statistics.median(w_ms) <= allowance,
        # (the minimal and record kernels are one template each: the joint space's instances)
        "explore_win_minimal_kernel_ms": ms(timed_runs("explore_minimal_kernel<pxb::ev::ExploreWinX")[-1]),
        "explore_minimal_kernel_ms": ms(timed_runs("explore_minimal_kernel<pxb::ev::ExploreLinkX")[-1]),
        "win_reach_init_kernel_ms": ms(timed_runs("reach_init_kernel<384")[-1]),
        "win_reach_finish_kernel_ms": ms(timed_runs("reach_finish_kernel<384")[-1])}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["per_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_win_bench.json"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.out, a.merge)
    if a.kernels:
        return kernels_only()
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "explore_win_bench needs a GPU"
    torch.cuda.set_device(0)
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]   # the subset tables written out with numpy
    import explore_oracle as X
    import explore_win_oracle as XW
    out = {"device": torch.cuda.get_device_name(0), "warm": 1, "clock": "host (time.perf_counter)"}
    cfg, row, grid, T, H, Tw = setup(pxb)
    q = query(pxb)
    new = timed(lambda: pxb.explore_win(cfg, row, DEPTH, SITE_DEPTH, RADIUS, grid, q, capacity=CAPACITY), a.reps)
    print(json.dumps({"explore_win": new}), flush=True)
    S = 2 * cfg.n_proposers * cfg.n_acceptors * SITE_DEPTH
    tables = (X.subset_table(S, cfg.delay_max, RADIUS)[1:], XW.win_subset_table(cfg.n_acceptors, grid))
    old = timed(lambda: composed(pxb, np, cfg, row, grid, T, H, q, tables), a.reps)
    ids_min, n_min, counts, reach, _ = pxb.explore_win(cfg, row, DEPTH, SITE_DEPTH, RADIUS, grid, q, capacity=CAPACITY)
    want, n_held = composed(pxb, np, cfg, row, grid, T, H, q, tables)
    assert n_min <= CAPACITY and np.array_equal(ids_min, want), "the two ways disagree"
    # what the per-variant minimal lists of the composed search add up to
    per_variant = pxb.explore_cover(cfg, variants(pxb, np, cfg, row, grid, T, H), DEPTH, SITE_DEPTH, RADIUS, q, capacity=0)[1]
    r = reach[0]
    out["end_to_end"] = {
        "space": "benign row, P 2, N 5, delay_max 4, depth %d, site_depth %d, radius %d, grid %r, all_mask EXEC_PANIC" % (
            DEPTH, SITE_DEPTH, RADIUS, GRID),
        "T": T, "H": H, "candidates": Tw,
        "explore_win": {"what": "pxb.explore_win(minimal=True, capacity=2^22), copies included", **new},
        "composed": {"what": "pxb.explore_win_rows of the H variants, pxb.explore_cover over them (held listing, capacity "
                             "2^22), the joint subset rule in numpy; no joint reach record", **old},
        "composed_median_over_explore_win_median": old["median_ms"] / new["median_ms"],
        "candidates_per_us_end_to_end": Tw / (1e3 * new["median_ms"]),
        "counts_ran_held_minimal_by_cell": [[[int(x) for x in c] for c in rw] for rw in counts[0]],
        "held": int(n_held), "minimal_listed": int(n_min), "minimal_summed_per_variant": int(per_variant),
        "first_minimal": [int(x) for x in ids_min[:4]],
        "reach_distance": dict(zip(pxb.COVER_NAMES, pxb.reach_distance_win(r)))}
    print(json.dumps(out["end_to_end"]), flush=True)
    # (b) the two device calls, alternating, by device events
    d = DeviceCalls(pxb, torch, np, cfg, row, grid, T, H)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_win, t_cov = [], []
    for k in range(1 + RUNS):
        pair = []
        for call in (d.win, d.cover):
            e0, e1 = ev(), ev()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            pair.append(e0.elapsed_time(e1))
        if k:
            t_win.append(pair[0])
            t_cov.append(pair[1])
    ratios = [x / y for x, y in zip(t_win, t_cov)]
    out["device_calls"] = {
        "method": "device events around each call on the default stream; %d runs behind a warm one, the two calls "
                  "alternating" % RUNS,
        "explore_win_device": stats(t_win), "explore_cover_device_H_parents": stats(t_cov),
        "win_over_cover": {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)}}
    print(json.dumps(out["device_calls"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
