"""pxb_explore_cover measurements ("Coverage of an exploration"):
writes profiles/explore_cover_bench.json.

The space is tools/explore_bench.py's: the benign row of P = 2, N = 5,
delay_max = 4 at depth 32, site_depth 4, radius 3: S = 80 sites, T = 5,309,121
candidates.  The query: a repeated Round2Success (R2S_REPEAT), minimal listing.

  (a) end to end      one pxb.explore_cover call (capacity given, so no sizing
                      run) against the path it replaces: pxb.explore_rows on the
                      host plus pxb.cover, timed on a slice of SLICE candidates
                      and scaled to T.  Host clock around blocking calls, WARM
                      untimed and REPS timed repeats, median [min, max].
  (b) device calls    pxb.explore_cover_device and pxb.explore_device (predicate
                      0xFE) over the same parent in the same session, RUNS runs
                      in which the two calls alternate, each timed by device
                      events around the call: median and range of the runs.
  (c) per kernel      --kernels: the same alternating device calls, to be run
                      under rocprofv3 --kernel-trace --stats in a run of its own;
                      --merge DIR then reads that run's kernel trace: the two
                      candidate kernels' times, their ratio per run and its
                      range, and the other kernels of the call.

python tools/explore_cover_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/explore_cover_bench.py --kernels
python tools/explore_cover_bench.py --merge DIR [--out PATH]"""
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
from explore_bench import CAPACITY, DEPTH, RADIUS, SITE_DEPTH, space, stats, timed  # noqa: E402

SLICE, RUNS = 1 << 18, 3
FLOOR_MASK = 0xFE


def query(pxb):
    return pxb.CoverQuery(all_mask=pxb.COVER_R2S_REPEAT)


def old_way(pxb, np, cfg, row, ids, q):
    """The matching candidates among `ids` without pxb.explore_cover: rows on the host, pxb.cover, numpy."""
    masks, status, _, _ = pxb.cover(cfg, pxb.explore_rows(cfg, row, DEPTH, SITE_DEPTH, RADIUS, ids), DEPTH)
    return ids[(status == pxb.TRACE_OK) & ((masks & q.all_mask) == q.all_mask)], masks


class DeviceCalls:
    """The two device calls over the one parent, with their buffers."""

    def __init__(self, pxb, torch, cfg, row):
        dev = torch.device("cuda:0")
        self.pxb, self.cfg = pxb, cfg
        self.d_row = torch.from_numpy(row.copy()).to(dev)
        self.d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_ids = torch.zeros(CAPACITY, dtype=torch.int64, device=dev)
        self.d_counts = torch.zeros((1, 4, 3), dtype=torch.int32, device=dev)
        self.d_reach = torch.zeros(pxb.EXPLORE_REACH_BYTES, dtype=torch.uint8, device=dev)

    def cover(self):
        self.d_n.zero_()
        self.pxb.explore_cover_device(self.cfg, self.d_row, 1, DEPTH, SITE_DEPTH, RADIUS, self.d_n, query=query(self.pxb),
                                      d_ids=self.d_ids, capacity=CAPACITY, d_counts=self.d_counts, d_reach=self.d_reach)

    def floor(self):
        self.d_n.zero_()
        self.pxb.explore_device(self.cfg, self.d_row, 1, DEPTH, SITE_DEPTH, RADIUS, FLOOR_MASK, self.d_n, d_ids=self.d_ids,
                                capacity=CAPACITY, d_counts=self.d_counts)


def kernels_only():
    """(c): RUNS alternating pairs of device calls behind one warm pair."""
    import torch
    import pxb
    assert torch.cuda.is_available(), "explore_cover_bench needs a GPU"
    cfg, row, T = space(pxb)
    d = DeviceCalls(pxb, torch, cfg, row)
    for _ in range(1 + RUNS):
        d.cover()
        d.floor()
        torch.cuda.synchronize()
    print(json.dumps({"candidates": T, "runs": RUNS}))


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
    cov, flo = timed_runs("paxos_explore_cover_kernel"), timed_runs("paxos_explore_kernel")
    ratios = [ms(a) / ms(b) for a, b in zip(cov, flo)]
    with open(path) as fh:
        out = json.load(fh)
    out["per_kernel"] = {
        "method": "rocprofv3 --kernel-trace --stats, a run of its own; %d alternating pairs of device calls behind a warm "
                  "pair" % RUNS,
        "explore_cover_kernel_ms": [ms(r) for r in cov], "explore_cover_kernel_vgprs": int(cov[0]["VGPR_Count"]),
        "explore_cover_kernel_scratch": int(cov[0]["Scratch_Size"]),
        "explore_kernel_ms": [ms(r) for r in flo], "explore_kernel_vgprs": int(flo[0]["VGPR_Count"]),
        "cover_over_explore": {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)},
        "reach_init_kernel_ms": ms(timed_runs("reach_init_kernel")[-1]),
        "reach_finish_kernel_ms": ms(timed_runs("reach_finish_kernel")[-1])}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["per_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_cover_bench.json"))
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
    assert torch.cuda.is_available(), "explore_cover_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "warm": 1, "clock": "host (time.perf_counter)"}
    cfg, row, T = space(pxb)
    q = query(pxb)
    new = timed(lambda: pxb.explore_cover(cfg, row, DEPTH, SITE_DEPTH, RADIUS, q, capacity=CAPACITY), a.reps)
    print(json.dumps({"explore_cover": new}), flush=True)
    # the slice: the last SLICE candidates (radius 3, where nearly all of the space lies)
    ids = np.arange(T - SLICE, T, dtype=np.uint64)
    old = timed(lambda: old_way(pxb, np, cfg, row, ids, q), a.reps)
    held, n_held, counts, reach, _ = pxb.explore_cover(cfg, row, DEPTH, SITE_DEPTH, RADIUS, q, minimal=False, capacity=CAPACITY)
    assert n_held <= CAPACITY
    want, masks = old_way(pxb, np, cfg, row, ids, q)
    # (a slice candidate that ran past the depth has no mask in the new call; the old way applies no such rule)
    assert set(held[held >= T - SLICE].tolist()) <= set(want.tolist()), "the two ways disagree"
    ids_min, n_min, _, _, _ = pxb.explore_cover(cfg, row, DEPTH, SITE_DEPTH, RADIUS, q, capacity=CAPACITY)
    scaled = {k: v * T / SLICE if k.endswith("_ms") else v for k, v in old.items()}
    r = reach[0]
    out["end_to_end"] = {
        "space": "benign row, P 2, N 5, delay_max 4, depth %d, site_depth %d, radius %d, all_mask R2S_REPEAT" % (
            DEPTH, SITE_DEPTH, RADIUS),
        "candidates": T,
        "explore_cover": {"what": "pxb.explore_cover(minimal=True, capacity=2^20), copies included", **new},
        "old_way_slice": {"what": "pxb.explore_rows on the host + pxb.cover + the query in numpy over the last %d "
                                  "candidates (no ran-OK rule, no minimality, no reach record)" % SLICE, **old},
        "old_way_scaled": {"what": "the slice's times x T / %d" % SLICE, **scaled},
        "old_scaled_median_over_explore_cover_median": scaled["median_ms"] / new["median_ms"],
        "candidates_per_us_end_to_end": T / (1e3 * new["median_ms"]),
        "counts_ran_held_minimal_by_radius": [[int(x) for x in c] for c in counts[0]],
        "held": int(n_held), "minimal_listed": int(n_min), "first_minimal": [int(x) for x in ids_min[:4]],
        "reach_distance": dict(zip(pxb.COVER_NAMES, pxb.reach_distance(r))),
        "reach_first": {n: f for n, (f, _) in r.by_name().items()},
        "reach_counts": {n: c for n, (_, c) in r.by_name().items()}}
    print(json.dumps(out["end_to_end"]), flush=True)
    # (b) the two device calls, alternating, by device events
    d = DeviceCalls(pxb, torch, cfg, row)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_cov, t_flo = [], []
    for k in range(1 + RUNS):
        pair = []
        for call in (d.cover, d.floor):
            e0, e1 = ev(), ev()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            pair.append(e0.elapsed_time(e1))
        if k:
            t_cov.append(pair[0])
            t_flo.append(pair[1])
    ratios = [x / y for x, y in zip(t_cov, t_flo)]
    out["device_calls"] = {
        "method": "device events around each call on the default stream; %d runs behind a warm one, the two calls "
                  "alternating" % RUNS,
        "explore_cover_device": stats(t_cov), "explore_device_0xFE": stats(t_flo),
        "cover_over_explore": {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)}}
    print(json.dumps(out["device_calls"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
