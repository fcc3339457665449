"""Explorer measurements ("Exploration"): writes
profiles/explore_bench.json.

The space: the benign row (every link byte 1, no skews, no windows) of P = 2,
N = 5, delay_max = 4 at depth 32, site_depth 4, radius 3: S = 80 sites, T =
5,309,121 candidates, predicate F_LOG_DIVERGENCE.

  (a) end to end      one pxb.explore call (minimal listing, capacity given, so
                      no sizing run) against what a user could do before it:
                      pxb.explore_rows on the host in chunks of 2^18 candidates,
                      pxb.run_scripted over the materialised rows and the
                      predicate in numpy (no minimality: the old way does less).
                      Host clock around blocking calls, WARM untimed and REPS
                      timed repeats, median [min, max].
  (b) per kernel      --kernels: the rows materialised once into device memory,
                      then pxb.explore_device and pxb.run_scripted_device over
                      them, to be run under rocprofv3 --kernel-trace --stats in a
                      run of its own; --merge DIR then reads that run's kernel
                      trace: the candidate kernel alone against the script
                      kernel over the same candidates (what the accessor and the
                      unranking cost), and the minimal and list kernels.

python tools/explore_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/explore_bench.py --kernels
python tools/explore_bench.py --merge DIR [--out PATH]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "cloud-haskell-paxos_amd"))
WARM = 1
DEPTH, SITE_DEPTH, RADIUS, CHUNK, CAPACITY = 32, 4, 3, 1 << 18, 1 << 20


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(f, reps):
    ms = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        if k >= WARM:
            ms.append(1e3 * (t1 - t0))
    return stats(ms)


def space(pxb):
    cfg = pxb.Config(seed=0xE5, n_proposers=2, n_acceptors=5, delay_max=4, step_cap=256)
    row = pxb.scripts_empty(cfg, [0], DEPTH)
    pxb.script_n_proposers(row)[0] = cfg.n_proposers
    pxb.script_skews(row)[:] = 0
    pxb.script_windows(cfg, row)[:] = 0
    pxb.script_links(cfg, row, DEPTH)[:] = 1
    return cfg, row[0], pxb.explore_total(cfg, SITE_DEPTH, RADIUS)


def old_way(pxb, np, cfg, row, T, mask):
    """The held candidates without pxb.explore: rows on the host, run_scripted, numpy."""
    held = []
    for a in range(0, T, CHUNK):
        ids = np.arange(a, min(a + CHUNK, T), dtype=np.uint64)
        res, _, _, status, sent = pxb.run_scripted(cfg, pxb.explore_rows(cfg, row, DEPTH, SITE_DEPTH, RADIUS, ids), DEPTH,
                                                   want_digests=False)
        ok = (status == pxb.TRACE_OK) & (sent.reshape(len(ids), -1).max(axis=1) <= DEPTH) & ((res[:, 3] & 0xFF & mask) != 0)
        held.append(ids[ok])
    return np.concatenate(held)


def kernels_only():
    """(b): the device calls whose kernels the profiler times (one warm call of each first)."""
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "explore_bench needs a GPU"
    dev = torch.device("cuda:0")
    cfg, row, T = space(pxb)
    stride = pxb.script_stride(cfg, DEPTH)
    d_all = torch.zeros(T * stride, dtype=torch.uint8, device=dev)
    for a in range(0, T, CHUNK):
        ids = np.arange(a, min(a + CHUNK, T), dtype=np.uint64)
        rows = pxb.explore_rows(cfg, row, DEPTH, SITE_DEPTH, RADIUS, ids)
        d_all[a * stride:(a + len(ids)) * stride] = torch.from_numpy(rows.reshape(-1)).to(dev)
    d_row = torch.from_numpy(row.copy()).to(dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(CAPACITY, dtype=torch.int64, device=dev)
    d_counts = torch.zeros((1, 4, 3), dtype=torch.int32, device=dev)
    d_res = torch.zeros((T, 4), dtype=torch.int32, device=dev)
    d_status = torch.zeros(T, dtype=torch.int32, device=dev)
    d_sent = torch.zeros(T * 2 * cfg.n_proposers * cfg.n_acceptors, dtype=torch.int16, device=dev)
    for _ in range(2):
        d_n.zero_()
        pxb.explore_device(cfg, d_row, 1, DEPTH, SITE_DEPTH, RADIUS, pxb.F_LOG_DIVERGENCE, d_n, d_ids=d_ids,
                           capacity=CAPACITY, d_counts=d_counts)
        pxb.run_scripted_device(cfg, d_all, T, DEPTH, d_results=d_res, d_status=d_status, d_sent=d_sent)
        torch.cuda.synchronize()
    print(json.dumps({"candidates": T, "listed": int(d_n.item())}))


def merge(path, prof_dir):
    rows = []
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731

    def last(name):                                  # (the second, warm call)
        hit = [r for r in rows if name in r["Kernel_Name"]]
        assert len(hit) >= 2, "kernel trace: %d dispatches of %s" % (len(hit), name)
        return hit[-1]
    cand, scr = last("paxos_explore_kernel"), last("paxos_script_kernel")
    with open(path) as fh:
        out = json.load(fh)
    n = out["end_to_end"]["candidates"]
    out["per_kernel"] = {
        "method": "rocprofv3 --kernel-trace --stats, a run of its own; the second of two device calls of each",
        "candidate_kernel_ms": us(cand) / 1e3, "candidate_kernel_vgprs": int(cand["VGPR_Count"]),
        "candidate_kernel_scratch": int(cand["Scratch_Size"]),
        "script_kernel_same_rows_ms": us(scr) / 1e3, "script_kernel_vgprs": int(scr["VGPR_Count"]),
        "candidate_over_script": us(cand) / us(scr),
        "candidates_per_us": n / us(cand),
        "minimal_kernel_ms": us(last("explore_minimal_kernel")) / 1e3,
        "scatter_kernel_ms": us(last("explore_scatter_kernel")) / 1e3}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["per_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_bench.json"))
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
    assert torch.cuda.is_available(), "explore_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)"}
    cfg, row, T = space(pxb)
    mask = pxb.F_LOG_DIVERGENCE
    new = timed(lambda: pxb.explore(cfg, row, DEPTH, SITE_DEPTH, RADIUS, mask, minimal=True, capacity=CAPACITY), a.reps)
    print(json.dumps({"explore": new}), flush=True)
    old = timed(lambda: old_way(pxb, np, cfg, row, T, mask), a.reps)
    ids, n, counts, _ = pxb.explore(cfg, row, DEPTH, SITE_DEPTH, RADIUS, mask, minimal=True, capacity=CAPACITY)
    held = pxb.explore(cfg, row, DEPTH, SITE_DEPTH, RADIUS, mask, minimal=False, capacity=CAPACITY)[0]
    assert np.array_equal(held, old_way(pxb, np, cfg, row, T, mask)[:CAPACITY]), "the two ways disagree"
    out["end_to_end"] = {
        "space": "benign row, P 2, N 5, delay_max 4, depth %d, site_depth %d, radius %d, F_LOG_DIVERGENCE" % (
            DEPTH, SITE_DEPTH, RADIUS),
        "candidates": T,
        "explore": {"what": "pxb.explore(minimal=True, capacity=2^20), copies included", **new},
        "old_way": {"what": "pxb.explore_rows on the host + pxb.run_scripted in chunks of 2^18 + the predicate in numpy "
                            "(no minimality)", **old},
        "old_median_over_explore_median": old["median_ms"] / new["median_ms"],
        "candidates_per_us_end_to_end": T / (1e3 * new["median_ms"]),
        "counts_ran_held_minimal_by_radius": [[int(x) for x in r] for r in counts[0]],
        "minimal_listed": int(n), "first_minimal": [int(x) for x in ids[:4]]}
    print(json.dumps(out["end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
