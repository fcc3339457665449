"""Batched-shrinker measurements ("Batched shrinker"): writes
profiles/shrink_batch_bench.json.

  (a) batch vs loop   the first 4,096 PANIC ids of a config-3 sweep shrunk at
                      depth 64 with one pxb.shrink_batch call (extract
                      included, chunk = 4096), end to end, against the only
                      way before it: a host loop of pxb.shrink, timed on the
                      first 64 of the same ids and scaled by 64 (that code is
                      unchanged).  Host clock around blocking calls, WARM
                      untimed and REPS timed repeats, median [min, max].  Also
                      the status counts, the launches, and the number of
                      distinct signatures (pxb.shrink_clusters).
  (b) per launch      --kernels: one device call over the same ids, to be run
                      under rocprofv3 --kernel-trace --stats in a run of its
                      own; --merge DIR then reads that run's kernel trace: per
                      dispatch of the candidate kernel its grid (64 lanes per
                      block: the launch's candidates, rounded up to 64) and
                      time, and the select kernel's time.

python tools/shrink_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shrink_bench.py --kernels
python tools/shrink_bench.py --merge DIR [--out PATH]"""
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
N_IDS, N_LOOP, SWEEP_N, DEPTH = 4096, 64, 1 << 14, 64


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


def panic_ids(pxb):
    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY)
    ids, _, n_matches, _, _, _ = pxb.sweep(pxb.CONFIGS[3], 0, SWEEP_N, q, N_IDS)
    assert len(ids) == N_IDS, "the sweep found %d panics, %d needed" % (n_matches, N_IDS)
    return ids


def kernels_only():
    """(b): the device call whose kernels the profiler times (one warm call first)."""
    import torch
    import pxb
    assert torch.cuda.is_available(), "shrink_bench needs a GPU"
    dev = torch.device("cuda:0")
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    d_ids = torch.tensor(ids.astype("int64"), device=dev)
    d_rows = torch.zeros(N_IDS * pxb.script_stride(cfg, DEPTH), dtype=torch.uint8, device=dev)
    d_la = torch.zeros(N_IDS, dtype=torch.int32, device=dev)
    for _ in range(2):
        pxb.extract_schedule_device(cfg, d_ids, N_IDS, DEPTH, d_rows)
        pxb.shrink_batch_device(cfg, d_rows, N_IDS, DEPTH, pxb.F_PANIC, d_launches=d_la)
        torch.cuda.synchronize()
    print(json.dumps({"max_launches_taken": int(d_la.max().item())}))


def merge(path, prof_dir):
    rows = []
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "shrink" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cand = [r for r in rows if "paxos_shrink_kernel" in r["Kernel_Name"]]
    sel = [r for r in rows if "shrink_select_kernel" in r["Kernel_Name"]]
    assert len(cand) >= 2 and len(cand) % 2 == 0, "kernel trace: %d dispatches of paxos_shrink_kernel" % len(cand)
    cand, sel = cand[len(cand) // 2:], sel[len(sel) // 2:]                  # (the second, warm call)
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    with open(path) as fh:
        out = json.load(fh)
    out["per_launch"] = {
        "method": "rocprofv3 --kernel-trace --stats, a run of its own; the second of two device calls",
        "launches": len(cand),
        "candidates_rounded_to_64": [int(r["Grid_Size_X"]) for r in cand],
        "candidate_kernel_vgprs": int(cand[0]["VGPR_Count"]), "candidate_kernel_scratch": int(cand[0]["Scratch_Size"]),
        "candidate_kernel_us": [us(r) for r in cand],
        "select_kernel_us": [us(r) for r in sel],
        "candidate_kernel_total_ms": sum(us(r) for r in cand) / 1e3,
        "select_kernel_total_ms": sum(us(r) for r in sel) / 1e3}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["per_launch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink_batch_bench.json"))
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
    assert torch.cuda.is_available(), "shrink_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)"}
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    sub = [int(i) for i in ids[:N_LOOP]]
    scale = N_IDS // N_LOOP

    def loop():
        for i in sub:
            try:
                pxb.shrink(cfg, i, pxb.F_PANIC, depth=DEPTH)
            except ValueError:                       # (not an input within the depth: its one launch is counted)
                pass
    lp = timed(loop, a.reps)
    bt = timed(lambda: pxb.shrink_batch(cfg, ids, pxb.F_PANIC, depth=DEPTH, chunk=N_IDS), a.reps)
    _, status, n_faults, launches, _, _, sig = pxb.shrink_batch(cfg, ids, pxb.F_PANIC, depth=DEPTH, chunk=N_IDS)
    csig, ccnt = pxb.shrink_clusters(sig, status)
    shrunk = (status == pxb.SHRINK_MINIMAL) | (status == pxb.SHRINK_BUDGET)
    out["batch_vs_loop"] = {
        "config": 3, "ids": N_IDS, "depth": DEPTH, "flag_mask": "F_PANIC", "max_launches": 64,
        "ids_from": "pxb.sweep(F_PANIC) over instances 0..%d" % (SWEEP_N - 1),
        "loop": {"what": "pxb.shrink(depth=64), %d ids, scaled by %d" % (N_LOOP, scale),
                 **{k: (v * scale if k.endswith("_ms") else v) for k, v in lp.items()}},
        "batch": {"what": "pxb.shrink_batch(ids, chunk=4096), extract and copies included", **bt},
        "loop_median_over_batch_median": lp["median_ms"] * scale / bt["median_ms"],
        "status_counts": {str(k): int((status == k).sum()) for k in range(5)},
        "launches": {"min": int(launches[shrunk].min()), "median": float(np.median(launches[shrunk])),
                     "max": int(launches.max())},
        "faults_left": {"min": int(n_faults[shrunk].min()), "median": float(np.median(n_faults[shrunk])),
                        "max": int(n_faults[shrunk].max())},
        "distinct_signatures": int(len(csig)), "largest_clusters": [int(x) for x in ccnt[:8]]}
    print(json.dumps(out["batch_vs_loop"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
