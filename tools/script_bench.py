"""Scripted-schedule measurements ("Scripted schedules"): writes
profiles/script_bench.json.  Recorded, not gated: no threshold.

  run_scripted   2^16 config-3 rows (ids 0 .. 2^16 - 1) through
                 pxb_run_scripted_device (results, status and send counts) at
                 depth 0, at depth 64 with all-keep rows, and at depth 64 with the
                 fully explicit rows pxb_schedule_extract writes.  Comparison
                 point: the closest path before it, pxb_trace_batch_device's
                 sizing call (capacity = 0: the count pass and the scan) on the
                 same ids, in the same session.
  extract        pxb_schedule_extract_device of the same ids at depth 64.
  shrink         one pxb.shrink end to end (host forms, launches included) of the
                 first panicking config-3 instance a sweep of 4,096 lists.

Host clock around the call and a device synchronise, WARM untimed and REPS timed
repeats, median [min, max].

python tools/script_bench.py [--reps R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "cloud-haskell-paxos_amd"))
WARM = 3
N, DEPTH = 1 << 16, 64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "script_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "script_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = pxb.CONFIGS[3]
    P, NA = cfg.n_proposers, cfg.n_acceptors
    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)", "config": 3,
           "rows": N, "depth": DEPTH}
    ids = np.arange(N, dtype=np.uint64)
    d_ids = torch.arange(N, dtype=torch.int64, device=dev)
    d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(N, dtype=torch.int32, device=dev)
    d_res = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    d_sent = torch.zeros((N, 2, P, NA), dtype=torch.int16, device=dev)

    def sizing():
        pxb.trace_batch_device(cfg, d_ids, N, d_off, d_status=d_st, d_results=d_res)
        torch.cuda.synchronize()
    out["trace_batch_sizing_call"] = timed(sizing, a.reps)
    base_res = d_res.clone()

    d_explicit = torch.zeros(N * pxb.script_stride(cfg, DEPTH), dtype=torch.uint8, device=dev)

    def extract():
        pxb.extract_schedule_device(cfg, d_ids, N, DEPTH, d_explicit)
        torch.cuda.synchronize()
    out["extract_depth64"] = {**timed(extract, a.reps), "bytes": int(d_explicit.numel())}

    cases = (("depth0", 0, torch.tensor(pxb.scripts_empty(cfg, ids, 0).reshape(-1), device=dev)),
             ("depth64_all_keep", DEPTH, torch.tensor(pxb.scripts_empty(cfg, ids, DEPTH).reshape(-1), device=dev)),
             ("depth64_explicit", DEPTH, d_explicit))
    for name, depth, d_rows in cases:
        def run():
            pxb.run_scripted_device(cfg, d_rows, N, depth, d_results=d_res, d_status=d_st, d_sent=d_sent)
            torch.cuda.synchronize()
        t = timed(run, a.reps)
        covered = (d_st == 0) & (d_sent.reshape(N, -1).to(torch.int32).max(dim=1).values <= depth)
        same = bool((d_res[d_st == 0] == base_res[d_st == 0]).all().item()) if name != "depth64_explicit" else None
        out["run_scripted_" + name] = {**t, "bailed": int((d_st != 0).sum().item()), "row_bytes": int(d_rows.numel()),
                                       "over_sizing_call": t["median_ms"] / out["trace_batch_sizing_call"]["median_ms"],
                                       "results_equal_trace_batch": same, "rows_within_depth": int(covered.sum().item())}
        print(json.dumps({name: out["run_scripted_" + name]}), flush=True)

    q = pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY)
    pid = int(pxb.sweep(cfg, 0, 4096, q, 1)[0][0])
    t0 = time.perf_counter()
    row, faults, launches = pxb.shrink(cfg, pid, pxb.F_PANIC, depth=DEPTH)
    out["shrink"] = {"instance": pid, "ms": 1e3 * (time.perf_counter() - t0), "launches": launches,
                     "faults_left": len(faults)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
