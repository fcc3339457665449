"""Query and sweep measurements ("Result queries"): writes
profiles/query_bench.json.

  query pass   pxb_query_device over N results (default 2^26 = 1 GiB) of
               BASELINE config 4 (a real run on this device) and of uniform
               random records: a sparse and a dense match, and a histogram of
               everything, each without histograms and with both at 8,194 bins.
               One HIP event pair around every call, WARM untimed calls, REPS
               timed ones; median, min and max.  Yardstick: a device-to-device
               copy of the same buffer (reads N x 16 B and writes N x 16 B, the
               bytes of the query's two reading passes), timed the same way.
  sweep        pxb_sweep of config 4 at M instances (default 2^24) against
               pxb_run_device of the same batch with the results left on the
               device (code this change does not touch), alternating, host clock
               around the blocking call / a device synchronise; five repeats.
  host bytes   what a sweep moves to the host beside pxb_run's 16 x n.

python tools/query_bench.py [--n N] [--m M] [--reps R] [--out PATH]"""
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


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    import torch
    import pxb
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--m", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "query_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, cap = a.n, 1 << 20
    cfg = pxb.CONFIGS[4]

    def timed(f):
        ms = []
        for k in range(WARM + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if k >= WARM:
                ms.append(e0.elapsed_time(e1))
        return stats(ms)

    d_tot = torch.zeros(pxb.NCOUNTERS, dtype=torch.int64, device=dev)
    data = {"config4": torch.zeros((n, 4), dtype=torch.int32, device=dev)}
    pxb.run_device(cfg, 0, n, d_results=data["config4"], d_totals=d_tot)
    torch.cuda.synchronize()
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    data["uniform"] = torch.randint(-(1 << 31), 1 << 31, (n, 4), dtype=torch.int32, device=dev, generator=g)
    d_copy = torch.empty_like(data["uniform"])
    d_ids = torch.zeros(n, dtype=torch.int64, device=dev)
    d_m = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
    d_hs = torch.zeros(pxb.HIST_MAX_BINS, dtype=torch.int64, device=dev)
    d_hr = torch.zeros(pxb.HIST_MAX_BINS, dtype=torch.int64, device=dev)

    # (name, query without histograms, capacity)
    variants = {
        "config4": [("sparse: PANIC | LOG_DIVERGENCE", pxb.Query(pxb.F_PANIC | pxb.F_LOG_DIVERGENCE, pxb.Q_ANY), cap),
                    ("dense: STEP_CAP, list of 2^20", pxb.Query(pxb.F_STEP_CAP, pxb.Q_ANY), cap),
                    ("dense: STEP_CAP, list of n", pxb.Query(pxb.F_STEP_CAP, pxb.Q_ANY), n),
                    ("everything, no list", pxb.Query(), 0)],
        "uniform": [("sparse: all eight flags, steps <= 8192", pxb.Query(0xFF, pxb.Q_ALL, steps_max=8192), cap),
                    ("dense: flags & 5, list of 2^20", pxb.Query(0x05, pxb.Q_ANY), cap),
                    ("dense: flags & 5, list of n", pxb.Query(0x05, pxb.Q_ANY), n),
                    ("everything, no list", pxb.Query(), 0)],
    }
    out = {"n_results": n, "bytes": 16 * n, "warm": WARM, "device": torch.cuda.get_device_name(0), "query": []}
    for name, d_res in data.items():
        copy = timed(lambda: d_copy.copy_(d_res))
        bar = copy["median_ms"] + (copy["max_ms"] - copy["min_ms"])
        out["query"].append({"data": name, "what": "device-to-device copy (yardstick)", **copy, "bar_ms": bar})
        for what, q0, capacity in variants[name]:
            for bins in (0, pxb.HIST_MAX_BINS):
                q = pxb.Query(**{**q0.__dict__, "n_bins_steps": bins, "n_bins_rounds": bins})

                def call():
                    d_cur.zero_()
                    pxb.query_device(d_res, 0, n, q, d_cur, d_ids if capacity else None, d_m if capacity else None,
                                     capacity, d_hs if bins else None, d_hr if bins else None)
                t = timed(call)
                out["query"].append({"data": name, "what": what, "bins_each": bins, "capacity": capacity,
                                     "matches": int(d_cur.item()), **t, "bar_ms": bar,
                                     "meets_bar": t["median_ms"] <= bar})
                print(json.dumps(out["query"][-1]), flush=True)
    del data, d_copy, d_ids, d_m
    torch.cuda.empty_cache()

    # sweep against run_device, alternating; a short list and a long one (the
    # list is copied to pageable host memory)
    m = a.m
    d_res = torch.zeros((m, 4), dtype=torch.int32, device=dev)
    out["sweep"] = []
    for capacity in (4096, cap):
        q = pxb.Query(pxb.F_STEP_CAP, pxb.Q_ANY, n_bins_steps=257)
        run_ms, sweep_ms, moved = [], [], None
        for k in range(1 + 5):
            t0 = time.perf_counter()
            pxb.run_device(cfg, 0, m, d_results=d_res, d_totals=d_tot)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ids, matched, n_matches, hs, hr, _ = pxb.sweep(cfg, 0, m, q, capacity)
            t2 = time.perf_counter()
            if k:
                run_ms.append(1e3 * (t1 - t0))
                sweep_ms.append(1e3 * (t2 - t1))
            moved = ids.nbytes + matched.nbytes + hs.nbytes + hr.nbytes + 8 + 8 * pxb.NCOUNTERS
        r, s = stats(run_ms), stats(sweep_ms)
        out["sweep"].append({"config": 4, "n_instances": m, "query": "STEP_CAP, 257 steps bins", "capacity": capacity,
                             "matches": n_matches, "run_device": r, "sweep": s,
                             "sweep_over_run": s["median_ms"] / r["median_ms"],
                             "within_run_spread": r["min_ms"] <= s["median_ms"] <= r["max_ms"],
                             "host_bytes": {"sweep": moved, "pxb_run": 16 * m}})
        print(json.dumps(out["sweep"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
