"""Batched-trace measurements ("Batched trace"): writes
profiles/trace_batch_bench.json.

  (a) batch vs loop   4,096 ids from a config-3 panic sweep traced with one
                      pxb.trace_batch call (tail = 8, and every record; each
                      sizes its buffer with the count-only call first, so it
                      is two pxb_trace_batch calls) against the only way
                      before it: a host loop of pxb.trace_instance, timed on
                      the first 256 of the same ids and scaled by 16 (that
                      code is unchanged).  Host clock around blocking calls,
                      WARM untimed and REPS timed repeats, median [min, max].
                      Bar: the batched median below the loop's minimum.
  (b) sizing call     the count pass alone (capacity = 0) over 2^16
                      contiguous config-4 ids beside pxb_run_device over the
                      same range (another shape and variant: no bar), host
                      clock around the call and a device synchronise.
  (c) write pass      --kernels: one device call with every record and one with
                      tail = 8 and nothing else, to be run under
                      rocprofv3 --kernel-trace --stats in a run of its own;
                      --merge DIR then reads that run's kernel trace (the
                      dispatches of paxos_trace_batch_kernel alternate: count,
                      write, count, write) and records bytes written / kernel
                      time.

python tools/trace_batch_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trace_batch_bench.py --kernels
python tools/trace_batch_bench.py --merge DIR [--out PATH]"""
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
WARM = 3
N_IDS, N_LOOP, SWEEP_N = 4096, 256, 1 << 14
RECORD_BYTES = 292


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
    """(c): the two device calls whose kernels the profiler times."""
    import torch
    import pxb
    assert torch.cuda.is_available(), "trace_batch_bench needs a GPU"
    dev = torch.device("cuda:0")
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    d_ids = torch.tensor(ids.astype("int64"), device=dev)
    d_off = torch.zeros(N_IDS + 1, dtype=torch.int64, device=dev)
    out = {}
    for name, tail in (("all", 0), ("tail8", 8)):
        pxb.trace_batch_device(cfg, d_ids, N_IDS, d_off, tail=tail)          # (sizing, on the host side only)
        torch.cuda.synchronize()
        total = int(d_off[-1].item())
        out[name] = {"records": total, "bytes": total * RECORD_BYTES}
    # one warm pair, then the profiled pair: its dispatches are the kernel's last four
    for _ in range(2):
        for name, tail in (("all", 0), ("tail8", 8)):
            d_rec = torch.zeros((out[name]["records"], pxb.TRACE_WORDS), dtype=torch.int32, device=dev)
            pxb.trace_batch_device(cfg, d_ids, N_IDS, d_off, d_rec, out[name]["records"], tail=tail)
            torch.cuda.synchronize()
    print(json.dumps(out))


def merge(path, prof_dir):
    rows = []
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "paxos_trace_batch_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) >= 4, "kernel trace: %d dispatches of paxos_trace_batch_kernel" % len(rows)
    dur = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[-4:]]
    with open(os.path.join(prof_dir, "kernels.json")) as fh:
        sizes = json.loads(fh.read().strip().splitlines()[-1])
    with open(path) as fh:
        out = json.load(fh)
    out["write_pass"] = {"method": "rocprofv3 --kernel-trace --stats, a run of its own; one dispatch each", "ids": N_IDS}
    for k, name in enumerate(("all", "tail8")):
        cnt_ns, wr_ns = dur[2 * k], dur[2 * k + 1]
        out["write_pass"][name] = {**sizes[name], "count_kernel_us": cnt_ns / 1e3, "write_kernel_us": wr_ns / 1e3,
                                   "write_gb_per_s": sizes[name]["bytes"] / wr_ns}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["write_pass"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_batch_bench.json"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.out, a.merge)
    if a.kernels:
        return kernels_only()
    import torch
    import pxb
    assert torch.cuda.is_available(), "trace_batch_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)"}

    # (a) one batched call against the loop of single traces
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    sub = [int(i) for i in ids[:N_LOOP]]
    scale = N_IDS // N_LOOP

    def loop():
        for i in sub:
            pxb.trace_instance(cfg, i, max_records=cfg.step_cap)
    lp = timed(loop, a.reps)
    rec_all, offs_all, status, _ = pxb.trace_batch(cfg, ids)
    a_out = {"config": 3, "ids": N_IDS, "ids_from": "pxb.sweep(F_PANIC) over instances 0..%d" % (SWEEP_N - 1),
             "bailed": int((status != 0).sum()),
             "loop": {"what": "pxb.trace_instance(max_records=step_cap), %d ids, scaled by %d" % (N_LOOP, scale),
                      **{k: (v * scale if k.endswith("_ms") else v) for k, v in lp.items()}}}
    for name, tail in (("tail8", 8), ("all", 0)):
        t = timed(lambda: pxb.trace_batch(cfg, ids, tail=tail), a.reps)
        rec, _, _, _ = pxb.trace_batch(cfg, ids, tail=tail)
        a_out[name] = {"what": "pxb.trace_batch(tail=%d), sizing call included" % tail, "records": len(rec),
                       "record_bytes": len(rec) * RECORD_BYTES, **t,
                       "loop_min_over_median": a_out["loop"]["min_ms"] / t["median_ms"],
                       "meets_bar": t["median_ms"] < a_out["loop"]["min_ms"]}
    out["batch_vs_loop"] = a_out
    print(json.dumps(a_out), flush=True)

    # (b) the sizing call beside the batch run of the same ids
    cfg4, n = pxb.CONFIGS[4], 1 << 16
    d_ids = torch.arange(n, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_res = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_tot = torch.zeros(pxb.NCOUNTERS, dtype=torch.int64, device=dev)

    def sizing():
        pxb.trace_batch_device(cfg4, d_ids, n, d_off, d_status=d_st, d_results=d_res)
        torch.cuda.synchronize()

    def run():
        pxb.run_device(cfg4, 0, n, d_results=d_res, d_totals=d_tot)
        torch.cuda.synchronize()
    s, r = timed(sizing, a.reps), timed(run, a.reps)
    out["sizing_call"] = {"config": 4, "ids": n, "count_pass": s, "run_device": r, "records": int(d_off[-1].item()),
                          "bailed": int(d_st.sum().item()), "count_over_run": s["median_ms"] / r["median_ms"]}
    print(json.dumps(out["sizing_call"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
