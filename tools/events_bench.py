"""Handler-event measurements ("Handler events"): writes
profiles/events_bench.json.  Recorded, not gated: no threshold.

The 4,096 first PANIC ids of a config-3 sweep, as extracted rows at depth 64,
on one GPU:

  events_sizing   pxb_trace_events_device, the sizing call (the count pass and
                  the scan);
  events_full     pxb_trace_events_device with room for every event (count pass,
                  scan, write pass to the staging buffer, reorder);
  trace_full      the yardstick: the same rows through pxb_trace_scripted_device
                  with room for every record, in the same session;
  oracle_scaled   the Python loop the call replaces: tests/event_oracle.py on the
                  first 32 rows, scaled to 4,096 (labelled as scaled).

Host clock around the call and a device synchronise; WARM untimed rounds, then
REPS rounds in which the three device calls alternate, so that drift hits all of
them alike; median [min, max] of each.  Also the bytes each full call writes,
the events and records per row, and whether the events call stays within the
trace call's time scaled by the bytes written, plus 25 %.

python tools/events_bench.py [--reps R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "cloud-haskell-paxos_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
WARM = 3
N, DEPTH, SWEEP, ORACLE_ROWS = 4096, 64, 1 << 18, 32


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "events_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = pxb.CONFIGS[3]
    sweep = SWEEP
    while True:                                              # (a sweep long enough to list N PANIC ids)
        ids, _, n_matches, _, _, _ = pxb.sweep(cfg, 0, sweep, pxb.Query(flag_mask=pxb.F_PANIC, flag_mode=pxb.Q_ANY), N)
        if len(ids) == N or sweep >= 1 << 26:
            break
        sweep *= 4
    assert len(ids) == N, "the sweep lists %d PANIC ids" % len(ids)
    rows = pxb.extract_schedule(cfg, ids, DEPTH)
    d_rows = torch.tensor(rows.reshape(-1), device=dev)
    d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(N, dtype=torch.int32, device=dev)
    d_res = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    pxb.trace_events_device(cfg, d_rows, N, DEPTH, d_off, d_status=d_st, d_results=d_res)
    torch.cuda.synchronize()
    n_events = int(d_off[N].item())
    ok = int((d_st == 0).sum().item())
    pxb.trace_scripted_device(cfg, d_rows, N, DEPTH, d_off, d_status=d_st, d_results=d_res)
    torch.cuda.synchronize()
    n_records = int(d_off[N].item())
    d_ev = torch.zeros(n_events * pxb.EVENT_BYTES, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros((n_records, pxb.TRACE_WORDS), dtype=torch.int32, device=dev)

    def sizing():
        pxb.trace_events_device(cfg, d_rows, N, DEPTH, d_off, d_status=d_st, d_results=d_res)

    def events():
        pxb.trace_events_device(cfg, d_rows, N, DEPTH, d_off, d_ev, n_events, d_st, d_res)

    def trace():
        pxb.trace_scripted_device(cfg, d_rows, N, DEPTH, d_off, d_rec, n_records, d_st, d_res)

    calls = (("events_sizing", sizing), ("events_full", events), ("trace_full", trace))
    ms = {name: [] for name, _ in calls}
    for k in range(WARM + a.reps):
        for j in range(3):                                   # (the order rotates from round to round)
            name, f = calls[(j + k) % 3]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if k >= WARM:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)", "config": 3,
           "rows": N, "depth": DEPTH, "rows_ok": ok, "panic_ids_in_sweep": int(n_matches), "sweep": sweep,
           "events": n_events, "records": n_records, "events_per_row": n_events / N, "records_per_row": n_records / N,
           "event_bytes_written": n_events * pxb.EVENT_BYTES, "record_bytes_written": n_records * pxb.TRACE_WORDS * 4}
    for name, _ in calls:
        out[name] = stats(ms[name])
    ratio_bytes = out["event_bytes_written"] / out["record_bytes_written"]
    ratio_time = out["events_full"]["median_ms"] / out["trace_full"]["median_ms"]
    out["bytes_ratio_events_over_trace"] = ratio_bytes
    out["time_ratio_events_over_trace"] = ratio_time
    out["within_bytes_ratio_plus_25_percent"] = bool(ratio_time <= ratio_bytes * 1.25)

    import event_oracle as EO
    t0 = time.perf_counter()
    n_or = 0
    for i in range(ORACLE_ROWS):
        n_or += len(EO.oracle_events(cfg, rows[i], DEPTH)[0])
    t = 1e3 * (time.perf_counter() - t0)
    out["oracle_scaled"] = {"rows_timed": ORACLE_ROWS, "ms_timed": t, "ms_scaled_to_all_rows": t * N / ORACLE_ROWS,
                            "events_timed": n_or, "note": "Python reference loop on 32 rows, scaled by 128; not measured on all rows"}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
