"""Coverage measurements ("Handler-path coverage"): writes
profiles/cover_bench.json.

On one GPU, in one session:

  rows        the events bench's workload, the first 4,096 PANIC ids of a
              config-3 sweep as extracted rows at depth 64: pxb_cover_device
              (masks, status, results and summary) against
              pxb_trace_events_device's sizing call (capacity 0) over the same
              rows.  The cover kernel runs the same tapped lane, folds instead of
              counting, and writes no events: it may take at most 1.25 x the
              sizing call's median (`within_1_25`; the exit status is 1 beyond it).
  range       pxb.cover_range over 2^20 ids of config 3 (host form, default
              chunk) against pxb_trace_batch_device's sizing call on the same
              ids; the ratio is reported, not bounded.
  host path   what the call replaces: pxb.trace_events plus pxb.cover_of_events
              on the first 32 rows, scaled to 4,096 (labelled as scaled).
  classes     the per-class counts and witnesses over the first 2^20 ids of
              configs 3 and 4.

Host clock around the call and a device synchronise.  WARM untimed rounds, then
three runs of --reps rounds each; within a round the two calls of a pair
alternate and the order flips from round to round.  Each run's median is taken,
and the median and the range of the three run medians are reported.

python tools/cover_bench.py [--reps R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "cloud-haskell-paxos_amd")]
WARM, RUNS = 3, 3
N, DEPTH, SWEEP, HOST_ROWS, RANGE = 4096, 64, 1 << 18, 32, 1 << 20
BOUND = 1.25


def interleaved(pair, reps, sync):
    """{name: {median_ms, min_ms, max_ms, run_medians_ms}} of the two calls of `pair`."""
    runs = {name: [] for name, _ in pair}
    for run in range(RUNS):
        ms = {name: [] for name, _ in pair}
        for k in range((WARM if run == 0 else 1) + reps):
            for j in range(2):
                name, f = pair[(j + k) % 2]
                sync()
                t0 = time.perf_counter()
                f()
                sync()
                if k >= (WARM if run == 0 else 1):
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        for name in ms:
            runs[name].append(statistics.median(ms[name]))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "run_medians_ms": v,
                   "runs": RUNS, "reps_per_run": reps} for name, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "cover_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
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
    d_masks = torch.zeros(N, dtype=torch.int32, device=dev)
    d_sum = torch.zeros(pxb.COVER_SUMMARY_BYTES, dtype=torch.uint8, device=dev)

    def sizing():
        pxb.trace_events_device(cfg, d_rows, N, DEPTH, d_off, d_status=d_st, d_results=d_res)

    def cover():
        pxb.cover_device(cfg, d_rows, N, DEPTH, d_masks, d_st, d_res, d_sum)

    out = {"device": torch.cuda.get_device_name(0), "warm": WARM, "clock": "host (time.perf_counter)", "config": 3,
           "rows": N, "depth": DEPTH, "sweep": sweep, "panic_ids_in_sweep": int(n_matches)}
    out["rows_form"] = interleaved((("events_sizing", sizing), ("cover", cover)), a.reps, sync)
    r = out["rows_form"]["cover"]["median_ms"] / out["rows_form"]["events_sizing"]["median_ms"]
    out["rows_form"]["ratio_cover_over_sizing"] = r
    out["rows_form"]["bound"] = BOUND
    out["rows_form"]["within_1_25"] = bool(r <= BOUND)
    sync()
    s_rows = pxb.cover_summary_from(d_sum.cpu())
    out["rows_form"]["rows_ok"] = s_rows.rows_ok
    out["rows_form"]["counts"] = dict(zip(pxb.COVER_NAMES, s_rows.counts))

    # the range form against the batched trace's sizing call on the same ids
    d_ids = torch.arange(RANGE, dtype=torch.int64, device=dev)
    d_off2 = torch.zeros(RANGE + 1, dtype=torch.int64, device=dev)

    def trace_sizing():
        pxb.trace_batch_device(cfg, d_ids, RANGE, d_off2)

    def cover_range():
        pxb.cover_range(cfg, 0, RANGE)

    out["range_form"] = dict(interleaved((("trace_batch_sizing", trace_sizing), ("cover_range", cover_range)),
                                         max(3, a.reps // 2), sync), ids=RANGE)
    out["range_form"]["ratio_cover_range_over_trace_sizing"] = (
        out["range_form"]["cover_range"]["median_ms"] / out["range_form"]["trace_batch_sizing"]["median_ms"])
    out["range_form"]["ids_per_s"] = RANGE / (1e-3 * out["range_form"]["cover_range"]["median_ms"])

    # the host path the call replaces, on HOST_ROWS rows, scaled
    t0 = time.perf_counter()
    ev, offs, st, _ = pxb.trace_events(cfg, rows[:HOST_ROWS], DEPTH)
    host_masks = [pxb.cover_of_events(ev[int(offs[i]):int(offs[i + 1])], cfg.n_acceptors) for i in range(HOST_ROWS)]
    t = 1e3 * (time.perf_counter() - t0)
    sync()
    assert host_masks == [int(x) & 0xFFFFFFFF for x in d_masks[:HOST_ROWS].cpu().numpy().view(np.uint32)]
    scaled = t * N / HOST_ROWS
    out["host_path_scaled"] = {"rows_timed": HOST_ROWS, "ms_timed": t, "ms_scaled_to_all_rows": scaled,
                               "speed_up_over_cover": scaled / out["rows_form"]["cover"]["median_ms"],
                               "note": "pxb.trace_events + pxb.cover_of_events on 32 rows, scaled by 128; "
                                       "not measured on all rows"}

    # class counts over the first 2^20 ids
    out["class_counts"] = {}
    for c in (3, 4):
        s = pxb.cover_range(pxb.CONFIGS[c], 0, RANGE).summary
        out["class_counts"]["config%d" % c] = {
            "ids": RANGE, "rows_ok": s.rows_ok, "rows_bailed": s.rows_bailed, "counts": dict(zip(pxb.COVER_NAMES, s.counts)),
            "witness": dict(zip(pxb.COVER_NAMES, s.witness)), "witness_steps": dict(zip(pxb.COVER_NAMES, s.witness_steps))}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if out["rows_form"]["within_1_25"] else 1


if __name__ == "__main__":
    sys.exit(main())
