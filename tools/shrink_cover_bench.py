"""Measurements of the shrinker over a coverage predicate (DESIGN.md §3,
"Shrinking over a coverage predicate"): writes profiles/shrink_cover_bench.json.

  (a) the price of the tapped lane and fold
      shrink_bench.py's workload (the first 4,096 PANIC ids of a config-3 sweep
      at depth 64) through pxb.shrink_batch and through pxb.shrink_cover_batch
      with the all-zero query and F_PANIC, which compute the same thing: the two
      alternate, REPS runs each after one untimed run of each, host clock around
      the blocking calls, end to end.  Their outputs must be identical.
  (b) the candidate kernels alone
      --kernels plain|cover: one warm and one measured device call of either, to
      be run under rocprofv3 --kernel-trace --stats in a run of its own each;
      --merge PLAIN_DIR COVER_DIR then sums the candidate kernel's dispatches of
      the second call of either trace.
  (c) a real use
      the Q7_STALE_EXEC ids of config 4's first 2^20 instances (pxb.cover_range)
      shrunk with all = Q7_STALE_EXEC in one pxb.shrink_cover_batch call, against
      the loop of pxb.shrink_cover calls it replaces, timed on 16 of the ids and
      SCALED to all of them.

python tools/shrink_cover_bench.py [--reps R] [--out PATH]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shrink_cover_bench.py --kernels plain
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shrink_cover_bench.py --kernels cover
python tools/shrink_cover_bench.py --merge PLAIN_DIR COVER_DIR [--out PATH]"""
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
sys.path.insert(0, HERE)
from shrink_bench import DEPTH, N_IDS, panic_ids, stats  # noqa: E402

N_LOOP, Q7_RANGE, Q7_CAP = 16, 1 << 20, 4096
KERNEL = {"plain": "paxos_shrink_kernel", "cover": "paxos_shrink_cover_kernel"}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def kernels_only(which):
    """(b): the device call whose kernels the profiler times (one warm call first)."""
    import torch
    import pxb
    assert torch.cuda.is_available(), "shrink_cover_bench needs a GPU"
    dev = torch.device("cuda:0")
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    d_ids = torch.tensor(ids.astype("int64"), device=dev)
    d_rows = torch.zeros(N_IDS * pxb.script_stride(cfg, DEPTH), dtype=torch.uint8, device=dev)
    d_la = torch.zeros(N_IDS, dtype=torch.int32, device=dev)
    for _ in range(2):
        pxb.extract_schedule_device(cfg, d_ids, N_IDS, DEPTH, d_rows)
        if which == "plain":
            pxb.shrink_batch_device(cfg, d_rows, N_IDS, DEPTH, pxb.F_PANIC, d_launches=d_la)
        else:
            pxb.shrink_cover_batch_device(cfg, d_rows, N_IDS, DEPTH, None, pxb.F_PANIC, d_launches=d_la)
        torch.cuda.synchronize()
    print(json.dumps({"which": which, "max_launches_taken": int(d_la.max().item())}))


def candidate_dispatches(prof_dir, kernel):
    rows = []
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if kernel + "<" in r["Kernel_Name"]]   # (a template's instance)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) >= 2 and len(rows) % 2 == 0, "kernel trace: %d dispatches of %s" % (len(rows), kernel)
    return rows[len(rows) // 2:]                         # (the second, warm call)


def merge(path, plain_dir, cover_dir):
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    out = {}
    if os.path.exists(path):
        with open(path) as fh:
            out = json.load(fh)
    per = {}
    for which, d in (("plain", plain_dir), ("cover", cover_dir)):
        cand = candidate_dispatches(d, KERNEL[which])
        per[which] = {"kernel": KERNEL[which], "launches": len(cand),
                      "candidates_rounded_to_64": [int(r["Grid_Size_X"]) for r in cand],
                      "vgprs": int(cand[0]["VGPR_Count"]), "scratch": int(cand[0]["Scratch_Size"]),
                      "total_ms": sum(us(r) for r in cand) / 1e3}
    assert per["plain"]["candidates_rounded_to_64"] == per["cover"]["candidates_rounded_to_64"], "different launches"
    out["candidate_kernels"] = {
        "method": "rocprofv3 --kernel-trace --stats, a run of its own each; the second of two device calls",
        **per, "cover_over_plain": per["cover"]["total_ms"] / per["plain"]["total_ms"],
        "yardstick": "pxb_explore_cover's candidate kernel over pxb_explore's: 1.28"}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["candidate_kernels"]))


def price(pxb, np, reps):
    cfg = pxb.CONFIGS[3]
    ids = panic_ids(pxb)
    plain = lambda: pxb.shrink_batch(cfg, ids, pxb.F_PANIC, depth=DEPTH, chunk=N_IDS)  # noqa: E731
    cover = lambda: pxb.shrink_cover_batch(cfg, ids, None, pxb.F_PANIC, depth=DEPTH, chunk=N_IDS)  # noqa: E731
    p, c = plain(), cover()                              # (untimed)
    same = all(np.array_equal(a, b) for a, b in zip(p, c[:7]))
    masks_ok = bool(np.array_equal(c[7], pxb.cover(cfg, c[0], DEPTH)[0]))
    tp, tc = [], []
    for _ in range(reps):
        tp.append(clock(plain)[0])
        tc.append(clock(cover)[0])
    return {"config": 3, "ids": N_IDS, "depth": DEPTH, "flag_mask": "F_PANIC", "query": "all-zero",
            "order": "plain, cover alternating, %d each after one untimed run of each" % reps,
            "shrink_batch": stats(tp), "shrink_cover_batch": stats(tc),
            "cover_over_plain_medians": statistics.median(tc) / statistics.median(tp),
            "outputs_identical": bool(same), "masks_equal_pxb_cover_of_returned_rows": masks_ok}


def real_use(pxb, np):
    cfg = pxb.CONFIGS[4]
    q = pxb.CoverQuery(all_mask=pxb.COVER_Q7_STALE_EXEC)
    t_find, found = clock(lambda: pxb.cover_range(cfg, 0, Q7_RANGE, q, Q7_CAP))
    ids = found.match_ids
    assert 0 < len(ids) == found.summary.n_matches, "the list holds %d of %d" % (len(ids), found.summary.n_matches)
    pxb.shrink_cover_batch(cfg, ids[:64], q, depth=DEPTH)                    # (untimed)
    t_batch, o = clock(lambda: pxb.shrink_cover_batch(cfg, ids, q, depth=DEPTH))
    _, status, n_faults, launches, _, _, sig, masks = o
    sub = [int(i) for i in ids[:N_LOOP]]

    def loop():
        for i in sub:
            try:
                pxb.shrink_cover(cfg, i, q, depth=DEPTH)
            except ValueError:                           # (not an input within the depth: its one launch is counted)
                pass
    loop_ms = clock(loop)[0]
    shrunk = (status == pxb.SHRINK_MINIMAL) | (status == pxb.SHRINK_BUDGET)
    csig, ccnt = pxb.shrink_clusters(sig, status)
    return {"config": 4, "range": "0..2^20-1", "query": "all = Q7_STALE_EXEC", "depth": DEPTH, "max_launches": 64,
            "ids": int(len(ids)), "cover_range_ms": t_find, "shrink_cover_batch_ms": t_batch,
            "status_counts": {str(k): int((status == k).sum()) for k in range(5)},
            "launches": {"min": int(launches[shrunk].min()), "median": float(np.median(launches[shrunk])),
                         "max": int(launches.max())},
            "faults_left": {"min": int(n_faults[shrunk].min()), "median": float(np.median(n_faults[shrunk])),
                            "max": int(n_faults[shrunk].max())},
            "every_returned_mask_has_q7": bool((masks[shrunk] & pxb.COVER_Q7_STALE_EXEC).all()),
            "distinct_signatures": int(len(csig)),
            "largest_clusters": [{"signature": "%016x" % int(s), "rows": int(n)} for s, n in zip(csig[:5], ccnt[:5])],
            "loop": {"what": "pxb.shrink_cover per id, %d ids timed once" % N_LOOP, "ms": loop_ms,
                     "SCALED_to_all_ids_ms": loop_ms * len(ids) / N_LOOP},
            "scaled_loop_over_batch": loop_ms * len(ids) / N_LOOP / t_batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink_cover_bench.json"))
    ap.add_argument("--kernels", choices=("plain", "cover"), default=None)
    ap.add_argument("--merge", nargs=2, default=None, metavar=("PLAIN_DIR", "COVER_DIR"))
    a = ap.parse_args()
    if a.merge:
        return merge(a.out, *a.merge)
    if a.kernels:
        return kernels_only(a.kernels)
    import numpy as np
    import torch
    import pxb
    assert torch.cuda.is_available(), "shrink_cover_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "clock": "host (time.perf_counter)"}
    out["price"] = price(pxb, np, a.reps)
    print(json.dumps(out["price"]), flush=True)
    out["real_use"] = real_use(pxb, np)
    print(json.dumps(out["real_use"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
