"""Measure same-message batch verification of aggregate sets against the
ordinary pipeline.

Two shapes: 64 groups x 16 sets x 128 keys (one slot of gossip aggregates: 16
aggregators per committee) and 64 groups x 2 sets x 440 keys (a block-import
mix: two aggregates of one committee and data); and, beside them, a batch that
fills the device: 2,048 groups x 16 sets x 128 keys (an epoch's gossip
aggregates in one call, e.g. a backlog after a stall).  Two paths over the same
signed sets, host arrays in both:
  (a) Device.verify_same_message_agg (bgv_verify_same_message_agg);
  (b) Device.verify with every set as a one-set job, its message replicated
      (the ordinary pipeline, which this path leaves untouched).
Both shapes are warmed up first; then the paths alternate in one process,
REPS times each (synchronised host clock around the call: both calls return
with their results on the host), and the whole comparison runs three times.
Writes the p50 of each path per repeat and the spread across the repeats to
profiles/same_message_agg.json.  Needs a HIP device: there is no CPU fallback.

    python tools/bench_same_message_agg.py [--reps 20] [--out profiles/same_message_agg.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lodestar_amd import native  # noqa: E402

SHAPES = [("gossip_aggregates_64x16x128", 64, 16, 128), ("block_import_64x2x440", 64, 2, 440),
          ("epoch_backlog_2048x16x128", 2048, 16, 128)]
N_KEYS = 1 << 15


def make(dev, groups, per_group, keys_per_set, seed):
    rng = np.random.default_rng(seed)
    n = groups * per_group
    idx = rng.integers(0, N_KEYS, size=n * keys_per_set).astype(np.uint32)
    pk_off = (np.arange(n + 1) * keys_per_set).astype(np.uint32)
    gmsgs = rng.integers(0, 256, size=(groups, 32), dtype=np.uint8)
    msgs = np.repeat(gmsgs, per_group, axis=0)
    jobs = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": pk_off, "pk_indices": idx,
            "msgs": np.ascontiguousarray(msgs)}
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign(jobs, sigs)
    jobs["sigs"] = sigs
    jobs["sig_len"] = np.full(n, 96, np.uint32)
    sma = {"n_sets": n, "n_groups": groups, "group_offsets": (np.arange(groups + 1) * per_group).astype(np.uint32),
           "pk_offsets": pk_off, "pk_indices": idx, "msgs": gmsgs, "sigs": sigs, "sig_len": jobs["sig_len"]}
    return sma, jobs


def run_a(dev, sma):
    t0 = time.perf_counter()
    ok, _ = dev.verify_same_message_agg(sma)
    dt = time.perf_counter() - t0
    assert ok.all() and dev.last_sm_stats.groups_retried == 0
    return dt * 1e3


def run_b(dev, jobs):
    t0 = time.perf_counter()
    jr, _ = dev.verify(jobs, want_set_codes=False)
    dt = time.perf_counter() - t0
    assert (jr == 1).all()
    return dt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "same_message_agg.json"))
    args = ap.parse_args()
    if args.reps < 20 or args.repeats < 3:
        ap.error("at least 20 repetitions per path and 3 repeats of the comparison")
    dev = native.Device(0)  # raises without a device
    try:
        dev.gen_keys(0, N_KEYS, 0x534D4147)
        data = {name: make(dev, g, k, m, 13 + g * k * m) for name, g, k, m in SHAPES}
        for name, *_ in SHAPES:  # warm-up of both shapes, both paths
            for _ in range(3):
                run_a(dev, data[name][0])
                run_b(dev, data[name][1])
        out = {"reps": args.reps, "repeats": args.repeats, "clock": "host perf_counter around the synchronous call", "shapes": {}}
        for name, g, k, m in SHAPES:
            sma, jobs = data[name]
            p50a, p50b = [], []
            for _ in range(args.repeats):
                ta, tb = [], []
                for _ in range(args.reps):  # alternating
                    ta.append(run_a(dev, sma))
                    tb.append(run_b(dev, jobs))
                p50a.append(float(np.median(ta)))
                p50b.append(float(np.median(tb)))
            st = dev.last_sm_stats.as_dict()
            spread_b = max(p50b) - min(p50b)
            res = {"groups": g, "sets_per_group": k, "keys_per_set": m, "n_sets": g * k, "n_keys": g * k * m,
                   "segments": st["n_segments"], "hashes": st["hashes"], "pairs": st["pairs"],
                   "same_message_agg_p50_ms": p50a, "one_set_jobs_p50_ms": p50b,
                   "same_message_agg_spread_ms": max(p50a) - min(p50a), "one_set_jobs_spread_ms": spread_b,
                   "speedup_p50": float(np.median(p50b) / np.median(p50a)),
                   "faster_by_more_than_the_spread": bool(max(p50a) < min(p50b) - spread_b)}
            out["shapes"][name] = res
            print(json.dumps({name: res}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
