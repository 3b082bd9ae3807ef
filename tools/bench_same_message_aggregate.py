"""Measure what the per-group aggregate signatures cost a same-message call.

Device.verify_same_message (bgv_verify_same_message) against
Device.verify_same_message_aggregate (bgv_verify_same_message_aggregate) on
identical host-resident batches, in one process, alternating.  The shapes of
tools/bench_same_message.py (64 groups x 64 sets, and 64 x 488: one slot's
committees, a batch that fills the device), each clean and with 1% of the
signatures replaced by wrong-message ones, so the per-set retry and with it
the second pass of the sums run.
Both shapes are warmed up first; then the two calls alternate REPS times
(synchronised host clock around the call: both return with their results on
the host), and the whole comparison runs three times.  Reported per shape:
the p50 of each call per repeat, the spread of each across the repeats, their
difference, and the device time of the two sum kernels of the first pass
(HIP events on the pubkey stream, bgv_sm_agg_ms).  Writes
profiles/same_message_aggregate.json.  Needs a HIP device: there is no CPU
fallback.

    python tools/bench_same_message_aggregate.py [--reps 20] [--out profiles/same_message_aggregate.json]
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
from tools.bench_same_message import N_KEYS, SHAPES, make  # noqa: E402


def with_faults(dev, sm, seed):
    """1% of the sets carry a valid signature over another message: they pass the decode and fail the pairing"""
    rng = np.random.default_rng(seed)
    n = sm["n_sets"]
    bad = np.sort(rng.choice(n, size=max(1, n // 100), replace=False))
    other = np.frombuffer(b"\x5a" * 32, np.uint8)
    jobs = {"n_sets": len(bad), "n_jobs": len(bad), "job_offsets": np.arange(len(bad) + 1, dtype=np.uint32),
            "pk_offsets": np.arange(len(bad) + 1, dtype=np.uint32), "pk_indices": np.ascontiguousarray(sm["pk_indices"][bad]),
            "msgs": np.ascontiguousarray(np.stack([other] * len(bad)))}
    wrong = np.zeros((len(bad), 192), np.uint8)
    dev.gen_sign(jobs, wrong)
    sigs = sm["sigs"].copy()
    sigs[bad] = wrong
    return dict(sm, sigs=sigs), bad


def run_plain(dev, sm, n_bad):
    t0 = time.perf_counter()
    ok, _ = dev.verify_same_message(sm)
    dt = time.perf_counter() - t0
    assert int((~ok).sum()) == n_bad
    return dt * 1e3


def run_aggregate(dev, sm, n_bad):
    t0 = time.perf_counter()
    out = dev.verify_same_message_aggregate(sm)
    dt = time.perf_counter() - t0
    assert int((~out["set_valid"]).sum()) == n_bad and int(out["agg_count"].sum()) == sm["n_sets"] - n_bad
    return dt * 1e3, dev.sm_agg_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "same_message_aggregate.json"))
    args = ap.parse_args()
    if args.reps < 20 or args.repeats < 3:
        ap.error("at least 20 repetitions per call and 3 repeats of the comparison")
    dev = native.Device(0)  # raises without a device
    try:
        dev.gen_keys(0, N_KEYS, 0x534D424E)
        cases = []
        for name, g, k in SHAPES:
            sm, _ = make(dev, g, k, 11 + g * k)
            cases.append((name + "_clean", g, k, sm, 0))
            faulty, bad = with_faults(dev, sm, 29 + g * k)
            cases.append((name + "_1pct_wrong_message", g, k, faulty, len(bad)))
        for _, _, _, sm, n_bad in cases:  # warm-up of every case, both calls
            for _ in range(3):
                run_plain(dev, sm, n_bad)
                run_aggregate(dev, sm, n_bad)
        out = {"reps": args.reps, "repeats": args.repeats, "clock": "host perf_counter around the synchronous call",
               "kernel_clock": "HIP events around k_sm_sig_seg + k_sm_sig_group of the first pass", "cases": {}}
        for name, g, k, sm, n_bad in cases:
            p50a, p50b, kern = [], [], []
            for _ in range(args.repeats):
                ta, tb = [], []
                for _ in range(args.reps):  # alternating
                    ta.append(run_plain(dev, sm, n_bad))
                    t, km = run_aggregate(dev, sm, n_bad)
                    tb.append(t)
                    kern.append(km)
                p50a.append(float(np.median(ta)))
                p50b.append(float(np.median(tb)))
            st = dev.last_sm_stats.as_dict()
            spread_a = max(p50a) - min(p50a)
            delta = float(np.median(p50b) - np.median(p50a))
            res = {"groups": g, "sets_per_group": k, "n_sets": g * k, "bad_sets": n_bad, "segments": st["n_segments"],
                   "sets_retried": st["sets_retried"],
                   "plain_p50_ms": p50a, "aggregate_p50_ms": p50b,
                   "plain_spread_ms": spread_a, "aggregate_spread_ms": max(p50b) - min(p50b),
                   "aggregate_minus_plain_ms": delta,
                   "slower_by_more_than_the_plain_spread": bool(delta > spread_a),
                   "sum_kernels_ms_p50": float(np.median(kern)), "sum_kernels_ms_max": float(np.max(kern))}
            out["cases"][name] = res
            print(json.dumps({name: res}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
