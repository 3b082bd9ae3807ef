"""Measure the split retry of the same-message entries against the per-set retry.

Device.verify_same_message (bgv_verify_same_message) on one context with
bgv_sm_retry mode 0 (every surviving set of a failing segment as a one-set job
of the ordinary pipeline: the baseline) and mode 1 (subs of 8, then the sets of
the failing subs), on identical host-resident batches, in one process,
alternating.  The shapes of tools/bench_same_message.py (64 groups x 64 sets,
and 64 x 488: one slot's committees), each clean, with 0.1 % and with 1 % of
the signatures replaced by wrong-message ones (a seeded choice).
Every case is warmed up first; then the two modes alternate REPS times
(synchronised host clock around the call: it returns with its results on the
host), and the whole comparison runs three times.  Reported per case: the p50
of each mode per repeat, the spread of mode 0 across the repeats, the
difference of the medians, whether it exceeds that spread, and the retry
counters of both modes (bgv_sm_retry_stats).  Writes profiles/sm_retry.json.
Needs a HIP device: there is no CPU fallback.

    python tools/bench_same_message_retry.py [--reps 20] [--out profiles/sm_retry.json]
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

RATES = [("clean", 0.0), ("0.1pct_wrong_message", 0.001), ("1pct_wrong_message", 0.01)]


def with_faults(dev, sm, rate, seed):
    """rate of the sets carry a valid signature over another message: they pass the decode and fail the pairing"""
    n = sm["n_sets"]
    if rate == 0.0:
        return sm, np.zeros(0, np.int64)
    rng = np.random.default_rng(seed)
    bad = np.sort(rng.choice(n, size=max(1, int(round(n * rate))), replace=False))
    other = np.frombuffer(b"\x5a" * 32, np.uint8)
    jobs = {"n_sets": len(bad), "n_jobs": len(bad), "job_offsets": np.arange(len(bad) + 1, dtype=np.uint32),
            "pk_offsets": np.arange(len(bad) + 1, dtype=np.uint32), "pk_indices": np.ascontiguousarray(sm["pk_indices"][bad]),
            "msgs": np.ascontiguousarray(np.stack([other] * len(bad)))}
    wrong = np.zeros((len(bad), 192), np.uint8)
    dev.gen_sign(jobs, wrong)
    sigs = sm["sigs"].copy()
    sigs[bad] = wrong
    return dict(sm, sigs=sigs), bad


def run(dev, mode, sm, bad):
    dev.sm_retry(mode)
    t0 = time.perf_counter()
    ok, _ = dev.verify_same_message(sm)
    dt = time.perf_counter() - t0
    assert np.nonzero(~ok)[0].tolist() == bad.tolist()
    return dt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sm_retry.json"))
    args = ap.parse_args()
    if args.reps < 20 or args.repeats < 3:
        ap.error("at least 20 repetitions per mode and 3 repeats of the comparison")
    dev = native.Device(0)  # raises without a device
    try:
        dev.gen_keys(0, N_KEYS, 0x534D424E)
        cases = []
        for name, g, k in SHAPES:
            sm, _ = make(dev, g, k, 11 + g * k)
            for tag, rate in RATES:
                faulty, bad = with_faults(dev, sm, rate, 29 + g * k)
                cases.append((f"{name}_{tag}", g, k, faulty, bad))
        for _, _, _, sm, bad in cases:  # warm-up of every case, both modes
            for _ in range(3):
                run(dev, 0, sm, bad)
                run(dev, 1, sm, bad)
        out = {"reps": args.reps, "repeats": args.repeats, "clock": "host perf_counter around the synchronous call",
               "baseline": "mode 0: the per-set retry through the ordinary pipeline, same run, same context", "cases": {}}
        for name, g, k, sm, bad in cases:
            p50 = {0: [], 1: []}
            path = {}
            for _ in range(args.repeats):
                t = {0: [], 1: []}
                for _ in range(args.reps):  # alternating
                    for mode in (0, 1):
                        t[mode].append(run(dev, mode, sm, bad))
                        path[mode] = dev.sm_retry_stats()
                for mode in (0, 1):
                    p50[mode].append(float(np.median(t[mode])))
            st = dev.last_sm_stats.as_dict()
            spread0 = max(p50[0]) - min(p50[0])
            delta = float(np.median(p50[1]) - np.median(p50[0]))
            res = {"groups": g, "sets_per_group": k, "n_sets": g * k, "bad_sets": int(len(bad)), "segments": st["n_segments"],
                   "sets_retried": st["sets_retried"],
                   "mode0_p50_ms": p50[0], "mode1_p50_ms": p50[1],
                   "mode0_spread_ms": spread0, "mode1_spread_ms": max(p50[1]) - min(p50[1]),
                   "mode1_minus_mode0_ms": delta,
                   "verdict": "within the spread" if abs(delta) <= spread0 else ("mode 1 faster" if delta < 0 else "mode 1 slower"),
                   "retry_mode0": path[0], "retry_mode1": path[1]}
            out["cases"][name] = res
            print(json.dumps({name: res}), flush=True)
        dev.sm_retry(0)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
