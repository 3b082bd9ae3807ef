"""What hashing each distinct signing root once (bgv_cfg.hash_dedup) costs and
gains on the range-sync segment, on one MI355X.

Shape: the C4 segment as bench.build_segment makes it, 100,352 sets in 784
jobs of 128 (125 attestation aggregates of 128 keys, the sync aggregate and two
singles per block) over a 2^20-row table; on-device arrays signed with
bgv_gen_sign.  Duplicate structure: consecutive sets of a block share a root in
runs of g = 1, 2, 4, i.e. a share delta = 0, 50, 75 % of the sets repeat an
earlier root.  bench.py builds every root distinct and cannot show the gain.

Two settings in one process, hash_dedup = 0 ("off") and 1 ("on"), three contexts each,
every shape warmed up first; the settings alternate inside every repeat:

  lone       one synchronous bgv_verify at a time, host clock around the call,
             REPS calls per setting, the comparison repeated REPEATS times
  in_flight  three batches in flight on the three contexts of a setting, as
             bench.py's timed step runs them (dist.run_in_flight), REPS steps
             per setting and repeat; per-batch time = elapsed / steps

Reported per leg and delta: the p50 of every repeat for both settings, the
spread (max - min of the repeats' p50) of the off setting, bgv_hash_stats and
stage_ms[hash_to_g2] (batches of this size record per-stage events).

  python tools/bench_hash_dedup.py                 -> profiles/hash_dedup.json
  python tools/bench_hash_dedup.py --kernels DIR   one `rocprofv3 --kernel-trace --stats` run of its own (a fresh
                                                   child process) at delta = 0 and 50 %; the times of k_msg_dedup,
                                                   k_hash_reps, k_hash_spread and k_hash are merged into the JSON

A path that finds no GPU fails; nothing falls back."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "hash_dedup.json")
BLOCKS, ATT_PER_BLOCK = 784, 125
RUNS = (1, 2, 4)
HASH_STAGE = 1  # bgv_stage_name(1) == "hash_to_g2"
KERNELS = ("k_msg_dedup", "k_hash_reps", "k_hash_spread", "k_hash")


def setup(n_ctx):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_hash_dedup: no GPU visible")
    import bench
    from lodestar_amd import native

    dev = torch.device("cuda", 0)
    ctx = {}
    for name, cfg in (("off", {"hash_dedup": 0}), ("on", {"hash_dedup": 1})):
        ctx[name] = []
        for _ in range(n_ctx):
            d = native.Device(0, **cfg)
            d.gen_keys(0, bench.N_VALIDATORS, bench.SEED)
            ctx[name].append(d)
    seg = bench.build_segment(list(range(BLOCKS)), att_per_block=ATT_PER_BLOCK)
    assert seg["n_sets"] == 100352 and seg["n_jobs"] == BLOCKS
    return torch, dev, bench, ctx, seg


def shape(torch, dev, bench, signer, seg, g):
    """the segment with roots shared in runs of g, on the device and signed"""
    a = dict(seg)
    n = seg["n_sets"]
    a["msgs"] = np.ascontiguousarray(seg["msgs"][(np.arange(n) // g) * g])  # 128 % g == 0: runs stay inside a block
    darr = bench.to_device(a, torch, dev)
    sigs = torch.zeros((n, 192), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    signer.gen_sign(darr, sigs, on_device=True)
    darr["sigs"] = sigs
    darr["sig_len"] = torch.full((n,), 96, dtype=torch.int32, device=dev)
    darr["scalars"] = None
    torch.cuda.synchronize()
    return darr


def call(d, darr):
    jr, _ = d.verify(darr, on_device=True, want_set_codes=False, sync_inputs=False)
    assert (jr == 1).all(), "a batch of the bench did not verify"


def lone(d, darr, reps):
    ms, hash_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(d, darr)
        ms.append((time.perf_counter() - t0) * 1e3)
        hash_ms.append(float(d.last_stats.stage_ms[HASH_STAGE]))
    return statistics.median(ms), statistics.median(hash_ms)


def in_flight(ds, darr, reps, torch):
    from concurrent.futures import ThreadPoolExecutor

    from lodestar_amd.dist import run_in_flight
    lat, t_sub, hash_ms = [], {}, []
    with ThreadPoolExecutor(max_workers=len(ds)) as ex:
        def submit(k):
            t_sub[k] = time.perf_counter()
            return ex.submit(ds[k % len(ds)].verify, darr, on_device=True, want_set_codes=False, sync_inputs=False)

        def finish(k, res):
            lat.append((time.perf_counter() - t_sub.pop(k)) * 1e3)
            hash_ms.append(float(ds[k % len(ds)].last_stats.stage_ms[HASH_STAGE]))
            return bool((res[0] == 1).all())

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert run_in_flight(submit, finish, reps, len(ds)), "a batch of the bench did not verify"
        torch.cuda.synchronize()
        per_batch = (time.perf_counter() - t0) * 1e3 / reps
    return per_batch, statistics.median(lat), statistics.median(hash_ms)


def measure(args):
    torch, dev, bench, ctx, seg = setup(3)
    out = {"shape": {"n_sets": seg["n_sets"], "n_jobs": seg["n_jobs"], "keys_per_attestation": bench.ATT_K,
                     "table_rows": bench.N_VALIDATORS, "on_device": True},
           "reps": args.reps, "repeats": args.repeats, "unit": "ms", "legs": {}}
    for g in RUNS:
        darr = shape(torch, dev, bench, ctx["off"][0], seg, g)
        for name in ("off", "on"):  # every context sizes its buffers for the shape
            for d in ctx[name]:
                call(d, darr)
        stats = {name: ctx[name][0].hash_stats() for name in ("off", "on")}
        leg = {"delta_pct": round(100 * (1 - 1 / g)), "hash_stats": stats,
               "lone": {"off": [], "on": [], "hash_stage_off": [], "hash_stage_on": []},
               "in_flight": {"off": [], "on": [], "latency_off": [], "latency_on": [], "hash_stage_off": [],
                             "hash_stage_on": []}}
        for _ in range(args.repeats):
            for name in ("off", "on"):
                p50, h = lone(ctx[name][0], darr, args.reps)
                leg["lone"][name].append(round(p50, 3))
                leg["lone"]["hash_stage_" + name].append(round(h, 3))
        for _ in range(args.repeats):
            for name in ("off", "on"):
                per_batch, p50, h = in_flight(ctx[name], darr, args.reps, torch)
                leg["in_flight"][name].append(round(per_batch, 3))
                leg["in_flight"]["latency_" + name].append(round(p50, 3))
                leg["in_flight"]["hash_stage_" + name].append(round(h, 3))
        for k in ("lone", "in_flight"):
            off, on = leg[k]["off"], leg[k]["on"]
            leg[k]["off_spread"] = round(max(off) - min(off), 3)
            leg[k]["gain"] = round(statistics.median(off) - statistics.median(on), 3)  # > 0: on is faster
            leg[k]["beyond_off_spread"] = abs(leg[k]["gain"]) > leg[k]["off_spread"]
        out["legs"][f"g{g}"] = leg
        print(f"[hash_dedup] g={g}", json.dumps(leg), file=sys.stderr, flush=True)
        del darr
    merge({k: v for k, v in out.items()})
    print(json.dumps(out))


def merge(update):
    cur = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            cur = json.load(f)
    cur.update(update)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
        f.write("\n")


def kernels_child(args):
    """under the profiler: delta = 0 then 50 %, the on context then the off context, `reps` calls each"""
    torch, dev, bench, ctx, seg = setup(1)
    for g in (1, 2):
        darr = shape(torch, dev, bench, ctx["off"][0], seg, g)
        for name in ("on", "off"):
            for _ in range(1 + args.reps):  # the first call sizes the buffers
                call(ctx[name][0], darr)
        del darr


def kernels(args):
    os.makedirs(args.kernels, exist_ok=True)
    reps = 3
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.kernels, "-o", "hash_dedup", "--",
           sys.executable, os.path.abspath(__file__), "--kernels-child", "--reps", str(reps)]
    subprocess.check_call(cmd)
    traces = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit("bench_hash_dedup: the profiler left no kernel trace")
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    by = {k: [] for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("bgv::", "").replace("void ", "").strip()
        if name in by:
            by[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    # dispatch order: per delta (0, 50 %), 1 + reps calls on the on context (the three new kernels), then on the off
    # context (k_hash); gen_sign hashes with a kernel of its own
    per = 1 + reps
    out = {}
    for k, v in by.items():
        assert len(v) == 2 * per, (k, len(v))
        out[k] = {"delta_0_us": round(statistics.median(v[1:per]), 1), "delta_50_us": round(statistics.median(v[per + 1:]), 1)}
    merge({"kernels_us": out, "kernels_source": "rocprofv3 --kernel-trace --stats, one run of its own; median of 3 calls"})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels", metavar="DIR", default=None)
    ap.add_argument("--kernels-child", action="store_true")
    args = ap.parse_args()
    if args.kernels_child:
        kernels_child(args)
    elif args.kernels:
        kernels(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
