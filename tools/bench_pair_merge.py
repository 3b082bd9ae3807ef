"""What one Miller pair per distinct signing root of a job (bgv_pair_merge)
costs and gains on the range-sync segment, on one MI355X.  The method of
tools/bench_hash_dedup.py.

Shape: the C4 segment as bench.build_segment makes it, 100,352 sets in 784
jobs of 128 over a 2^20-row table; on-device arrays signed with bgv_gen_sign.
Consecutive sets of a block share a root in runs of g = 1, 2, 4, so a job has
128 / g classes.  bench.py builds every root distinct and cannot show the gain.

Three settings in one process, three contexts each, every shape warmed up
first; the settings alternate inside every repeat:

  off    hash_dedup = 0, one pair per set
  dedup  hash_dedup = 1, one pair per set
  merge  bgv_pair_merge on (which implies the root classes)

  lone       one synchronous bgv_verify at a time, host clock around the call,
             REPS calls per setting, the comparison repeated REPEATS times
  in_flight  three batches in flight on the three contexts of a setting, as
             bench.py's timed step runs them (dist.run_in_flight), REPS steps
             per setting and repeat; per-batch time = elapsed / steps

Reported per leg and g: the p50 of every repeat for the three settings, every
setting's spread (max - min of the repeats' p50), merge against off and
against dedup (a difference counts only beyond the spread of the setting it
is compared with), bgv_pair_stats, bgv_hash_stats, and from the stage events
(batches of this size record them) the hash, key-scaling (which holds the
class sums), set-pair Miller and fold stages.

  python tools/bench_pair_merge.py                 -> profiles/pair_merge.json
  python tools/bench_pair_merge.py --kernels DIR   one `rocprofv3 --kernel-trace --stats` run of its own (a fresh
                                                   child process) at g = 1 and 2: the times of the class pass, the
                                                   class sums, the line and Miller kernels, merged into the JSON

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
OUT = os.path.join(ROOT, "profiles", "pair_merge.json")
BLOCKS, ATT_PER_BLOCK = 784, 125
RUNS = (1, 2, 4)
SETTINGS = (("off", {"hash_dedup": 0}), ("dedup", {"hash_dedup": 1}), ("merge", {"pair_merge": True}))
STAGES = {"hash": 1, "pk_scale": 3, "miller": 6, "fold": 8}  # bgv_stage_name
KERNELS = ("k_pm_claim", "k_pm_link", "k_pm_items", "k_pm_item_job", "k_pm_h", "k_pm_lines", "k_pm_sum", "k_lines",
           "k_miller_steps", "k_miller", "k_job_chain", "k_msg_dedup", "k_hash_reps", "k_hash_spread", "k_hash", "k_pk")


def setup(n_ctx, names=None):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_merge: no GPU visible")
    import bench
    from lodestar_amd import native

    dev = torch.device("cuda", 0)
    ctx = {}
    for name, cfg in SETTINGS:
        if names and name not in names:
            continue
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


def stage_ms(d):
    return {k: float(d.last_stats.stage_ms[i]) for k, i in STAGES.items()}


def lone(d, darr, reps):
    ms, st = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(d, darr)
        ms.append((time.perf_counter() - t0) * 1e3)
        st.append(stage_ms(d))
    return statistics.median(ms), {k: round(statistics.median(s[k] for s in st), 3) for k in STAGES}


def in_flight(ds, darr, reps, torch):
    from concurrent.futures import ThreadPoolExecutor

    from lodestar_amd.dist import run_in_flight
    lat, t_sub, st = [], {}, []
    with ThreadPoolExecutor(max_workers=len(ds)) as ex:
        def submit(k):
            t_sub[k] = time.perf_counter()
            return ex.submit(ds[k % len(ds)].verify, darr, on_device=True, want_set_codes=False, sync_inputs=False)

        def finish(k, res):
            lat.append((time.perf_counter() - t_sub.pop(k)) * 1e3)
            st.append(stage_ms(ds[k % len(ds)]))
            return bool((res[0] == 1).all())

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert run_in_flight(submit, finish, reps, len(ds)), "a batch of the bench did not verify"
        torch.cuda.synchronize()
        per_batch = (time.perf_counter() - t0) * 1e3 / reps
    return per_batch, statistics.median(lat), {k: round(statistics.median(s[k] for s in st), 3) for k in STAGES}


def compare(leg, a, b):
    """setting a against setting b: > 0 means a is faster; a gain or a cost only beyond b's spread"""
    diff = round(statistics.median(leg[b]) - statistics.median(leg[a]), 3)
    spread = leg["spread"][b]
    return {"ms": diff, "spread_of_" + b: spread, "verdict": "gain" if diff > spread else "cost" if -diff > spread else "inside the spread"}


def measure(args):
    torch, dev, bench, ctx, seg = setup(3)
    names = [n for n, _ in SETTINGS]
    out = {"shape": {"n_sets": seg["n_sets"], "n_jobs": seg["n_jobs"], "keys_per_attestation": bench.ATT_K,
                     "table_rows": bench.N_VALIDATORS, "on_device": True},
           "reps": args.reps, "repeats": args.repeats, "unit": "ms", "legs": {}}
    for g in (args.g or RUNS):
        darr = shape(torch, dev, bench, ctx["off"][0], seg, g)
        for name in names:  # every context sizes its buffers for the shape
            for d in ctx[name]:
                call(d, darr)
        leg = {"classes_per_job": 128 // g,
               "pair_stats": {n: ctx[n][0].pair_stats() for n in names},
               "hash_stats": {n: ctx[n][0].hash_stats() for n in names},
               "miller_path": ctx["merge"][0].miller_path(),
               "layout": {k: int(getattr(ctx["merge"][0].last_stats, k)) for k in ("split", "miller_lanes", "pairs_per_item", "lines")},
               "lone": {n: [] for n in names}, "in_flight": {n: [] for n in names}}
        leg["lone"]["stages"] = {n: [] for n in names}
        leg["in_flight"]["stages"] = {n: [] for n in names}
        leg["in_flight"]["latency"] = {n: [] for n in names}
        for _ in range(args.repeats):
            for name in names:
                p50, st = lone(ctx[name][0], darr, args.reps)
                leg["lone"][name].append(round(p50, 3))
                leg["lone"]["stages"][name].append(st)
        for _ in range(args.repeats):
            for name in names:
                per_batch, p50, st = in_flight(ctx[name], darr, args.reps, torch)
                leg["in_flight"][name].append(round(per_batch, 3))
                leg["in_flight"]["latency"][name].append(round(p50, 3))
                leg["in_flight"]["stages"][name].append(st)
        for k in ("lone", "in_flight"):
            leg[k]["spread"] = {n: round(max(leg[k][n]) - min(leg[k][n]), 3) for n in names}
            leg[k]["merge_vs_off"] = compare(leg[k], "merge", "off")
            leg[k]["merge_vs_dedup"] = compare(leg[k], "merge", "dedup")
            leg[k]["dedup_vs_off"] = compare(leg[k], "dedup", "off")
        out["legs"][f"g{g}"] = leg
        print(f"[pair_merge] g={g}", json.dumps(leg), file=sys.stderr, flush=True)
        del darr
    if args.out:  # an A/B run of a variant library (BGV_LIB): its own file
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    else:
        merge(out)
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
    """under the profiler: g = 1 then 2, the merge context then the dedup context, 1 + reps calls each"""
    torch, dev, bench, ctx, seg = setup(1, ("dedup", "merge"))
    for g in (1, 2):
        darr = shape(torch, dev, bench, ctx["dedup"][0], seg, g)
        for name in ("merge", "dedup"):
            for _ in range(1 + args.reps):  # the first call sizes the buffers
                call(ctx[name][0], darr)
        del darr


def kernels(args):
    os.makedirs(args.kernels, exist_ok=True)
    reps = 3
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.kernels, "-o", "pair_merge", "--",
           sys.executable, os.path.abspath(__file__), "--kernels-child", "--reps", str(reps)]
    subprocess.check_call(cmd)
    traces = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit("bench_pair_merge: the profiler left no kernel trace")
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    by = {k: [] for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("bgv::", "").replace("void ", "").strip()
        if name in by:
            by[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    # dispatch order: per g (1, 2), 1 + reps calls on the merge context, then on the dedup context; a kernel both
    # settings launch has 4 (1 + reps) dispatches, one only one of them launches has 2 (1 + reps); gen_sign and the
    # key generation use kernels of their own
    per = 1 + reps
    out = {}
    for k, v in by.items():
        if len(v) == 4 * per:
            out[k] = {"g1_merge_us": round(statistics.median(v[1:per]), 1), "g1_dedup_us": round(statistics.median(v[per + 1:2 * per]), 1),
                      "g2_merge_us": round(statistics.median(v[2 * per + 1:3 * per]), 1),
                      "g2_dedup_us": round(statistics.median(v[3 * per + 1:]), 1)}
        elif len(v) == 2 * per:
            out[k] = {"g1_us": round(statistics.median(v[1:per]), 1), "g2_us": round(statistics.median(v[per + 1:]), 1)}
        elif v:
            out[k] = {"dispatches": len(v), "median_us": round(statistics.median(v), 1)}
    merge({"kernels_us": out, "kernels_source": "rocprofv3 --kernel-trace --stats, one run of its own; median of 3 calls"})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--g", type=int, action="append", help="only these run lengths (default 1, 2, 4)")
    ap.add_argument("--out", default=None, help="write the result here instead of merging it into profiles/pair_merge.json")
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
