"""Measure same-message batches of committee sets (bgv_verify_same_message_bits)
against the same sets as explicit index lists (bgv_verify_same_message_agg).

One process, one device, two contexts that hold the same 2^20-key table and the
same resident 2^20-entry shuffling (a permutation of the table): one without
sums, one with (bgv_index_list_sums).  Three paths over the same signed sets,
host arrays in all of them:
  (e)  Device.verify_same_message_agg on the explicit lists: the baseline, the
       entry and kernels this comparison leaves untouched (sums-less context);
  (b0) Device.verify_same_message_bits on the context without sums;
  (b1) Device.verify_same_message_bits on the context with sums.
Shapes: 64 groups x 16 sets x 128 keys, 64 x 2 x 440 and
2,048 x 16 x 128; every set is a window of the shuffling (set i starts at
i * keys mod the room left), at participation 100%, 99% and 90%: the clear bits
come from a fixed seed and the signatures are those of the participating keys.
Method as section 3c: every (shape, participation) is warmed up on all paths,
then the paths alternate, REPS times each (host clock around the synchronous
call, staging and PCIe inside), and the comparison runs REPEATS times.  The
yardstick is path (e) of the same run: a bits path is "slower" only if its
median p50 loses to (e)'s by more than the spread of (e)'s p50s.
Per entry: the three p50s of each path, (e)'s spread, the differences, the
bytes each path stages for the keys and in all, and bgv_bits_path_stats of
(b0) and (b1).  Writes profiles/same_message_bits.json.  Needs a HIP device:
there is no CPU fallback.

    python tools/bench_same_message_bits.py [--reps 20] [--repeats 3] [--out profiles/same_message_bits.json]

--one SHAPE PCT PATH runs one warmed-up call of one path (explicit, bits or
bits_sums) and nothing else, for a kernel trace of that call:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_same_message_bits.py --one gossip_aggregates_64x16x128 99 bits
    python tools/c2_timeline.py DIR/.../*_kernel_trace.csv
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
PARTICIPATION = [100, 99, 90]
N_KEYS = 1 << 20
LIST_ID = 0
SEED = 0x534D4253


def make(dev, shuffling, groups, per_group, keys_per_set, pct, seed):
    """(explicit arrays, bits arrays) of one shape at one participation, signed by the device"""
    rng = np.random.default_rng(seed)
    n = groups * per_group
    room = N_KEYS - keys_per_set + 1
    off = (np.arange(n, dtype=np.int64) * keys_per_set) % room
    present = np.ones((n, keys_per_set), bool) if pct == 100 else rng.random((n, keys_per_set)) < pct / 100.0
    present[:, 0] |= ~present.any(axis=1)  # a set is never empty
    bytes_per_set = (keys_per_set + 7) // 8
    bits = np.packbits(present, axis=1, bitorder="little")
    assert bits.shape == (n, bytes_per_set)
    src = np.zeros(n, native.SET_SRC_DTYPE)
    src["list"], src["off"], src["len"] = LIST_ID, off, keys_per_set
    src["bits_off"] = np.arange(n, dtype=np.int64) * bytes_per_set
    window = shuffling[(off[:, None] + np.arange(keys_per_set)[None, :]).reshape(-1)].reshape(n, keys_per_set)
    idx = np.ascontiguousarray(window[present], np.uint32)
    pk_off = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.uint32)
    gmsgs = rng.integers(0, 256, size=(groups, 32), dtype=np.uint8)
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": pk_off,
                  "pk_indices": idx, "msgs": np.ascontiguousarray(np.repeat(gmsgs, per_group, axis=0))}, sigs)
    common = {"n_sets": n, "n_groups": groups, "group_offsets": (np.arange(groups + 1) * per_group).astype(np.uint32),
              "msgs": gmsgs, "sigs": sigs, "sig_len": np.full(n, 96, np.uint32)}
    explicit = dict(common, pk_offsets=pk_off, pk_indices=idx)
    as_bits = dict(common, src=src, bits=np.ascontiguousarray(bits.reshape(-1)), bits_len=int(bits.size),
                   pk_indices=np.zeros(1, np.uint32), n_indices=0)
    return explicit, as_bits


def staged_bytes(explicit, as_bits):
    """what a host batch copies into the staging buffer, per path: the key side and everything"""
    n, G = explicit["n_sets"], explicit["n_groups"]
    rest = 32 * G + 192 * n + 4 * n
    key_e = 4 * (n + 1) + 4 * int(explicit["pk_indices"].size)
    key_b = 16 * n + int(as_bits["bits_len"])
    return {"explicit_keys": key_e, "bits_keys": key_b, "explicit_total": key_e + rest, "bits_total": key_b + rest}


def timed(call, arrays, dev):
    t0 = time.perf_counter()
    ok, _ = call(arrays)
    dt = time.perf_counter() - t0
    assert ok.all() and dev.last_sm_stats.groups_retried == 0
    return dt * 1e3


def trace_one(shape, pct, path):
    name, g, k, m = next(x for x in SHAPES if x[0] == shape)
    pct = int(pct)
    shuffling = np.random.default_rng(SEED).permutation(N_KEYS).astype(np.uint32)
    d = native.Device(0)
    try:
        d.gen_keys(0, N_KEYS, SEED)
        d.index_list_set(LIST_ID, shuffling)
        if path == "bits_sums":
            d.index_list_sums(LIST_ID, True)
        explicit, as_bits = make(d, shuffling, g, k, m, pct, 13 + g * k * m + pct)
        call, arrays = (d.verify_same_message_agg, explicit) if path == "explicit" else (d.verify_same_message_bits, as_bits)
        for _ in range(4):  # three warm-ups, then the call the trace is read for (the last k_batch_final)
            ms = timed(call, arrays, d)
        print(json.dumps({"shape": name, "participation_pct": pct, "path": path, "last_call_ms": ms}))
    finally:
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "same_message_bits.json"))
    ap.add_argument("--one", nargs=3, metavar=("SHAPE", "PCT", "PATH"), help="one warmed-up call of one path, for a kernel trace")
    args = ap.parse_args()
    if args.one:
        return trace_one(*args.one)
    if args.reps < 20 or args.repeats < 3:
        ap.error("at least 20 repetitions per path and 3 repeats of the comparison")
    shuffling = np.random.default_rng(SEED).permutation(N_KEYS).astype(np.uint32)
    d0, d1 = native.Device(0), native.Device(0)  # raises without a device
    try:
        for d in (d0, d1):
            d.gen_keys(0, N_KEYS, SEED)
            d.index_list_set(LIST_ID, shuffling)
        t0 = time.perf_counter()
        d1.index_list_sums(LIST_ID, True)
        out = {"reps": args.reps, "repeats": args.repeats, "clock": "host perf_counter around the synchronous call",
               "table_keys": N_KEYS, "list_entries": int(shuffling.size), "sums_build_host_ms": (time.perf_counter() - t0) * 1e3,
               "sums_build_device_ms": d1.index_list_sums_ms(), "entries": {}}
        paths = (("explicit", d0, d0.verify_same_message_agg), ("bits", d0, d0.verify_same_message_bits),
                 ("bits_sums", d1, d1.verify_same_message_bits))
        for name, g, k, m in SHAPES:
            for pct in PARTICIPATION:
                explicit, as_bits = make(d0, shuffling, g, k, m, pct, 13 + g * k * m + pct)
                data = {"explicit": explicit, "bits": as_bits, "bits_sums": as_bits}
                for _ in range(3):  # warm-up of every path
                    for p, dev, call in paths:
                        timed(call, data[p], dev)
                p50 = {p: [] for p, _, _ in paths}
                for _ in range(args.repeats):
                    t = {p: [] for p, _, _ in paths}
                    for _ in range(args.reps):  # alternating
                        for p, dev, call in paths:
                            t[p].append(timed(call, data[p], dev))
                    for p in t:
                        p50[p].append(float(np.median(t[p])))
                st = d1.last_sm_stats.as_dict()
                spread = max(p50["explicit"]) - min(p50["explicit"])
                med = {p: float(np.median(v)) for p, v in p50.items()}
                res = {"groups": g, "sets_per_group": k, "keys_per_set": m, "participation_pct": pct, "n_sets": g * k,
                       "n_keys": int(explicit["pk_indices"].size), "segments": st["n_segments"], "hashes": st["hashes"],
                       "explicit_p50_ms": p50["explicit"], "bits_p50_ms": p50["bits"], "bits_sums_p50_ms": p50["bits_sums"],
                       "explicit_spread_ms": spread,
                       "bits_minus_explicit_ms": med["bits"] - med["explicit"],
                       "bits_sums_minus_explicit_ms": med["bits_sums"] - med["explicit"],
                       "bits_slower_by_more_than_the_spread": bool(med["bits"] - med["explicit"] > spread),
                       "bits_sums_slower_by_more_than_the_spread": bool(med["bits_sums"] - med["explicit"] > spread),
                       "staged_bytes": staged_bytes(explicit, as_bits),
                       "path_stats_bits": d0.bits_path_stats(), "path_stats_bits_sums": d1.bits_path_stats()}
                out["entries"][f"{name}_p{pct}"] = res
                print(json.dumps({f"{name}_p{pct}": res}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        d0.close()
        d1.close()


if __name__ == "__main__":
    main()
