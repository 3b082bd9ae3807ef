"""Measure bgv_verify_bits over index lists with resident prefix sums
(bgv_index_list_sums: window sum minus absent members) against the same call
on a context without sums, whose code path is the direct gather.

One process, one device, two contexts that hold the same table and lists: sums
on and sums off.  Host-resident batches, host clock around the synchronous
call (staging and PCIe inside the timed region).  Both contexts are warmed up,
then alternate, REPS times each; the comparison runs REPEATS times and the
spread of the baseline's p50 across the repeats is the yardstick: the sums
path is "slower" only if it loses by more than that spread.

Shapes, the same signed sets through both contexts:
  c4_100 .. c4_50  the C4 segment of bench.build_segment (100,352 sets) as
                   windows of the shuffling / sync-committee lists
                   (tools/bench_bits.py segment_as_bits) at participation
                   100%, 99%, 90%, 60% and 50%: random clear bits from a fixed
                   seed, signatures generated for the participating keys;
  epoch_99         its first 32 blocks (3,136 sets) at 99%;
  gossip           the 64-set gossip batch of tools/bench_bits.py (~90%).
Per shape: keys_expanded / keys_gathered (bgv_bits_path_stats), the p50s of
both paths, the baseline's spread, the difference, and the device time of the
pk_gather and hash_to_g2 stages on both contexts (contexts that record stage
timings; the expansion kernels' time beside them).  Also: the build time of bgv_index_list_sums for a 2^20-entry and a
512-entry list (HIP events, and the host clock around the call), and the C4
99% shape with three batches in flight per path (three contexts per path, one
thread each, dist.run_in_flight) as ms per batch.  --parent names the JSON a
tools/bench_bits.py run of the parent commit wrote on the same box: its C4
bits p50 is recorded beside the sums-off p50.
Writes profiles/bits_sums.json.  Needs a HIP device.

    python tools/bench_bits_sums.py [--reps 9] [--repeats 3] [--parent FILE] [--out profiles/bits_sums.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lodestar_amd import dist, native  # noqa: E402
from tools.bench_bits import L_SHUFFLE, L_SYNC, gossip_batch, segment_as_bits, timed  # noqa: E402

X = native.SRC_EXPLICIT
L_BUILD = 7  # the build-time measurement's own list
DEPTH = 3
ST_HASH_TO_G2, ST_PK_GATHER = 1, 2  # bgv_stage_name(): "hash_to_g2", "pk_gather"


def at_participation(a: dict, lists: dict, p: float | None, seed: int):
    """the bits batch `a` with every list set's bits redrawn at participation p
    (None: kept as they are); returns (bits arrays, the explicit batch of the
    participating keys).  Every list set's length is a multiple of 8."""
    src = a["src"]
    n = a["n_sets"]
    lens = src["len"].astype(np.int64)
    is_list = src["list"] != X
    assert not (lens[is_list] % 8).any()
    starts = np.concatenate([[0], np.cumsum(lens)])
    total = int(starts[-1])
    set_id = np.repeat(np.arange(n), lens)
    j = np.arange(total) - starts[set_id]
    at = src["off"].astype(np.int64)[set_id] + j
    cand = np.empty(total, np.uint32)
    sel = ~is_list[set_id]
    cand[sel] = a["pk_indices"][at[sel]]
    for lid, lst in lists.items():
        sel = src["list"][set_id] == lid
        cand[sel] = lst[at[sel]]
    member = is_list[set_id]
    mask = np.ones(total, bool)
    if p is None:
        old = np.unpackbits(a["bits"], bitorder="little")
        mask[member] = old[(8 * src["bits_off"].astype(np.int64))[set_id][member] + j[member]].astype(bool)
    elif p < 1.0:
        mask[member] = np.random.default_rng(seed).random(int(member.sum())) < p
    counts = np.add.reduceat(mask, starts[:-1])
    for i in np.flatnonzero(counts == 0):  # a set keeps at least one key
        mask[starts[i]] = True
        counts[i] = 1
    new_src = src.copy()
    new_src["bits_off"][is_list] = (np.concatenate([[0], np.cumsum(lens[is_list] // 8)])[:-1]).astype(np.uint32)
    bits = np.packbits(mask[member], bitorder="little")
    out = dict(a, src=new_src, bits=bits, bits_len=int(bits.size))
    plain = {"n_sets": n, "n_jobs": a["n_jobs"], "job_offsets": a["job_offsets"], "msgs": a["msgs"], "n_raw": 0,
             "pk_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), "pk_indices": cand[mask]}
    return out, plain


def stage_ms(d, bits, reps=5):
    g, h, e = [], [], []
    for _ in range(reps):
        timed(d.verify_bits, bits)
        s = d.last_stats.stage_ms
        g.append(float(s[ST_PK_GATHER]))
        h.append(float(s[ST_HASH_TO_G2]))
        e.append(d.bits_expand_ms())
    return round(float(np.median(g)), 4), round(float(np.median(h)), 4), round(float(np.median(e)), 4)


def in_flight_ms(ctxs, bits, steps=9):
    """ms per batch with len(ctxs) batches in flight, one worker thread per context"""
    pool = ThreadPoolExecutor(len(ctxs))
    try:
        def submit(k):
            return pool.submit(ctxs[k % len(ctxs)].verify_bits, bits, want_set_codes=False)

        def finish(k, res):
            return bool((res[0] == 1).all())

        assert dist.run_in_flight(submit, finish, len(ctxs), len(ctxs))  # warm-up
        t0 = time.perf_counter()
        assert dist.run_in_flight(submit, finish, steps, len(ctxs))
        return (time.perf_counter() - t0) * 1e3 / steps
    finally:
        pool.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--parent", default=None, help="JSON of the parent commit's tools/bench_bits.py run on the same box")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bits_sums.json"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions per path")
    on = [native.Device(0) for _ in range(DEPTH)]   # raises without a device
    off = [native.Device(0) for _ in range(DEPTH)]
    t_on, t_off = native.Device(0, timing=1), native.Device(0, timing=1)  # per-stage events at every size
    every = on + off + [t_on, t_off]
    with_sums = on + [t_on]
    try:
        for d in every:
            d.gen_keys(0, bench.N_VALIDATORS, bench.SEED)
        out = {"reps": args.reps, "repeats": args.repeats,
               "clock": "host perf_counter around the synchronous call, host-resident batches",
               "baseline": "bgv_verify_bits on a context without sums (the direct gather), same process, alternating",
               "stored_form": "Jacobian, 144 B per entry", "shapes": {}}

        def install(lists):
            for d in every:
                for k, v in lists.items():
                    d.index_list_set(k, v)
            for d in with_sums:
                for k in lists:
                    d.index_list_sums(k, True)

        # ---- build time of the sums
        build = {}
        perm = np.random.default_rng(bench.SEED).permutation(bench.N_VALIDATORS).astype(np.uint32)
        for name, lst in (("list_2^20", perm), ("list_512", perm[:512])):
            on[0].index_list_set(L_BUILD, lst)
            dev_ms, host_ms = [], []
            for _ in range(4):
                t0 = time.perf_counter()
                on[0].index_list_sums(L_BUILD, True)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                dev_ms.append(on[0].index_list_sums_ms())
            build[name] = {"entries": int(lst.size), "device_ms_hip_events": round(float(np.median(dev_ms[1:])), 3),
                           "host_call_ms": round(float(np.median(host_ms[1:])), 3), "bytes": (int(lst.size) + 1) * 144}
        on[0].index_list_set(L_BUILD, np.zeros(0, np.uint32))
        out["sums_build"] = build
        print(json.dumps({"sums_build": build}), flush=True)

        seg = bench.build_segment(list(range(args.blocks)))
        epoch = bench.build_segment(list(range(32)))
        seg_bits, seg_lists = segment_as_bits(seg)
        ep_bits, ep_lists = segment_as_bits(epoch)
        _, g_bits, g_lists = gossip_batch()
        shapes = [(f"c4_{pct}", seg_bits, seg_lists, pct / 100.0) for pct in (100, 99, 90, 60, 50)]
        shapes += [("epoch_99", ep_bits, ep_lists, 0.99), ("gossip", g_bits, g_lists, None)]
        installed = None
        for name, base, lists, p in shapes:
            if installed is not lists:
                install(lists)
                installed = lists
            bits, plain = at_participation(base, lists, p, seed=bench.SEED + int(1000 * (p or 0)))
            plain = bench.signed(on[0], plain)
            bits = dict(bits, sigs=plain["sigs"], sig_len=plain["sig_len"])
            d_on, d_off = on[0], off[0]
            for _ in range(3):  # warm-up, both paths
                timed(d_off.verify_bits, bits)
                timed(d_on.verify_bits, bits)
            path_on, path_off = d_on.bits_path_stats(), d_off.bits_path_stats()
            p50_on, p50_off = [], []
            for _ in range(args.repeats):
                ta, tb = [], []
                for _ in range(args.reps):  # alternating
                    tb.append(timed(d_off.verify_bits, bits))
                    ta.append(timed(d_on.verify_bits, bits))
                p50_on.append(float(np.median(ta)))
                p50_off.append(float(np.median(tb)))
            gather_on, hash_on, expand_on = stage_ms(t_on, bits)
            gather_off, hash_off, expand_off = stage_ms(t_off, bits)
            spread_on, spread_off = max(p50_on) - min(p50_on), max(p50_off) - min(p50_off)
            diff = float(np.median(p50_on) - np.median(p50_off))
            res = {"n_sets": int(bits["n_sets"]), "participation": p if p is not None else "as built (~0.9)",
                   "sets_complement": path_on["sets_complement"], "keys_expanded": path_on["keys_expanded"],
                   "keys_gathered": path_on["keys_gathered"], "keys_gathered_sums_off": path_off["keys_gathered"],
                   "gathered_over_expanded": round(path_on["keys_gathered"] / max(path_on["keys_expanded"], 1), 5),
                   "sums_p50_ms": [round(x, 3) for x in p50_on], "no_sums_p50_ms": [round(x, 3) for x in p50_off],
                   "sums_spread_ms": round(spread_on, 3), "no_sums_spread_ms": round(spread_off, 3),
                   "sums_minus_no_sums_ms": round(diff, 3),
                   # slower: by more than the baseline's own run-to-run spread; faster: by more than either path's
                   "verdict": ("slower" if diff > spread_off else "faster" if diff < -max(spread_on, spread_off)
                               else "within the run-to-run spread"),
                   "stage_ms": {"pk_gather": {"sums": gather_on, "no_sums": gather_off},
                                "hash_to_g2": {"sums": hash_on, "no_sums": hash_off},
                                "expansion_kernels": {"sums": expand_on, "no_sums": expand_off}},
                   "layout": d_on.last_stats.layout()}
            if name == "c4_99":
                fl_on, fl_off = [], []
                for _ in range(args.repeats):  # alternating
                    fl_off.append(in_flight_ms(off, bits))
                    fl_on.append(in_flight_ms(on, bits))
                res["three_in_flight_ms_per_batch"] = {"sums": [round(x, 3) for x in fl_on], "no_sums": [round(x, 3) for x in fl_off]}
            if name == "c4_100" and args.parent:
                with open(args.parent) as f:
                    par = json.load(f)["shapes"]["c4"]
                lo, hi = min(par["bits_p50_ms"]), max(par["bits_p50_ms"])
                mine = float(np.median(p50_off))
                res["parent_bench_bits_c4"] = {"bits_p50_ms": par["bits_p50_ms"], "bits_spread_ms": par["bits_spread_ms"],
                                               "no_sums_p50_ms_here": round(mine, 3),
                                               "no_sums_minus_parent_ms": round(mine - float(np.median(par["bits_p50_ms"])), 3),
                                               "within_parent_spread": bool(lo - par["bits_spread_ms"] <= mine <= hi + par["bits_spread_ms"])}
            out["shapes"][name] = res
            print(json.dumps({name: res}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        for d in every:
            d.close()


if __name__ == "__main__":
    main()
