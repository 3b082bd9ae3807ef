"""Measure sets given as committee bitfields over resident index lists
(bgv_verify_bits) against explicit index lists (bgv_verify), host-resident
batches in both: the staging copy and the PCIe transfer are inside the timed
region, as for a Node caller.

Three shapes, the same signed sets through both paths:
  c4      the C4 segment of bench.build_segment (1,024 blocks, 100,352 sets):
          every 128-key attestation is a window of the shuffling (list 0, all
          bits set, so the keys are exactly the baseline's), every 512-key sync
          aggregate a window of list 1, the two singles per block explicit;
  epoch   its first 32 blocks (3,136 sets);
  gossip  64 sets: 21 aggregate-and-proofs (selection proof and aggregator
          signature as explicit singles, the aggregate as a 128-member committee
          with ~90% participation) and one more single.
The lists are uploaded once per shape, outside the timed region (a node
uploads them once per epoch shuffling / sync-committee period).  Both paths
are warmed up, then alternate in one process, REPS times each (host clock
around the synchronous call); the comparison runs REPEATS times, and the
spread of the p50 across the repeats is reported beside it.  The expansion
kernels' own time comes from HIP events on a second context that records stage
timings (bgv_cfg.timing = 1).  Also reports the host-to-device bytes of each
path.  Writes profiles/bits_expand.json.  Needs a HIP device.

    python tools/bench_bits.py [--reps 9] [--repeats 3] [--out profiles/bits_expand.json]
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
import bench  # noqa: E402
from lodestar_amd import native  # noqa: E402

X = native.SRC_EXPLICIT
L_SHUFFLE, L_SYNC = 0, 1


def segment_as_bits(seg: dict):
    """the sets of a bench.build_segment batch as (list, window, bits) sources: returns (bits arrays, lists)"""
    perm = np.random.default_rng(bench.SEED).permutation(bench.N_VALIDATORS).astype(np.uint32)
    # windows that run over the end of the shuffling in the segment wrap around: the list repeats its head
    shuffle = np.concatenate([perm, perm[: bench.ATT_PER_BLOCK * bench.ATT_K]])
    where = np.empty(bench.N_VALIDATORS, np.int64)
    where[perm] = np.arange(bench.N_VALIDATORS)
    po, idx = seg["pk_offsets"], seg["pk_indices"]
    n = seg["n_sets"]
    src = np.zeros(n, native.SET_SRC_DTYPE)
    bits, sync, explicit = bytearray(), [], []
    n_sync = n_explicit = 0
    for i in range(n):
        keys = idx[po[i]:po[i + 1]]
        k = keys.size
        at = int(where[keys[0]])
        if k == bench.ATT_K and np.array_equal(shuffle[at:at + k], keys):
            src[i] = (L_SHUFFLE, at, k, len(bits))
            bits += b"\xff" * (k // 8)
        elif k == bench.SYNC_K:
            src[i] = (L_SYNC, n_sync, k, len(bits))
            bits += b"\xff" * (k // 8)
            sync.append(keys)
            n_sync += k
        else:
            src[i] = (X, n_explicit, k, 0)
            explicit.append(keys)
            n_explicit += k
    a = {"n_sets": n, "n_jobs": seg["n_jobs"], "job_offsets": seg["job_offsets"], "src": src,
         "bits": np.frombuffer(bytes(bits), np.uint8).copy(), "bits_len": len(bits),
         "pk_indices": np.concatenate(explicit).astype(np.uint32) if explicit else np.zeros(1, np.uint32),
         "n_indices": n_explicit, "msgs": seg["msgs"], "n_raw": 0}
    return a, {L_SHUFFLE: shuffle, L_SYNC: np.concatenate(sync).astype(np.uint32)}


def gossip_batch(seed: int = 64):
    """64 sets in 22 jobs: (explicit arrays, bits arrays, lists)"""
    rng = np.random.default_rng(seed)
    shuffle = rng.permutation(bench.N_VALIDATORS).astype(np.uint32)[: 64 * 2048]  # one slot's committees
    src, bits, explicit, keys, jobs = [], bytearray(), [], [], [0]
    for j in range(22):
        for s in range(3 if j < 21 else 1):
            if s < 2:
                v = int(rng.integers(bench.N_VALIDATORS))
                src.append((X, len(explicit), 1, 0))
                explicit.append(v)
                keys.append(np.array([v], np.uint32))
            else:
                off = 128 * int(rng.integers(0, shuffle.size // 128))
                b = rng.random(128) < 0.9
                src.append((L_SHUFFLE, off, 128, len(bits)))
                bits += np.packbits(b, bitorder="little").tobytes()
                keys.append(shuffle[off:off + 128][b])
        jobs.append(len(src))
    n = len(src)
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    common = {"n_sets": n, "n_jobs": len(jobs) - 1, "job_offsets": np.array(jobs, np.uint32), "msgs": msgs, "n_raw": 0}
    plain = dict(common, pk_offsets=np.concatenate([[0], np.cumsum([k.size for k in keys])]).astype(np.uint32),
                 pk_indices=np.concatenate(keys).astype(np.uint32))
    a = dict(common, src=np.array(src, native.SET_SRC_DTYPE), bits=np.frombuffer(bytes(bits), np.uint8).copy(),
             bits_len=len(bits), pk_indices=np.array(explicit, np.uint32), n_indices=len(explicit))
    return plain, a, {L_SHUFFLE: shuffle}


def h2d_bytes(a: dict) -> int:
    n = a["n_sets"]
    common = n * (32 + 192 + 4) + a["job_offsets"].nbytes
    if "src" in a:
        return int(common + a["src"].nbytes + a["bits_len"] + 4 * a["n_indices"])
    return int(common + a["pk_indices"].nbytes + a["pk_offsets"].nbytes)


def timed(call, arrays):
    t0 = time.perf_counter()
    jr, _ = call(arrays, want_set_codes=False)
    dt = time.perf_counter() - t0
    assert (jr == 1).all()
    return dt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bits_expand.json"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions per path")
    dev = native.Device(0)           # raises without a device
    dev_t = native.Device(0, timing=1)  # per-stage events: the expansion kernels' own time
    try:
        for d in (dev, dev_t):
            d.gen_keys(0, bench.N_VALIDATORS, bench.SEED)
        seg = bench.build_segment(list(range(args.blocks)))
        epoch = bench.build_segment(list(range(32)))
        g_plain, g_bits, g_lists = gossip_batch()
        shapes = [("c4", seg, *segment_as_bits(seg)), ("epoch", epoch, *segment_as_bits(epoch)),
                  ("gossip", g_plain, g_bits, g_lists)]
        out = {"reps": args.reps, "repeats": args.repeats, "clock": "host perf_counter around the synchronous call, host-resident batches",
               "baseline": "bgv_verify with explicit pk_offsets / pk_indices, same process, alternating", "shapes": {}}
        for name, plain, bits, lists in shapes:
            for d in (dev, dev_t):
                for k, v in lists.items():
                    d.index_list_set(k, v)
            # the two batches hold the same keys: the device expansion is the baseline's index list
            off, idx = dev.debug_bits_expand(bits, cap=plain["pk_indices"].size)
            assert np.array_equal(off, plain["pk_offsets"]) and np.array_equal(idx, plain["pk_indices"])
            plain = bench.signed(dev, plain)
            bits = dict(bits, sigs=plain["sigs"], sig_len=plain["sig_len"])
            for _ in range(3):  # warm-up, both paths
                timed(dev.verify, plain)
                timed(dev.verify_bits, bits)
            p50a, p50b = [], []
            for _ in range(args.repeats):
                ta, tb = [], []
                for _ in range(args.reps):  # alternating
                    tb.append(timed(dev.verify, plain))
                    ta.append(timed(dev.verify_bits, bits))
                p50a.append(float(np.median(ta)))
                p50b.append(float(np.median(tb)))
            ex = []
            for _ in range(5):
                timed(dev_t.verify_bits, bits)
                ex.append(dev_t.bits_expand_ms())
            spread_a, spread_b = max(p50a) - min(p50a), max(p50b) - min(p50b)
            diff = float(np.median(p50a) - np.median(p50b))
            res = {"n_sets": int(plain["n_sets"]), "n_jobs": int(plain["n_jobs"]), "n_keys": int(plain["pk_indices"].size),
                   "explicit_p50_ms": [round(x, 3) for x in p50b], "bits_p50_ms": [round(x, 3) for x in p50a],
                   "explicit_spread_ms": round(spread_b, 3), "bits_spread_ms": round(spread_a, 3),
                   "bits_minus_explicit_ms": round(diff, 3),
                   # slower: by more than the baseline's own run-to-run spread; faster: by more than either path's
                   "verdict": ("slower" if diff > spread_b else "faster" if diff < -max(spread_a, spread_b)
                               else "within the run-to-run spread"),
                   "explicit_h2d_bytes": h2d_bytes(plain), "bits_h2d_bytes": h2d_bytes(bits),
                   "expand_kernels_ms": round(float(np.median(ex)), 4), "layout": dev.last_stats.layout()}
            out["shapes"][name] = res
            print(json.dumps({name: res}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        dev.close()
        dev_t.close()


if __name__ == "__main__":
    main()
