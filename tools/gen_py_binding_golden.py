"""Generate tests/golden/py_binding.json: what the public functions of the Python
binding (lodestar_amd/verifier.py, lodestar_amd/native.py) make of a seeded corpus.

The file pins the binding's host side: per encoder result the keys in order and a
SHA-256 digest of every entry (dtype, shape, contiguity and bytes of an array; type
and value of a scalar), per make_*_batch struct every non-pointer field and for every
pointer field whether it is NULL or which entry of `arrays` it addresses, every
refusal with its type, text and code, and for the run_* functions against a stand-in
device the arguments the device saw, the per-call results and the metrics dict.
tests/test_py_binding_golden.py replays record() and compares it with the file.

Needs neither the library nor a GPU.  Rerun it only when the binding's behaviour is
meant to change:

    python tools/gen_py_binding_golden.py
"""
import asyncio
import ctypes
import hashlib
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lodestar_amd import native  # noqa: E402
from lodestar_amd import verifier as V  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "py_binding.json")
SEED = 0x5EED0B1D


def digest(v) -> str:
    h = hashlib.sha256()
    if isinstance(v, np.ndarray):
        h.update(f"ndarray|{v.dtype.descr!r}|{v.shape!r}|{bool(v.flags['C_CONTIGUOUS'])}|".encode())
        h.update(v.tobytes())
    else:
        h.update(f"{type(v).__name__}|{v!r}".encode())
    return h.hexdigest()


def dict_record(d: dict) -> dict:
    return {"keys": list(d), "sha256": {k: digest(v) for k, v in d.items()}}


def dict_digest(d: dict) -> str:
    """one digest over dict_record(d): the keys in order and every entry"""
    return hashlib.sha256(json.dumps(dict_record(d)).encode()).hexdigest()


def attempt(fn, *args, **kw):
    """fn's outcome: {"ok": what it returned} or the exception's type, text and code"""
    try:
        return {"ok": fn(*args, **kw)}
    except (V.BlsError, V.QueueError, KeyError) as e:
        return {"raises": type(e).__name__, "text": str(e), "code": getattr(e, "code", None)}
    except Exception as e:  # noqa: BLE001 -- an interpreter's or numpy's own error: its wording is theirs, the type is pinned
        return {"raises": type(e).__name__}


def encode_record(fn, items, scalars, whole: bool = False) -> dict:
    """whole: one digest over the result instead of one per entry"""
    r = attempt(fn, items, scalars)
    if "ok" in r:
        a = r["ok"]
        r = {"dict_sha256": dict_digest(a)} if whole else dict_record(a)
        r["scalars_is_input"] = a["scalars"] is scalars
    return r


# ------------------------------------------------------------------ corpus
class Corpus:
    def __init__(self):
        self.rng = np.random.default_rng(SEED)
        self.raw_a, self.raw_b = self.blob(96), self.blob(96)

    def blob(self, n: int) -> bytes:
        return self.rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    def single(self, pk, sig_len=96, root_len=32):
        return V.create_single_signature_set_from_components(pk, self.blob(root_len), self.blob(sig_len))

    def aggregate(self, pks, sig_len=96, root_len=32):
        return V.create_aggregate_signature_set_from_components(pks, self.blob(root_len), self.blob(sig_len))

    def committee(self, ref, bits, sig_len=96, root_len=32):
        return V.create_committee_signature_set_from_components(ref, bits, self.blob(root_len), self.blob(sig_len))

    def jobs(self) -> dict:
        A, B, I = V.PublicKey(raw=self.raw_a), V.PublicKey(raw=self.raw_b), lambda i: V.PublicKey(index=i)
        plain0 = [self.single(I(5)), self.aggregate([I(1), I(2), A, I(3)], 192), self.single(A, 7)]
        plain1 = [self.aggregate([A, B, I(9)], 0), self.single(I(7))]
        com13 = self.committee(V.CommitteeRef(1, 3, 13), bytes([0b10110101, 0b00010010]))
        com5 = self.committee(V.CommitteeRef(0, 0, 5), bytes([0b00010011]), 192)
        return {
            "explicit_raw_key_three_times": [plain0, plain1],
            "mixed_with_committee_sets": [[plain0[0], com13, plain0[1], plain0[2]], [com5, plain1[0], com13, plain1[1]]],
            "empty_job_list": [],
            "empty_job_between_full_ones": [plain0, [], plain1],
            "index_keys_only": [[self.single(I(0x7FFFFFFF)), self.aggregate([I(0), I(4)])]],
        }

    def key_forms(self, k: int, n_keys: int):
        """the three ways a set of an aggregate group names its keys, in turn"""
        idx = [(17 * k + 3 * j) % 1000 for j in range(n_keys)]
        if k % 3 == 0:
            pks = [V.PublicKey(index=i) for i in idx]
            if k % 2 == 0:
                pks[len(pks) // 2] = V.PublicKey(raw=self.raw_a if k % 4 == 0 else self.raw_b)
            return pks
        return idx if k % 3 == 1 else np.array(idx, dtype=np.int64 if k % 2 else np.uint32)

    def single_groups(self, sizes):
        out, k = [], 0
        for size in sizes:
            sets = []
            for _ in range(size):
                pk = V.PublicKey(raw=self.raw_b if k % 10 == 0 else self.raw_a) if k % 5 == 0 else V.PublicKey(index=k * 7)
                sets.append((pk, self.blob((96, 192, 7, 0)[k % 4] if k % 9 == 0 else 96)))
                k += 1
            out.append((self.blob(32), sets))
        return out

    def agg_groups(self, sizes, committees: bool):
        out, k = [], 0
        for size in sizes:
            sets = []
            for _ in range(size):
                if committees and k % 2 == 0:
                    # lengths 5 and 13 first: the second bitfield starts at byte 1, the third at byte 3
                    length = (5, 13, 64, 9)[(k // 2) % 4]
                    bits = bytearray(self.blob((length + 7) // 8))
                    bits[0] |= 1
                    keys = V.CommitteeKeys(V.CommitteeRef((k // 2) % 3, k, length), bytes(bits))
                else:
                    keys = self.key_forms(k - 1 if committees else k, 1 + k % 4)
                sets.append((keys, self.blob((96, 192, 7, 0)[k % 4] if k % 9 == 0 else 96)))
                k += 1
            out.append((self.blob(32), sets))
        return out


# the cases recorded entry by entry; every other result is pinned by one digest over all its entries
PER_ENTRY = ("mixed_with_committee_sets", "groups_1_64_65")


def record_encoders(c: Corpus) -> dict:
    out = {}
    for name, jobs in c.jobs().items():
        n = sum(len(j) for j in jobs)
        for label, sc in (("scalars", np.arange(1, max(n, 1) + 1, dtype=np.uint64)), ("no_scalars", None)):
            whole = sc is None or name not in PER_ENTRY
            out[f"encode_jobs/{name}/{label}"] = encode_record(V.encode_jobs, jobs, sc, whole)
            out[f"encode_jobs_bits/{name}/{label}"] = encode_record(V.encode_jobs_bits, jobs, sc, whole)
        r = attempt(V.encode_device_batch, jobs, None)  # equals the no_scalars record of the encoder it chose
        out[f"encode_device_batch/{name}"] = ({"use_bits": r["ok"][0], "dict_sha256": dict_digest(r["ok"][1])} if "ok" in r else r)
    for shape, sizes in (("one_group_one_set", [1]), ("groups_1_64_65", [1, 64, 65]), ("no_group", [])):
        n = sum(sizes)
        sc = np.arange(3, max(n, 1) + 3, dtype=np.uint64)
        whole = shape not in PER_ENTRY
        out[f"encode_same_message/{shape}"] = encode_record(V.encode_same_message, c.single_groups(sizes), sc, whole)
        out[f"encode_same_message_agg/{shape}"] = encode_record(V.encode_same_message_agg, c.agg_groups(sizes, False), sc, whole)
        out[f"encode_same_message_bits/{shape}"] = encode_record(V.encode_same_message_bits, c.agg_groups(sizes, True), None,
                                                                 whole)
        out[f"encode_same_message_bits/{shape}/explicit_only"] = encode_record(V.encode_same_message_bits,
                                                                               c.agg_groups(sizes, False), sc, True)
    return out


# ------------------------------------------------------------------ merging
def result_record(r):
    if isinstance(r, V.SameMessageAggregate):
        return {"valid": [bool(x) for x in r.valid], "aggregate": bytes(r.aggregate).hex(), "count": int(r.count)}
    if isinstance(r, Exception):
        return {"error": type(r).__name__, "text": str(r), "code": getattr(r, "code", None)}
    return r


def six_calls(c: Corpus):
    """six calls: calls 0 and 3 share a message, calls 1 and 4 share another; call 2 carries an AggregateRequest
    whose take has a false entry, call 5 one with a previous (and call 1's message, yet forms its own group)"""
    m0, m1, m2 = c.blob(32), c.blob(32), c.blob(32)
    g = c.single_groups([3, 2, 4, 1, 2, 3])
    return [(g[0][1], m0), (g[1][1], m1), (g[2][1], m2, V.AggregateRequest(None, (True, False, True, True))),
            (g[3][1], bytearray(m0)), (g[4][1], m1, None), (g[5][1], m1, V.AggregateRequest(c.blob(96), None))]


def record_merging(c: Corpus) -> dict:
    calls = six_calls(c)
    groups, where, group_of = V.merge_same_message_groups(calls)
    g2, w2 = V.merge_same_message(calls)
    return {
        "where": [[w.start, w.stop] for w in where], "group_of": group_of,
        "group_sizes": [len(s) for _m, s in groups], "group_messages": [digest(m) for m, _s in groups],
        "encoded": dict_digest(V.encode_same_message(groups)),
        "merge_same_message_agrees": digest(repr((g2, w2))) == digest(repr((groups, where))),
    }


# ------------------------------------------------------------------ refusals
def record_refusals(c: Corpus) -> dict:
    I = lambda i: V.PublicKey(index=i)  # noqa: E731
    raw48 = V.PublicKey(raw=bytes(48))
    ref = V.CommitteeRef(0, 0, 9)
    sig = b"\xaa" * 96
    M, M31 = bytes(32), bytes(31)
    short, good = V.CommitteeKeys(ref, b"\x01"), V.CommitteeKeys(ref, b"\x01\x01")
    job_sets = {
        "empty_aggregate": c.aggregate([]),
        "raw_compressed_key": c.single(raw48),
        "root_31_bytes": c.single(I(1), root_len=31),
        "empty_aggregate_and_root_31_bytes": c.aggregate([], root_len=31),
        "single_without_key": V.ISignatureSet(V.SignatureSetType.single, M, sig),
        "key_none_in_aggregate": c.aggregate([I(1), None]),
        "index_negative": c.single(I(-1)),
        "index_2_31": c.aggregate([I(0), I(0x80000000)]),
        "committee_short_bitfield": c.committee(ref, b"\x01"),
        "committee_short_bitfield_and_root_31_bytes": c.committee(ref, b"\x01", root_len=31),
        "committee_long_bitfield": c.committee(V.CommitteeRef(0, 0, 8), b"\x01\x00"),
        "committee_no_such_list": c.committee(V.CommitteeRef(native.MAX_INDEX_LISTS, 0, 8), b"\x01"),
        "committee_negative_list": c.committee(V.CommitteeRef(-1, 0, 8), b"\x01"),
        "committee_negative_offset": c.committee(V.CommitteeRef(0, -1, 8), b"\x01"),
        "committee_negative_length": c.committee(V.CommitteeRef(0, 0, -8), b""),
        "committee_window_past_2_32": c.committee(V.CommitteeRef(0, 0xFFFFFFFF, 8), b"\x01"),
        "committee_nobody_signed": c.committee(V.CommitteeRef(0, 0, 16), b"\x00\x00"),
        "committee_root_31_bytes": c.committee(ref, b"\x01\x01", root_len=31),
        "committee_missing": V.ISignatureSet(V.SignatureSetType.committee, M, sig, bits=b"\x01"),
        "committee_bits_missing": V.ISignatureSet(V.SignatureSetType.committee, M, sig, committee=ref),
    }
    out = {}
    ok_set = c.single(I(2))
    for name, s in job_sets.items():
        out[f"check_sets/{name}"] = attempt(V.check_sets, [ok_set, s])
        out[f"encode_jobs/{name}"] = attempt(V.encode_jobs, [[ok_set], [s]])
        out[f"encode_jobs_bits/{name}"] = attempt(V.encode_jobs_bits, [[ok_set], [s]])
    single = {
        "message_31_bytes": ([(I(1), sig)], M31),
        "key_none": ([(I(1), sig), (None, sig)], M),
        "raw_compressed_key": ([(raw48, sig)], M),
        "index_negative": ([(I(-5), sig)], M),
        "index_2_31": ([(I(0x80000000), sig)], M),
        "key_none_and_message_31_bytes": ([(None, sig)], M31),
    }
    for name, (sets, m) in single.items():
        out[f"check_same_message/{name}"] = attempt(V.check_same_message, sets, m)
    agg_sets = {
        "message_31_bytes": ([([1], sig)], M31),
        "keys_none": ([(None, sig)], M),
        "keys_empty": ([([1], sig), ([], sig)], M),
        "key_none": ([([1, None], sig)], M),
        "raw_compressed_key": ([([I(1), raw48], sig)], M),
        "index_negative": ([(np.array([3, -1]), sig)], M),
        "index_2_31": ([([0x80000000], sig)], M),
        "committee_short_bitfield": ([(good, sig), (short, sig)], M),
        "committee_long_bitfield": ([(V.CommitteeKeys(V.CommitteeRef(0, 0, 8), b"\x01\x00"), sig)], M),
        "committee_no_such_list": ([(V.CommitteeKeys(V.CommitteeRef(8, 0, 8), b"\x01"), sig)], M),
        "committee_negative_offset": ([(V.CommitteeKeys(V.CommitteeRef(0, -1, 8), b"\x01"), sig)], M),
        "committee_window_past_2_32": ([(V.CommitteeKeys(V.CommitteeRef(0, 0xFFFFFFFF, 8), b"\x01"), sig)], M),
        "committee_nobody_signed": ([(V.CommitteeKeys(V.CommitteeRef(0, 0, 16), b"\x00\x00"), sig)], M),
        "committee_missing": ([(V.CommitteeKeys(None, b"\x01"), sig)], M),
        "committee_bits_missing": ([(V.CommitteeKeys(ref, None), sig)], M),
        "short_bitfield_then_empty_explicit_set": ([(short, sig), ([], sig)], M),
        "empty_explicit_set_then_short_bitfield": ([([], sig), (short, sig)], M),
    }
    for name, (sets, m) in agg_sets.items():
        out[f"check_aggregate_same_message/{name}"] = attempt(V.check_aggregate_same_message, sets, m)
    groups = {
        "empty_group": [(M, [(I(1), sig)]), (M, [])],
        "message_31_bytes": [(M31, [(I(1), sig)])],
        "empty_group_and_message_31_bytes": [(M31, [])],
        "raw_compressed_key": [(M, [(raw48, sig)])],
    }
    for name, g in groups.items():
        out[f"encode_same_message/{name}"] = attempt(V.encode_same_message, g)
        as_lists = [(m, [([pk], s) for pk, s in sets]) for m, sets in g]
        out[f"encode_same_message_agg/{name}"] = attempt(V.encode_same_message_agg, as_lists)
        out[f"encode_same_message_bits/{name}"] = attempt(V.encode_same_message_bits, as_lists)
    for fn in (V.encode_same_message_agg, V.encode_same_message_bits):
        out[f"{fn.__name__}/keys_empty"] = attempt(fn, [(M, [([1], sig), ([], sig)])])
        out[f"{fn.__name__}/keys_empty_and_message_31_bytes"] = attempt(fn, [(M31, [([], sig)])])
    bits = {
        "committee_short_bitfield": [(M, [(good, sig), (short, sig)])],
        "short_bitfield_then_empty_explicit_set": [(M, [(short, sig), ([], sig)])],
        "empty_explicit_set_then_short_bitfield": [(M, [([], sig), (short, sig)])],
    }
    for name, g in bits.items():
        out[f"encode_same_message_bits/{name}"] = attempt(V.encode_same_message_bits, g)
    requests = {
        "previous_95_bytes": ([(I(1), sig)], V.AggregateRequest(bytes(95), None)),
        "take_one_short": ([(I(1), sig), (I(2), sig)], V.AggregateRequest(None, (True,))),
        "previous_95_bytes_and_take_one_short": ([(I(1), sig)], V.AggregateRequest(bytes(95), ())),
    }
    for name, (sets, agg) in requests.items():
        out[f"check_aggregate_request/{name}"] = attempt(V.check_aggregate_request, sets, agg)
    out["PublicKey.from_bytes/47_bytes"] = attempt(V.PublicKey.from_bytes, bytes(47))
    for code in (1, 8, 9, 10, 99):
        e = V.error_for_code(code)
        out[f"error_for_code/{code}"] = {"text": str(e), "code": e.code}
    for r in out.values():  # a check that passes returns None
        if "ok" in r:
            r["ok"] = None if r["ok"] is None else "returned"
    return out


# ------------------------------------------------------------------ structs
def struct_record(b, arrays: dict) -> dict:
    where = {native._ptr(v): k for k, v in arrays.items() if isinstance(v, np.ndarray)}
    out = {"struct": type(b).__name__}
    for name, ctype in b._fields_:
        v = getattr(b, name)
        if ctype is ctypes.c_void_p:
            out[name] = "NULL" if v is None else "arrays[%s]" % where.get(v, "?")
        else:
            out[name] = int(v)
    return out


def record_structs(c: Corpus) -> dict:
    jobs = c.jobs()
    sc = np.arange(1, 200, dtype=np.uint64)
    makers = {
        "Device.make_batch": (native.Device.make_batch, V.encode_jobs(jobs["explicit_raw_key_three_times"], sc)),
        "Device.make_sm_batch": (native.Device.make_sm_batch, V.encode_same_message(c.single_groups([1, 6]), sc)),
        "Device.make_sma_batch": (native.Device.make_sma_batch, V.encode_same_message_agg(c.agg_groups([2, 5], False), sc)),
        "make_bits_batch": (native.make_bits_batch, V.encode_jobs_bits(jobs["mixed_with_committee_sets"], sc)),
        "make_smb_batch": (native.make_smb_batch, V.encode_same_message_bits(c.agg_groups([2, 5], True), sc)),
    }
    out = {
        "Device.make_bits_batch is make_bits_batch": native.Device.make_bits_batch is native.make_bits_batch,
        "Device.make_smb_batch is make_smb_batch": native.Device.make_smb_batch is native.make_smb_batch,
    }
    for name, (make, arrays) in makers.items():
        full = out[f"{name}/full"] = struct_record(make(arrays), arrays)
        out[f"{name}/on_device"] = struct_record(make(arrays, True), arrays)
        out[f"{name}/on_device_unsynced"] = struct_record(make(arrays, on_device=True, sync_inputs=False), arrays)
        no_raw = {**arrays, "raw_pks": None, "n_raw": 0, "scalars": None}
        out[f"{name}/no_raw_no_scalars"] = struct_record(make(no_raw), no_raw)
        for k in arrays:  # a required key is one whose absence raises
            less = {q: v for q, v in arrays.items() if q != k}
            r = attempt(make, less)
            if "ok" in r:  # the fields that differ from the full struct's
                r = {"fields_changed": {f: v for f, v in struct_record(r["ok"], less).items() if v != full[f]}}
            out[f"{name}/without_{k}"] = r
        counts = {q: v for q, v in arrays.items() if q not in ("bits_len", "n_indices", "n_raw")}
        out[f"{name}/without_counts"] = struct_record(make(counts), counts)
    return out


# ------------------------------------------------------------------ runners
class StandInDevice:
    """records what the run_* functions hand to the device and answers by rule: set i is valid unless i % 3 == 2"""

    def __init__(self, stats: bool):
        self.calls = []
        if stats:
            self.last_sm_stats = native.BgvSmStats()
            self.last_sm_stats.groups_retried = 2
            self.sm_retry_stats = lambda: {"mode": 1, "segments": 1, "subs": 4, "subs_failed": 2, "leaves": 9, "pairs": 13,
                                           "hashes": 2}

    def _note(self, name, arrays, **kw):
        self.calls.append({"call": name, "arrays": dict_digest(arrays), **{k: digest(v) for k, v in kw.items()}})
        n = arrays["n_sets"]
        return np.arange(n) % 3 != 2, np.zeros(n, np.int32)

    def verify_same_message(self, arrays, **kw):
        return self._note("verify_same_message", arrays, **kw)

    def verify_same_message_agg(self, arrays, **kw):
        return self._note("verify_same_message_agg", arrays, **kw)

    def verify_same_message_bits(self, arrays, **kw):
        return self._note("verify_same_message_bits", arrays, **kw)

    def bits_path_stats(self):
        self.calls.append({"call": "bits_path_stats"})
        return {"sets_complement": 2, "keys_expanded": 777, "keys_gathered": 3}

    def verify_same_message_aggregate(self, arrays, take=None, prev=None, **kw):
        ok, sc = self._note("verify_same_message_aggregate", arrays, take=take, prev=prev, **kw)
        G = arrays["n_groups"]
        code = np.zeros(G, np.int32)
        if G > 1:
            code[-1] = 1  # the last group's `previous` does not decode
        sig = (np.arange(G * 96) % 251).astype(np.uint8).reshape(G, 96)
        return {"set_valid": ok, "set_code": sc, "agg_sig": sig, "agg_count": np.arange(G, dtype=np.uint32) + 1, "agg_code": code}


def agg_calls(c: Corpus, committees: bool):
    m0, m1 = c.blob(32), c.blob(32)
    g = c.agg_groups([3, 2, 4], committees)
    return [(g[0][1], m0), (g[1][1], m1), (g[2][1], m0)]


def record_runners(c: Corpus) -> dict:
    out = {}
    plain = [call[:2] for call in six_calls(c)]
    cases = {
        "run_same_message_calls/plain": (V.run_same_message_calls, plain),
        "run_same_message_calls/with_aggregate_requests": (V.run_same_message_calls, six_calls(c)),
        "run_same_message_aggregate_calls": (V.run_same_message_aggregate_calls, six_calls(c)),
        "run_same_message_aggregate_calls/no_request": (V.run_same_message_aggregate_calls, plain),
        "run_same_message_agg_calls/explicit": (V.run_same_message_agg_calls, agg_calls(c, False)),
        "run_same_message_agg_calls/committees": (V.run_same_message_agg_calls, agg_calls(c, True)),
    }
    for name, (run, calls) in cases.items():
        for stats in (True, False):
            for label, metrics in (("fresh_metrics", {}), ("running_metrics", V._new_metrics()), ("no_metrics", None)):
                if metrics:
                    metrics.update(same_message_sets_started=100, same_message_agg_retries=7, aggregated_pubkeys_total=1000,
                                   sm_retry_pairs=5)
                dev = StandInDevice(stats)
                seen = []
                res = run(dev, calls, (lambda n: seen.append(n) or np.arange(n, dtype=np.uint64) + 9) if stats else None, metrics)
                out[f"{name}/{'device_with_stats' if stats else 'device_without_stats'}/{label}"] = {
                    "device_calls": dev.calls if label == "fresh_metrics" else digest(json.dumps(dev.calls)),
                    "scalars_asked": seen, "results": [result_record(r) for r in res],
                    "metrics": metrics}
    return out


# ---------------------------------------------------------------- verifiers
def _pool(devices, idle):
    pool = object.__new__(V.BlsGpuVerifier)
    pool.devices = devices
    pool._ctx_dev, pool.n_devices, pool.prio_reserved = list(range(len(devices))), len(devices), False
    pool._dev_locks, pool._idle = [threading.Lock() for _ in devices], list(idle)
    pool.metrics, pool._rng, pool._closed = V._new_metrics(), None, False
    pool._sm = V.SameMessageQueue(pool._run_same_message)
    pool._sma = V.SameMessageQueue(pool._run_same_message_agg)
    return pool


def _pool_metrics(pool) -> dict:
    m = dict(pool.metrics)
    t = m.pop("device_time_s")
    m["device_time_s is a float >= 0"] = isinstance(t, float) and t >= 0
    return m


def record_verifiers(c: Corpus) -> dict:
    """the bulk-context choice of the pool's two same-message runners and the AggregateRequest prelude of both
    verify_and_aggregate_same_message methods, on verifiers built around stand-in devices"""
    out = {}
    sets = c.single_groups([4])[0][1]
    m = c.blob(32)
    for name, idle in (("all_idle", [True, True]), ("second_idle", [False, True]), ("none_idle", [False, False])):
        for runner in ("_run_same_message", "_run_same_message_agg"):
            pool = _pool([StandInDevice(True), StandInDevice(True)], idle)
            calls = [(sets, m)] if runner == "_run_same_message" else agg_calls(c, True)
            res = getattr(pool, runner)(calls)
            out[f"pool.{runner}/{name}"] = {"results": [result_record(r) for r in res], "metrics": _pool_metrics(pool),
                                            "calls_per_device": [[x["call"] for x in d.calls] for d in pool.devices]}

    def single_thread(closed):
        st = object.__new__(V.BlsGpuSingleThreadVerifier)
        st.device, st._closed, st.metrics = StandInDevice(True), closed, {}
        return st

    def aggregate(v, sets, m, **kw):
        r = attempt(lambda: asyncio.run(v.verify_and_aggregate_same_message(sets, m, **kw)))
        return {"result": result_record(r["ok"])} if "ok" in r else r

    prev = c.blob(96)
    for kind, make in (("pool", lambda closed: _pool([StandInDevice(True)], [True])),
                       ("single_thread", single_thread)):
        for closed in (False, True):
            v = make(closed)
            v._closed = closed
            if kind == "pool" and closed:
                v._sm.abort()
            tag = f"{kind}.verify_and_aggregate_same_message/{'closed' if closed else 'open'}"
            out[f"{tag}/take_and_previous"] = aggregate(v, sets[:3], m, previous=bytearray(prev), take=[1, 0, "x"])
            out[f"{tag}/no_sets"] = aggregate(v, [], m)
            out[f"{tag}/no_sets_with_previous"] = aggregate(v, iter(()), m, previous=prev)
            out[f"{tag}/no_sets_previous_95_bytes"] = aggregate(v, [], m, previous=prev[:95])
            out[f"{tag}/take_one_short"] = aggregate(v, sets, m, take=[True])
            out[f"{tag}/message_31_bytes"] = aggregate(v, sets, m[:31])
            dev = v.devices[0] if kind == "pool" else v.device
            out[f"{tag}/device_calls"] = dev.calls
    return out


def record() -> dict:
    c = Corpus()
    return {
        "generator": "tools/gen_py_binding_golden.py",
        "encoders": record_encoders(c),
        "merging": record_merging(c),
        "refusals": record_refusals(c),
        "structs": record_structs(c),
        "runners": record_runners(c),
        "verifiers": record_verifiers(c),
    }


def dumps(rec: dict) -> str:
    """one line per case, so that a regenerated file diffs by case"""
    def line(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))

    parts = []
    for section in sorted(rec):
        v = rec[section]
        if isinstance(v, dict):
            v = "{\n" + ",\n".join(f"{line(k)}:{line(v[k])}" for k in sorted(v)) + "\n}"
        else:
            v = line(v)
        parts.append(f"{line(section)}:{v}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main():
    with open(OUT, "w") as f:
        f.write(dumps(record()))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
