"""Same-message batch verification of aggregate sets on the GPU
(bgv_verify_same_message_agg): stage parity of the per-set keys and the
per-group sums against the Python oracle, a differential against the untouched
bgv_verify (every set as a one-set job with its message replicated),
equivalence with bgv_verify_same_message on single-key sets, the identity
segment, library-drawn scalars, an on-device batch and the Python binding.
Run on an MI355X (-m gpu)."""
import asyncio
import hashlib

import numpy as np
import pytest

from oracle import bls12_381 as B
from oracle import cref
from tests import gpu_util as G
from tests import hostcheck as H

pytestmark = pytest.mark.gpu

SEED = 0x41474753
N_KEYS = 1024
NEG_ROW, INF_ROW = N_KEYS, N_KEYS + 1  # the golden extra rows: -P_24 of the interop keys, the identity
RAW0 = 0x80000000                      # raw key 0: P_24 of the interop keys
SEG = 64  # msm_g1.h SM_SEG
# stage parity: 1, 2, maximum - 1, maximum, maximum + 1, two segments and a bit (325 sets);
# the differential adds two groups, so that 36 faults are 5% (720 sets)
SIZES = [1, 2, SEG - 1, SEG, SEG + 1, 130]
SIZES_D = SIZES + [200, 195]
COUNTS = [1, 2, 31, 32, 33, 101, 512]  # around the gather's 32-key chunk; a sync-committee-sized set
COUNT_P = [0.3, 0.2, 0.1, 0.1, 0.1, 0.15, 0.05]
EDGE = [1, 2**64 - 1, 2**60, 0xF]


def msg_of(g):
    return hashlib.sha256(b"same-message aggregate group %d" % g).digest()


@pytest.fixture(scope="module")
def dev():
    from lodestar_amd import native
    d = native.Device(0)
    d.gen_keys(0, N_KEYS, SEED)
    d.pubkeys_set(N_KEYS, b"".join(bytes.fromhex(x) for x in G.batch_vectors()["extra_table"]), native.PK_UNCOMPRESSED_96)
    yield d
    d.close()


@pytest.fixture(scope="module")
def sks():
    return [cref.device_sk(SEED, i) for i in range(N_KEYS)]


def raw_p24():
    return np.frombuffer(B.g1_serialize(B.sk_to_pk(B.interop_secret_key(24))), np.uint8).copy()


def flatten(keys):
    off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32)
    return off, np.array([x for k in keys for x in k], np.uint32)


def sign(dev, keys, msgs_per_set):
    """device signatures of table-row key lists: (sum_j sk_j) H(m) per set"""
    n = len(keys)
    po, idx = flatten(keys)
    arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po, "pk_indices": idx,
              "msgs": np.ascontiguousarray(msgs_per_set, np.uint8)}
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign(arrays, sigs)
    return sigs


@pytest.fixture(scope="module")
def big(dev):
    """the clean 720-set batch shared by the tests (left unchanged); its first six groups are the stage-parity batch"""
    rng = np.random.default_rng(17)
    sizes = SIZES_D
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    counts = rng.choice(COUNTS, size=n, p=COUNT_P)
    b5 = int(off[5])
    counts[b5:b5 + len(COUNTS)] = COUNTS  # every count is present, in the group of 130
    keys = [[int(x) for x in rng.integers(0, N_KEYS, size=c)] for c in counts]
    scalars = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    scalars[b5:b5 + 4] = EDGE  # the edge scalars
    scalars[off[2]:off[3]] = 0x0123456789ABCDEF  # a group with all-equal scalars
    keys[b5 + 10] = keys[b5 + 10][:1] * 2 + [5, 6, 7]  # one validator twice inside one set
    # two sets of one segment with the same keys in reversed order and equal scalars: one point in two
    # Jacobian representations meets itself in a bucket
    keys[b5 + 21] = keys[b5 + 20][::-1] if len(keys[b5 + 20]) > 1 else [3, 4, 5]
    keys[b5 + 20] = keys[b5 + 21][::-1]
    scalars[b5 + 21] = scalars[b5 + 20]
    group = np.repeat(np.arange(len(sizes)), sizes)
    msgs = np.stack([np.frombuffer(msg_of(g), np.uint8) for g in range(len(sizes))])
    sigs = sign(dev, keys, msgs[group])
    return {"n": n, "sizes": sizes, "off": off, "keys": keys, "scalars": scalars, "group": group, "msgs": msgs, "sigs": sigs}


def head(L, groups):
    """the first `groups` groups of a layout as a layout of its own"""
    n = int(L["off"][groups])
    return {"n": n, "sizes": L["sizes"][:groups], "off": L["off"][:groups + 1], "keys": L["keys"][:n], "scalars": L["scalars"][:n],
            "group": L["group"][:n], "msgs": L["msgs"][:groups], "sigs": L["sigs"][:n]}


def sma_arrays(L, keys=None, sigs=None, sig_len=None, scalars="layout"):
    n = L["n"]
    po, idx = flatten(L["keys"] if keys is None else keys)
    return {"n_sets": n, "n_groups": len(L["sizes"]), "group_offsets": L["off"], "pk_offsets": po, "pk_indices": idx,
            "raw_pks": raw_p24(), "n_raw": 1, "msgs": L["msgs"],
            "sigs": np.ascontiguousarray(L["sigs"] if sigs is None else sigs, np.uint8),
            "sig_len": np.full(n, 96, np.uint32) if sig_len is None else sig_len,
            "scalars": L["scalars"] if isinstance(scalars, str) else scalars}


def one_set_jobs(L, keys, sigs, sig_len):
    """the yardstick's batch: set i as a one-set job, its group's message replicated"""
    n = L["n"]
    po, idx = flatten(keys)
    return {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po, "pk_indices": idx,
            "raw_pks": raw_p24(), "n_raw": 1, "msgs": np.ascontiguousarray(L["msgs"][L["group"]]),
            "sigs": np.ascontiguousarray(sigs, np.uint8), "sig_len": sig_len, "scalars": L["scalars"]}


class FixedBaseG1:
    """k G1 for many k: the 255 doublings of G1 once (oracle arithmetic), then per scalar the mixed
    additions of the set bits in Jacobian coordinates over Python integers and one inversion.  Checked
    against B.E1.mul by the test that uses it."""

    def __init__(self):
        self.pow2 = [B.G1]
        for _ in range(254):
            self.pow2.append(B.E1.dbl(self.pow2[-1]))

    def mul(self, k):
        p = B.P
        X, Y, Z = 1, 1, 0
        for j in range(255):
            if not (k >> j) & 1:
                continue
            x2, y2 = self.pow2[j]
            if Z == 0:
                X, Y, Z = x2, y2, 1
                continue
            zz = Z * Z % p
            h = (x2 * zz - X) % p
            r = (y2 * zz * Z - Y) % p
            assert h != 0  # distinct multiples of G1: never a doubling
            hh = h * h % p
            hhh = hh * h % p
            v = X * hh % p
            X3 = (r * r - hhh - 2 * v) % p
            Y, Z = (r * (v - X3) - Y * hhh) % p, Z * h % p
            X = X3
        if Z == 0:
            return None
        zi = pow(Z, p - 2, p)
        return (X * zi * zi % p, Y * zi * zi * zi % p)


def test_stage_parity(dev, big, sks):
    L = head(big, len(SIZES))
    assert L["n"] == 325 and {len(k) for k in L["keys"]} >= set(COUNTS)
    out = dev.debug_same_message_agg(sma_arrays(L))
    assert out["set_valid"].all()
    assert (out["set_code"] == 0).all()
    st = out["stats"]
    n_segments = sum((s + SEG - 1) // SEG for s in SIZES)
    assert st["n_sets"] == L["n"] and st["n_groups"] == len(SIZES) and st["n_segments"] == n_segments
    assert st["hashes"] == len(SIZES)
    assert st["pairs"] <= 2 * n_segments
    assert st["groups_retried"] == 0 and st["sets_retried"] == 0
    # PK_i = (sum_j sk_ij) G1 per set
    fb = FixedBaseG1()
    set_sk = [sum(sks[j] for j in k) % B.R for k in L["keys"]]
    for k in (set_sk[0], set_sk[200]):
        assert fb.mul(k) == B.E1.mul(B.G1, k)
    for i, k in enumerate(set_sk):
        assert out["pk_set"][i].tobytes() == H.g1_b(fb.mul(k)), i
    for g in range(len(SIZES)):
        lo, hi = int(L["off"][g]), int(L["off"][g + 1])
        # sum r_i PK_i = (sum r_i sk_i) G1 and sum r_i sigma_i = (sum r_i sk_i) H(m): one oracle multiplication each
        k = sum(int(L["scalars"][i]) * set_sk[i] for i in range(lo, hi)) % B.R
        hm = B.hash_to_g2(msg_of(g))
        assert out["h_group"][g].tobytes() == H.g2_b(hm), g
        assert out["p_group"][g].tobytes() == H.g1_b(B.E1.mul(B.G1, k)), g
        assert out["s_group"][g].tobytes() == H.g2_b(B.E2.mul(hm, k)), g


def not_in_g2_signature(rng):
    """a compressed point on E2 outside G2 (a random x with a square right-hand side)"""
    while True:
        b = bytearray(rng.integers(0, 256, size=96, dtype=np.uint8).tobytes())
        b[0] = 0x80 | (b[0] & 0x0F)
        b[48] &= 0x0F
        code, pt = B.g2_decompress(bytes(b))
        if code == 0 and not B.g2_in_subgroup(pt):
            return bytes(b)


def not_on_curve_signature(rng):
    while True:
        b = bytearray(rng.integers(0, 256, size=96, dtype=np.uint8).tobytes())
        b[0] = 0x80 | (b[0] & 0x0F)
        b[48] &= 0x0F
        if B.g2_decompress(bytes(b))[0] == B.BLST_POINT_NOT_ON_CURVE:
            return bytes(b)


# the ten kinds of tests/test_gpu_same_message.py, then the two of aggregates: an identity row inside a finite
# aggregate (the set stays VALID) and an aggregate that is the identity (a key and its negation)
KINDS = ["wrong_message", "other_validator", "flag_byte", "x_ge_p", "not_on_curve", "length_32", "not_in_g2",
         "identity_sig", "index_past_table", "identity_row", "identity_in_finite", "identity_aggregate"]
STILL_VALID = ("identity_in_finite",)


def faulted(dev, L):
    """5% of the sets touched, every kind three times; groups 0 and 3 stay clean, group 1 is all bad"""
    rng = np.random.default_rng(29)
    keys, sigs, sig_len = [list(k) for k in L["keys"]], L["sigs"].copy(), np.full(L["n"], 96, np.uint32)
    off, sizes = L["off"], L["sizes"]
    where = [int(off[1]), int(off[1]) + 1]  # the group of two: entirely bad
    for g, count in ((2, 5), (4, 6), (5, 8), (6, 9), (7, 6)):
        where += [int(off[g]) + int(x) for x in rng.choice(sizes[g], size=count, replace=False)]
    assert len(where) == 3 * len(KINDS)
    plan = ["wrong_message", "wrong_message"] + [KINDS[k % len(KINDS)] for k in range(2, len(where))]
    plan[plan.index("wrong_message", 2)] = "other_validator"  # three of each: the first two slots took two
    assert all(plan.count(k) == 3 for k in KINDS)
    wrong = sign(dev, [keys[i] for i in where], np.stack([np.frombuffer(msg_of(99), np.uint8)] * len(where)))
    other = sign(dev, [[(keys[i][0] + 1) % N_KEYS] + keys[i][1:] for i in where], L["msgs"][L["group"][where]])
    kinds, seen = {}, {}
    for k, i in enumerate(where):
        kind = plan[k]
        kinds[i] = kind
        nth = seen[kind] = seen.get(kind, -1) + 1
        if kind == "wrong_message":
            sigs[i] = wrong[k]
        elif kind == "other_validator":
            sigs[i] = other[k]
        elif kind == "flag_byte":
            sigs[i, 0] &= 0x7F
        elif kind == "x_ge_p":
            sigs[i, :96] = np.frombuffer(bytes([0x9F]) + b"\xff" * 95, np.uint8)
        elif kind == "not_on_curve":
            sigs[i, :96] = np.frombuffer(not_on_curve_signature(rng), np.uint8)
        elif kind == "length_32":
            sig_len[i] = 32
        elif kind == "not_in_g2":
            sigs[i, :96] = np.frombuffer(not_in_g2_signature(rng), np.uint8)
        elif kind == "identity_sig":
            sigs[i, :96] = np.frombuffer(bytes([0xC0]) + bytes(95), np.uint8)
        elif kind == "index_past_table":  # first, middle and last within a list that spans two chunks
            ks = (keys[i] + [1, 2, 3] * 12)[:35]
            ks[[0, 17, 34][nth]] = N_KEYS + 2 + k
            keys[i] = ks
        elif kind == "identity_row":  # nothing but identity rows
            keys[i] = [INF_ROW] * (nth + 1)
        elif kind == "identity_in_finite":  # the signature still fits: the row adds nothing
            keys[i] = keys[i][:]
            keys[i].insert([0, len(keys[i]) // 2, len(keys[i])][nth], INF_ROW)
        elif kind == "identity_aggregate":  # P_24 (raw key 0) beside -P_24, alone or around rows that cancel nothing
            keys[i] = [[RAW0, NEG_ROW], [NEG_ROW, INF_ROW, RAW0], [NEG_ROW, RAW0, NEG_ROW, RAW0]][nth]
    return keys, sigs, sig_len, kinds


def test_differential_against_bgv_verify(dev, big):
    L = big
    keys, sigs, sig_len, kinds = faulted(dev, L)
    assert set(kinds.values()) == set(KINDS) and len(kinds) == 36 and L["n"] == 720  # 5%
    jr, sc = dev.verify(one_set_jobs(L, keys, sigs, sig_len))  # the yardstick: unchanged by this work
    ok, code = dev.verify_same_message_agg(sma_arrays(L, keys, sigs, sig_len))
    st = dev.last_sm_stats.as_dict()
    want_ok = jr == 1
    want_code = sc.copy()
    # include/bgv.h names one code of its own: an identity signature is rejected before aggregation with
    # BGV_SET_VERIFY_FAIL (bgv_verify reports such a set as a failed pairing: result 0, code 0)
    ident = np.array([i for i, k in kinds.items() if k == "identity_sig"])
    assert (jr[ident] == 0).all() and (sc[ident] == 0).all()
    want_code[ident] = 5
    touched = sorted(kinds)
    bad = [i for i in touched if kinds[i] not in STILL_VALID]
    print("faults:", {i: (kinds[i], int(jr[i]), int(sc[i]), bool(ok[i]), int(code[i])) for i in touched})
    print("stats:", st)
    assert not want_ok[bad].any() and want_ok.sum() == L["n"] - len(bad)
    assert {int(c) for c in sc[bad]} >= {0, 1, 2, 3, 6, 8, 9}  # every code the fault kinds stand for
    for i in touched:
        if kinds[i] in ("identity_row", "identity_aggregate"):
            assert sc[i] == 6, (i, kinds[i])  # BGV_SET_PK_IS_INFINITY
        if kinds[i] == "index_past_table":
            assert sc[i] == 9, i  # BGV_SET_INDEX_RANGE
    assert (ok == want_ok).all(), np.nonzero(ok != want_ok)[0]
    assert (code == want_code).all(), np.nonzero(code != want_code)[0]
    # the C restatement re-checks 16 sampled sets, faulted and clean, on the oracle-aggregated key
    table = dev.pubkeys_get(0, N_KEYS + 2)
    rng = np.random.default_rng(5)
    have_key = [i for i in bad if kinds[i] not in ("index_past_table", "identity_row", "identity_aggregate")]
    clean = [i for i in np.nonzero(want_ok)[0] if len(keys[i]) <= 101]
    sample = list(rng.choice(have_key, size=8, replace=False)) + list(rng.choice(clean, size=7, replace=False))
    sample.append(next(i for i in touched if kinds[i] == "identity_in_finite"))
    for i in map(int, sample):
        pk = cref.aggregate([table[96 * j:96 * j + 96] for j in keys[i] if j != INF_ROW])
        s = sigs[i, :96].tobytes() if sig_len[i] == 96 else bytes(int(sig_len[i]))
        r = cref.verify_job([pk], [msg_of(int(L["group"][i]))], [s], [int(L["scalars"][i])])
        assert (r == 1) == bool(ok[i]), (i, kinds.get(i), r)
        if r < 0:
            assert -r == int(code[i]), (i, kinds.get(i), r)
    # clean groups are not retried: only segments that hold a failing pairing go to the per-set retry
    seg_sizes = {}
    for i in bad:
        g = int(L["group"][i])
        s0 = int(L["off"][g]) + (i - int(L["off"][g])) // SEG * SEG
        seg_sizes[s0] = min(SEG, int(L["off"][g + 1]) - s0)
    assert st["sets_retried"] <= sum(seg_sizes.values())
    assert 1 <= st["groups_retried"] <= 6 and st["hashes"] == len(SIZES_D)


def test_single_key_sets_match_the_single_key_entry(dev):
    """the layout of tests/test_gpu_same_message.py through both entries: verdicts, codes and group sums"""
    sizes = [1, 2, SEG - 1, SEG, SEG + 1, 2 * SEG, 300]
    rng = np.random.default_rng(7)
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    idx = rng.integers(0, N_KEYS, size=n).astype(np.uint32)
    scalars = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    b6 = int(off[6])
    scalars[b6:b6 + 4] = EDGE
    scalars[off[2]:off[3]] = 0x0123456789ABCDEF
    idx[b6 + 10] = idx[b6 + 11]
    scalars[b6 + 10] = scalars[b6 + 11]
    group = np.repeat(np.arange(len(sizes)), sizes)
    msgs = np.stack([np.frombuffer(msg_of(100 + g), np.uint8) for g in range(len(sizes))])
    sigs = sign(dev, [[int(x)] for x in idx], msgs[group])
    sig_len = np.full(n, 96, np.uint32)
    single = {"n_sets": n, "n_groups": len(sizes), "group_offsets": off, "pk_indices": idx, "msgs": msgs, "sigs": sigs,
              "sig_len": sig_len, "scalars": scalars}
    agg = dict(single, pk_offsets=np.arange(n + 1, dtype=np.uint32))
    a, b = dev.debug_same_message(single), dev.debug_same_message_agg(agg)
    assert a["set_valid"].all() and b["set_valid"].all()
    for k in ("set_code", "p_group", "s_group", "h_group"):
        assert np.array_equal(a[k], b[k]), k
    # and with faults of every stage: a wrong signature, an index past the table, the identity row, an identity and a
    # malformed signature
    idx2, sigs2, len2 = idx.copy(), sigs.copy(), sig_len.copy()
    sigs2[b6 + 70] = sigs[b6 + 71]
    assert idx[b6 + 70] != idx[b6 + 71]
    idx2[int(off[4]) + 3] = N_KEYS + 7
    idx2[int(off[5]) + 100] = INF_ROW
    sigs2[int(off[3]) + 9, :96] = np.frombuffer(bytes([0xC0]) + bytes(95), np.uint8)
    len2[int(off[2]) + 1] = 32
    single2 = dict(single, pk_indices=idx2, sigs=sigs2, sig_len=len2)
    a, b = dev.debug_same_message(single2), dev.debug_same_message_agg(dict(single2, pk_offsets=agg["pk_offsets"]))
    assert (~a["set_valid"]).sum() == 5
    for k in ("set_valid", "set_code", "p_group", "s_group", "h_group"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"]["sets_retried"] == b["stats"]["sets_retried"] > 0


def test_identity_segment_goes_to_the_retry(dev, sks):
    """PK_0 = A + B + P_24 and PK_1 = -P_24 - (A + B) with equal scalars and correct signatures: the segment's
    sum is the identity, which is no error; both sets verify in the per-set retry"""
    sk24 = B.interop_secret_key(24)
    ab = B.E1.add(B.E1.mul(B.G1, sks[3]), B.E1.mul(B.G1, sks[4]))
    raw = np.frombuffer(B.g1_serialize(B.sk_to_pk(sk24)) + B.g1_serialize(B.E1.neg(ab)), np.uint8).copy()
    sk0 = (sks[3] + sks[4] + sk24) % B.R
    m = msg_of(2000)
    sigs = np.zeros((2, 192), np.uint8)
    sigs[0, :96] = np.frombuffer(cref.sign(sk0, m), np.uint8)
    sigs[1, :96] = np.frombuffer(cref.sign(B.R - sk0, m), np.uint8)
    arrays = {"n_sets": 2, "n_groups": 1, "group_offsets": np.array([0, 2], np.uint32),
              "pk_offsets": np.array([0, 3, 5], np.uint32), "pk_indices": np.array([3, RAW0, 4, NEG_ROW, RAW0 | 1], np.uint32),
              "raw_pks": raw, "n_raw": 2, "msgs": np.frombuffer(m, np.uint8).reshape(1, 32).copy(), "sigs": sigs,
              "sig_len": np.full(2, 96, np.uint32), "scalars": np.array([0x1234567, 0x1234567], np.uint64)}
    out = dev.debug_same_message_agg(arrays)
    assert out["set_valid"].tolist() == [True, True]
    assert out["set_code"].tolist() == [0, 0]
    assert out["p_group"][0].tobytes() == bytes(96)  # the identity, reported as all-zero
    assert out["pk_set"][0].tobytes() == H.g1_b(B.E1.mul(B.G1, sk0))
    assert out["stats"]["sets_retried"] == 2 and out["stats"]["groups_retried"] == 1 and out["stats"]["pairs"] == 0
    # the retry decides every set on its own: a wrong signature beside the pair fails alone
    sigs[1, :96] = sigs[0, :96]
    ok, code = dev.verify_same_message_agg(arrays)
    assert ok.tolist() == [True, False] and code.tolist() == [0, 0]


def test_library_drawn_scalars(dev, big):
    L = head(big, len(SIZES))
    for _ in range(2):  # two different draws, the same verdicts
        ok, code = dev.verify_same_message_agg(sma_arrays(L, scalars=None))
        assert ok.all() and (code == 0).all()
        assert dev.last_sm_stats.groups_retried == 0
    bad = int(L["off"][4]) + 17
    sigs = L["sigs"].copy()
    sigs[bad] = L["sigs"][bad + 1]  # a valid signature of another aggregate
    assert sorted(L["keys"][bad]) != sorted(L["keys"][bad + 1])
    verdicts = []
    for _ in range(2):
        ok, code = dev.verify_same_message_agg(sma_arrays(L, sigs=sigs, scalars=None))
        verdicts.append(ok.copy())
        assert np.nonzero(~ok)[0].tolist() == [bad]
        assert (code == 0).all()
        assert dev.last_sm_stats.groups_retried == 1 and dev.last_sm_stats.sets_retried <= SEG
    assert (verdicts[0] == verdicts[1]).all()


def test_empty_batch(dev):
    arrays = {"n_sets": 0, "n_groups": 0, "group_offsets": np.array([0], np.uint32), "pk_offsets": np.array([0], np.uint32),
              "pk_indices": np.zeros(1, np.uint32), "msgs": np.zeros((1, 32), np.uint8), "sigs": np.zeros((1, 192), np.uint8),
              "sig_len": np.zeros(1, np.uint32)}
    ok, code = dev.verify_same_message_agg(arrays)
    assert len(ok) == 0 and len(code) == 0


def test_on_device_batch(dev, big):
    """inputs resident in HBM: the verdicts of the host batch, one wrong signature included"""
    import torch
    import bench
    L = head(big, len(SIZES))
    bad = int(L["off"][5]) + 77
    sigs = L["sigs"].copy()
    sigs[bad] = L["sigs"][bad - 1]
    assert sorted(L["keys"][bad]) != sorted(L["keys"][bad - 1])
    a = sma_arrays(L, sigs=sigs)
    ok_host, code_host = dev.verify_same_message_agg(a)
    da = bench.to_device(a, torch, torch.device("cuda", 0))
    ok, code = dev.verify_same_message_agg(da, on_device=True)
    assert np.nonzero(~ok)[0].tolist() == [bad]
    assert (ok == ok_host).all() and (code == code_host).all()


def test_bindings_three_calls_at_once():
    """BlsGpuVerifier.verify_aggregate_sets_same_message: two batchable calls and one not, one bad signature"""
    from lodestar_amd import verifier as V

    async def main():
        v = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1)
        try:
            for d in v._contexts():
                d.gen_keys(0, 64, SEED)
            d0 = v.devices[0]
            m1, m2 = msg_of(3000), msg_of(3001)
            rng = np.random.default_rng(3)

            def call(n, m, as_indices=False):
                keys = [[int(x) for x in rng.integers(0, 64, size=int(c))] for c in rng.choice([1, 2, 33, 40], size=n)]
                sigs = sign(d0, keys, np.stack([np.frombuffer(m, np.uint8)] * n))
                return [(k if as_indices else [V.PublicKey(index=i) for i in k], sigs[j, :96].tobytes()) for j, k in enumerate(keys)]

            a, b, c = call(20, m1), call(20, m1, as_indices=True), call(5, m2)
            n_keys = sum(len(k) for k, _ in a + b + c)
            b[7] = (b[7][0], b[8][1])  # another aggregate's signature
            assert sorted(b[7][0]) != sorted(b[8][0])
            ra, rb, rc = await asyncio.gather(
                v.verify_aggregate_sets_same_message(a, m1, V.VerifySignatureOpts(batchable=True)),
                v.verify_aggregate_sets_same_message(b, m1, V.VerifySignatureOpts(batchable=True)),
                v.verify_aggregate_sets_same_message(c, m2))
            assert ra == [True] * 20
            assert rb == [k != 7 for k in range(20)]
            assert rc == [True] * 5
            assert 1 <= v._sma.device_calls <= 2  # merged: 40 > 32 buffered signatures flush the buffer
            assert v._sm.device_calls == 0  # the single-key buffer is not involved
            assert v.metrics["same_message_agg_sets_started"] == 45 and v.metrics["same_message_agg_retries"] == 1
            assert v.metrics["aggregated_pubkeys_total"] == n_keys and v.metrics["same_message_sets_started"] == 0
            assert await v.verify_aggregate_sets_same_message([], m1) == []
            s = V.BlsGpuSingleThreadVerifier(0)
            try:
                s.device.gen_keys(0, 64, SEED)
                assert await s.verify_aggregate_sets_same_message(b, m1) == rb
            finally:
                await s.close()
        finally:
            await v.close()

    asyncio.run(main())
