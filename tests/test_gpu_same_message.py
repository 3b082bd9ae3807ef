"""Same-message batch verification on the GPU (bgv_verify_same_message):
stage parity of the per-group sums against the Python oracle, a differential
against the untouched bgv_verify (every set as a one-set job with its message
replicated), the cancellation and identity-aggregate cases, library-drawn
scalars and the Python binding.  Run on an MI355X (-m gpu)."""
import asyncio
import hashlib

import numpy as np
import pytest

from oracle import bls12_381 as B
from oracle import cref
from tests import gpu_util as G
from tests import hostcheck as H

pytestmark = pytest.mark.gpu

SEED = 0x53414D45
N_KEYS = 1024
SEG = 64  # msm_g1.h SM_SEG
# 1, 2, maximum - 1, maximum, maximum + 1 (= 63, 64, 65), two full segments, 300: 623 sets
SIZES = [1, 2, SEG - 1, SEG, SEG + 1, 2 * SEG, 300]
EDGE = [1, 2**64 - 1, 0x1000000000000000, 0xF]


def msg_of(g):
    return hashlib.sha256(b"same-message group %d" % g).digest()


@pytest.fixture(scope="module")
def dev():
    from lodestar_amd import native
    d = native.Device(0)
    d.gen_keys(0, N_KEYS, SEED)
    # two more rows from the golden generator: -P_24 of the interop keys (any non-identity row) and the identity
    d.pubkeys_set(N_KEYS, b"".join(bytes.fromhex(x) for x in G.batch_vectors()["extra_table"]), native.PK_UNCOMPRESSED_96)
    yield d
    d.close()


@pytest.fixture(scope="module")
def layout(dev):
    """the clean batch shared by the tests (left unchanged): indices, signatures, scalars"""
    rng = np.random.default_rng(7)
    n = sum(SIZES)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    idx = rng.integers(0, N_KEYS, size=n).astype(np.uint32)
    scalars = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    big = int(off[6])
    scalars[big:big + 4] = EDGE  # the edge scalars
    scalars[off[2]:off[3]] = 0x0123456789ABCDEF  # a group with all-equal scalars
    idx[big + 10] = idx[big + 11]  # one validator twice, with equal scalars: one bucket gets P + P
    scalars[big + 10] = scalars[big + 11]
    group = np.repeat(np.arange(len(SIZES)), SIZES)
    msgs = np.stack([np.frombuffer(msg_of(g), np.uint8) for g in range(len(SIZES))])
    sigs = sign(dev, idx, msgs[group])
    return {"n": n, "off": off, "idx": idx, "scalars": scalars, "group": group, "msgs": msgs, "sigs": sigs}


def sign(dev, idx, msgs_per_set):
    n = len(idx)
    arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32),
              "pk_offsets": np.arange(n + 1, dtype=np.uint32), "pk_indices": np.ascontiguousarray(idx, np.uint32),
              "msgs": np.ascontiguousarray(msgs_per_set, np.uint8)}
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign(arrays, sigs)
    return sigs


def sm_arrays(L, idx=None, sigs=None, sig_len=None, scalars="layout"):
    n = L["n"]
    return {"n_sets": n, "n_groups": len(SIZES), "group_offsets": L["off"],
            "pk_indices": np.ascontiguousarray(L["idx"] if idx is None else idx, np.uint32), "msgs": L["msgs"],
            "sigs": np.ascontiguousarray(L["sigs"] if sigs is None else sigs, np.uint8),
            "sig_len": np.full(n, 96, np.uint32) if sig_len is None else sig_len,
            "scalars": L["scalars"] if isinstance(scalars, str) else scalars}


def one_set_jobs(L, idx, sigs, sig_len):
    """the yardstick's batch: set i as a one-set job, its group's message replicated"""
    n = L["n"]
    return {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32),
            "pk_offsets": np.arange(n + 1, dtype=np.uint32), "pk_indices": np.ascontiguousarray(idx, np.uint32),
            "msgs": np.ascontiguousarray(L["msgs"][L["group"]]), "sigs": np.ascontiguousarray(sigs, np.uint8),
            "sig_len": sig_len, "scalars": L["scalars"]}


def test_stage_parity(dev, layout):
    L = layout
    out = dev.debug_same_message(sm_arrays(L))
    assert out["set_valid"].all()
    assert (out["set_code"] == 0).all()
    st = out["stats"]
    n_segments = sum((s + SEG - 1) // SEG for s in SIZES)
    assert st["n_sets"] == L["n"] and st["n_groups"] == len(SIZES) and st["n_segments"] == n_segments
    assert st["hashes"] == len(SIZES)
    assert st["pairs"] <= 2 * n_segments
    assert st["groups_retried"] == 0 and st["sets_retried"] == 0
    for g in range(len(SIZES)):
        lo, hi = int(L["off"][g]), int(L["off"][g + 1])
        # sum r_i pk_i = (sum r_i sk_i) G1 and sum r_i sigma_i = (sum r_i sk_i) H(m): one oracle multiplication each
        k = sum(int(L["scalars"][i]) * cref.device_sk(SEED, int(L["idx"][i])) for i in range(lo, hi)) % B.R
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


KINDS = ["wrong_message", "other_validator", "flag_byte", "x_ge_p", "not_on_curve", "length_32", "not_in_g2",
         "identity_sig", "index_past_table", "identity_row"]


def faulted(dev, L):
    """~5% of the sets faulted, every kind at least three times; groups 0, 3 and 5 stay clean, group 1 is all bad"""
    rng = np.random.default_rng(23)
    idx, sigs, sig_len = L["idx"].copy(), L["sigs"].copy(), np.full(L["n"], 96, np.uint32)
    off = L["off"]
    where = [int(off[1]), int(off[1]) + 1]  # the group of two: entirely bad
    for g, count in ((2, 5), (4, 6), (6, 19)):
        where += [int(off[g]) + int(x) for x in rng.choice(SIZES[g], size=count, replace=False)]
    kinds = {}
    wrong = sign(dev, idx[where], np.stack([np.frombuffer(msg_of(99), np.uint8)] * len(where)))
    other = sign(dev, (idx[where] + 1) % N_KEYS, L["msgs"][L["group"][where]])
    for k, i in enumerate(where):
        kind = "wrong_message" if k < 2 else KINDS[k % len(KINDS)]
        kinds[i] = kind
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
        elif kind == "index_past_table":
            idx[i] = N_KEYS + 2 + k
        elif kind == "identity_row":
            idx[i] = N_KEYS + 1
    return idx, sigs, sig_len, kinds


def test_differential_against_bgv_verify(dev, layout):
    L = layout
    idx, sigs, sig_len, kinds = faulted(dev, L)
    assert set(kinds.values()) == set(KINDS)
    assert 0.04 * L["n"] <= len(kinds) <= 0.06 * L["n"]
    jr, sc = dev.verify(one_set_jobs(L, idx, sigs, sig_len))  # the yardstick: unchanged by this work
    ok, code = dev.verify_same_message(sm_arrays(L, idx, sigs, sig_len))
    st = dev.last_sm_stats.as_dict()
    want_ok = jr == 1
    want_code = sc.copy()
    # include/bgv.h names one code of its own: an identity signature is rejected before aggregation with
    # BGV_SET_VERIFY_FAIL (bgv_verify reports such a set as a failed pairing: result 0, code 0)
    ident = np.array([i for i, k in kinds.items() if k == "identity_sig"])
    assert (jr[ident] == 0).all() and (sc[ident] == 0).all()
    want_code[ident] = 5
    bad = sorted(kinds)
    print("faults:", {i: (kinds[i], int(jr[i]), int(sc[i]), bool(ok[i]), int(code[i])) for i in bad})
    print("stats:", st)
    assert not want_ok[bad].any() and want_ok.sum() == L["n"] - len(bad)
    assert {int(c) for c in sc[bad]} >= {0, 1, 2, 3, 6, 8, 9}  # every code the fault kinds stand for
    assert (ok == want_ok).all(), np.nonzero(ok != want_ok)[0]
    assert (code == want_code).all(), np.nonzero(code != want_code)[0]
    # the C restatement re-checks 16 sampled sets, faulted and clean (those with a key to hand it)
    rng = np.random.default_rng(5)
    have_key = [i for i in bad if kinds[i] not in ("index_past_table", "identity_row")]
    sample = list(rng.choice(have_key, size=8, replace=False)) + list(rng.choice(np.nonzero(want_ok)[0], size=8, replace=False))
    for i in map(int, sample):
        s = sigs[i, :96].tobytes() if sig_len[i] == 96 else bytes(int(sig_len[i]))
        r = cref.verify_job([dev.pubkeys_get(int(idx[i]), 1)], [msg_of(int(L["group"][i]))], [s], [int(L["scalars"][i])])
        assert (r == 1) == bool(ok[i]), (i, kinds.get(i), r)
        if r < 0:
            assert -r == int(code[i]), (i, kinds.get(i), r)
    # clean groups are not retried: only segments that hold a fault go to the per-set retry
    seg_sizes = {}
    for i in bad:
        g = int(L["group"][i])
        s0 = int(L["off"][g]) + (i - int(L["off"][g])) // SEG * SEG
        seg_sizes[s0] = min(SEG, int(L["off"][g + 1]) - s0)
    assert st["sets_retried"] <= sum(seg_sizes.values())
    assert 1 <= st["groups_retried"] <= 4 and st["hashes"] == len(SIZES)


def g2_point(b96):
    code, pt = B.g2_decompress(bytes(b96))
    assert code == 0
    return pt


def test_cancellation_needs_distinct_scalars(dev):
    """sigma_1 + D and sigma_2 - D: the unweighted sums verify, the weighted ones must not"""
    m = msg_of(1000)
    idx = np.array([3, 4], np.uint32)
    good = sign(dev, idx, np.stack([np.frombuffer(m, np.uint8)] * 2))
    D = B.E2.mul(B.hash_to_g2(b"cancellation point D"), 0xC0FFEE)  # a G2 subgroup point
    s1 = B.E2.add(g2_point(good[0, :96]), D)
    s2 = B.E2.add(g2_point(good[1, :96]), B.E2.neg(D))
    sigs = np.zeros((2, 192), np.uint8)
    sigs[0, :96] = np.frombuffer(B.g2_compress(s1), np.uint8)
    sigs[1, :96] = np.frombuffer(B.g2_compress(s2), np.uint8)
    arrays = {"n_sets": 2, "n_groups": 1, "group_offsets": np.array([0, 2], np.uint32), "pk_indices": idx,
              "msgs": np.frombuffer(m, np.uint8).reshape(1, 32).copy(), "sigs": sigs, "sig_len": np.full(2, 96, np.uint32)}
    # equal scalars: the aggregate check cannot tell (this is why the multipliers are random) -- the
    # group passes as a whole, as it would for blst's verifyMultipleAggregateSignatures with equal randomness
    ok, _ = dev.verify_same_message(dict(arrays, scalars=np.array([5, 5], np.uint64)))
    assert ok.tolist() == [True, True]
    ok, code = dev.verify_same_message(dict(arrays, scalars=np.array([5, 7], np.uint64)))
    assert ok.tolist() == [False, False]
    assert code.tolist() == [0, 0]
    assert dev.last_sm_stats.sets_retried == 2 and dev.last_sm_stats.groups_retried == 1


def test_identity_aggregate_is_no_error():
    """P and -P with equal scalars and correct signatures: sum r_i pk_i is the identity, both sets are valid"""
    from lodestar_amd import native
    d = native.Device(0)
    try:
        G.load_golden_table(d)
        neg_row = G.batch_vectors()["extra_table_base"]  # -P_24
        sk = B.interop_secret_key(24)
        assert d.pubkeys_get(neg_row, 1) == B.g1_serialize(B.E1.neg(B.sk_to_pk(sk)))
        m = msg_of(2000)
        sigs = np.zeros((2, 192), np.uint8)
        sigs[0, :96] = np.frombuffer(cref.sign(sk, m), np.uint8)
        sigs[1, :96] = np.frombuffer(cref.sign(B.R - sk, m), np.uint8)
        arrays = {"n_sets": 2, "n_groups": 1, "group_offsets": np.array([0, 2], np.uint32),
                  "pk_indices": np.array([24, neg_row], np.uint32), "msgs": np.frombuffer(m, np.uint8).reshape(1, 32).copy(),
                  "sigs": sigs, "sig_len": np.full(2, 96, np.uint32), "scalars": np.array([0x1234567, 0x1234567], np.uint64)}
        out = d.debug_same_message(arrays)
        assert out["set_valid"].tolist() == [True, True]
        assert out["set_code"].tolist() == [0, 0]
        assert out["p_group"][0].tobytes() == bytes(96)  # the identity, reported as all-zero
        # a third, ordinary member beside the pair
        sk5 = B.interop_secret_key(5)
        sigs3 = np.zeros((3, 192), np.uint8)
        sigs3[:2] = sigs
        sigs3[2, :96] = np.frombuffer(cref.sign(sk5, m), np.uint8)
        arrays3 = dict(arrays, n_sets=3, group_offsets=np.array([0, 3], np.uint32), pk_indices=np.array([24, neg_row, 5], np.uint32),
                       sigs=sigs3, sig_len=np.full(3, 96, np.uint32), scalars=np.array([9, 9, 11], np.uint64))
        ok, _ = d.verify_same_message(arrays3)
        assert ok.tolist() == [True, True, True]
        assert d.last_sm_stats.sets_retried == 0
    finally:
        d.close()


def test_library_drawn_scalars(dev, layout):
    L = layout
    verdicts = []
    for _ in range(2):  # two different draws, the same verdicts
        ok, code = dev.verify_same_message(sm_arrays(L, scalars=None))
        assert ok.all() and (code == 0).all()
        assert dev.last_sm_stats.groups_retried == 0
    bad = int(L["off"][4]) + 17
    sigs = L["sigs"].copy()
    sigs[bad] = L["sigs"][bad + 1]  # a valid signature of another validator
    assert L["idx"][bad] != L["idx"][bad + 1]
    for _ in range(2):
        ok, code = dev.verify_same_message(sm_arrays(L, sigs=sigs, scalars=None))
        verdicts.append(ok.copy())
        assert np.nonzero(~ok)[0].tolist() == [bad]
        assert (code == 0).all()
        assert dev.last_sm_stats.groups_retried == 1 and dev.last_sm_stats.sets_retried <= SEG
    assert (verdicts[0] == verdicts[1]).all()


def test_on_device_batch(dev, layout):
    """inputs resident in HBM: the verdicts of the host batch, one wrong signature included"""
    import torch
    import bench
    L = layout
    bad = int(L["off"][6]) + 77  # in the group of 300
    sigs = L["sigs"].copy()
    sigs[bad] = L["sigs"][bad - 1]  # its neighbour's: a valid signature of another validator
    assert L["idx"][bad] != L["idx"][bad - 1]
    a = sm_arrays(L, sigs=sigs)
    ok_host, code_host = dev.verify_same_message(a)
    da = bench.to_device(a, torch, torch.device("cuda", 0))
    ok, code = dev.verify_same_message(da, on_device=True)
    assert np.nonzero(~ok)[0].tolist() == [bad]
    assert (ok == ok_host).all() and (code == code_host).all()


def test_empty_batch(dev):
    arrays = {"n_sets": 0, "n_groups": 0, "group_offsets": np.array([0], np.uint32), "pk_indices": np.zeros(1, np.uint32),
              "msgs": np.zeros((1, 32), np.uint8), "sigs": np.zeros((1, 192), np.uint8), "sig_len": np.zeros(1, np.uint32)}
    ok, code = dev.verify_same_message(arrays)
    assert len(ok) == 0 and len(code) == 0


def test_bindings_three_calls_at_once():
    """BlsGpuVerifier.verify_signature_sets_same_message: two batchable calls and one not, one bad signature"""
    from lodestar_amd import verifier as V

    async def main():
        v = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1)
        try:
            for d in v._contexts():
                d.gen_keys(0, 64, SEED)
            d0 = v.devices[0]
            m1, m2 = msg_of(3000), msg_of(3001)

            def call(idxs, m):
                sigs = sign(d0, np.array(idxs, np.uint32), np.stack([np.frombuffer(m, np.uint8)] * len(idxs)))
                return [(V.PublicKey(index=i), sigs[k, :96].tobytes()) for k, i in enumerate(idxs)]

            a, b, c = call(list(range(0, 20)), m1), call(list(range(20, 40)), m1), call(list(range(40, 45)), m2)
            b[7] = (b[7][0], b[8][1])  # another validator's signature
            ra, rb, rc = await asyncio.gather(
                v.verify_signature_sets_same_message(a, m1, V.VerifySignatureOpts(batchable=True)),
                v.verify_signature_sets_same_message(b, m1, V.VerifySignatureOpts(batchable=True)),
                v.verify_signature_sets_same_message(c, m2))
            assert ra == [True] * 20
            assert rb == [k != 7 for k in range(20)]
            assert rc == [True] * 5
            assert 1 <= v._sm.device_calls <= 2  # merged: 40 > 32 buffered signatures flush the buffer
            assert v.metrics["same_message_sets_started"] == 45 and v.metrics["same_message_retries"] == 1
            assert await v.verify_signature_sets_same_message([], m1) == []
            s = V.BlsGpuSingleThreadVerifier(0)
            try:
                s.device.gen_keys(0, 64, SEED)
                assert await s.verify_signature_sets_same_message(b, m1) == rb
            finally:
                await s.close()
        finally:
            await v.close()

    asyncio.run(main())
