"""Same-message batches of committee sets on the GPU
(bgv_verify_same_message_bits): parity with bgv_verify_same_message_agg on the
numpy expansion, on a context with resident sums and on one without, host and
on-device; degenerate windows of the crafted list; faults through the per-set
retry; an on-device batch that breaks the contract; library-drawn scalars.
Run on an MI355X (-m gpu)."""
import hashlib

import numpy as np
import pytest

from oracle import bls12_381 as O
from oracle import cref
from tests import hostcheck as H
from tests.test_gpu_bits import Builder, np_expand, to_device
from tests.test_gpu_bits_sums import (CRAFT_HEAD, L_CRAFT, L_PERM, L_PLAIN, L_SYNC, N_KEYS, ROW_INF, ROW_NP, ROW_NQ, ROW_P,
                                      ROW_P2, ROW_Q, ROW_R, SEED, SUMMED, build_lists, open_device, want_path)
from tests.test_gpu_same_message_agg import EDGE, SEG, FixedBaseG1, raw_p24

pytestmark = pytest.mark.gpu

X = 0xFFFFFFFF
RAW0 = 0x80000000  # raw key 0: P_24 of the interop keys
SIZES = [1, 2, SEG - 1, SEG, SEG + 1, 130]  # 325 sets
LENS = [1, 2, 31, 32, 33, 64, 65, 128, 512]  # both sides of the gather's 32-key chunk
BAD_ENCODING, PK_IS_INFINITY, INDEX_RANGE = 1, 6, 9
STAT_KEYS = ("n_sets", "n_groups", "n_segments", "hashes", "pairs", "groups_retried", "sets_retried")


def msg_of(g):
    return hashlib.sha256(b"same-message bits group %d" % g).digest()


@pytest.fixture(scope="module")
def lists():
    return build_lists()


@pytest.fixture(scope="module")
def devs(lists):
    """(context with sums, context without): the 4,400-key table plus the hand-placed rows, the permutation,
    the crafted list, the 512-entry list and L_PLAIN, which never gets sums; left unchanged by the tests"""
    ds, dp = open_device(lists, True), open_device(lists, False)
    yield ds, dp
    ds.close()
    dp.close()


@pytest.fixture(scope="module")
def row_sk():
    """the secret key of every table row: generated rows, then P again, -P, the identity, -Q"""
    sk = [cref.device_sk(SEED, i) for i in range(N_KEYS)]
    return sk + [sk[ROW_P], O.R - sk[ROW_P], 0, O.R - sk[ROW_Q]]


def set_sk(keys, row_sk):
    return sum(O.interop_secret_key(24) if k == RAW0 else row_sk[k] for k in keys) % O.R


def finish(b, sizes, lists, row_sk, dev, rng, tag=0):
    """a Builder's sets as a same-message batch in `sizes` groups: messages, scalars and the signatures of the
    participating keys (the device signs sets of generated rows, the C reference the others)"""
    a = b.arrays()
    n = a["n_sets"]
    assert n == sum(sizes)
    G = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    group = np.repeat(np.arange(G), sizes)
    msgs = np.stack([np.frombuffer(msg_of(tag + g), np.uint8) for g in range(G)])
    po, idx = np_expand(a, lists)
    keys = [idx[po[i]:po[i + 1]].tolist() for i in range(n)]
    by_hand = [i for i in range(n) if any(k >= N_KEYS for k in keys[i])]
    safe = [k if i not in by_hand else [0] for i, k in enumerate(keys)]
    spo = np.concatenate([[0], np.cumsum([len(k) for k in safe])]).astype(np.uint32)
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": spo,
                  "pk_indices": np.array([x for k in safe for x in k], np.uint32), "msgs": np.ascontiguousarray(msgs[group])}, sigs)
    for i in by_hand:
        k = set_sk(keys[i], row_sk)
        if k:  # an identity aggregate keeps the placeholder: a signature that decodes
            sigs[i, :96] = np.frombuffer(cref.sign(k, msg_of(tag + int(group[i]))), np.uint8)
    a.pop("n_jobs")
    a.pop("job_offsets")
    a.update({"n_groups": G, "group_offsets": off, "msgs": msgs, "raw_pks": raw_p24(), "n_raw": 1, "sigs": sigs,
              "sig_len": np.full(n, 96, np.uint32),
              "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)})
    return a, keys


def expansion(a, lists):
    """the bgv_sma_batch the contract names: pk_offsets / pk_indices are the numpy expansion, the rest is equal"""
    e = {"n_jobs": 1, "job_offsets": None, **a}
    po, idx = np_expand(e, lists)
    return {"n_sets": a["n_sets"], "n_groups": a["n_groups"], "group_offsets": a["group_offsets"], "pk_offsets": po,
            "pk_indices": idx, "raw_pks": a["raw_pks"], "n_raw": a["n_raw"], "msgs": a["msgs"], "sigs": a["sigs"],
            "sig_len": a["sig_len"], "scalars": a["scalars"]}


def stats_of(out):
    return {k: out["stats"][k] for k in STAT_KEYS}


# ------------------------------------------------------------ 1. parity
def pattern(kind, length, rng):
    bits = np.ones(length, bool)
    if kind == "one_clear" and length > 1:
        bits[int(rng.integers(length))] = False
    elif kind == "half":
        bits = rng.random(length) < 0.5
        bits[int(rng.integers(length))] = True
    return bits


def exactly(length, pop, rng):
    bits = np.zeros(length, bool)
    bits[rng.permutation(length)[:pop]] = True
    return bits


@pytest.fixture(scope="module")
def parity(devs, lists, row_sk):
    """325 sets in groups of 1, 2, 63, 64, 65 and 130; signed once, left unchanged"""
    ds, _ = devs
    rng = np.random.default_rng(31)
    b = Builder()
    n = sum(SIZES)
    b5 = n - 130
    special = {
        b5 + 20: lambda: b.committee(L_PERM, 700, exactly(128, 66, rng)),   # absent 62: complement
        b5 + 21: lambda: b.committee(L_PERM, 900, exactly(128, 65, rng)),   # absent 63: direct
        b5 + 22: lambda: b.committee(L_SYNC, 100, exactly(5, 4, rng)),      # absent 1: complement
        b5 + 23: lambda: b.committee(L_SYNC, 200, exactly(5, 3, rng)),      # absent 2: direct
        b5 + 24: lambda: b.explicit([7]),
        b5 + 25: lambda: b.explicit([RAW0, 8, 9]),                          # a raw key inside an explicit run
        b5 + 26: lambda: b.explicit(rng.integers(0, N_KEYS, size=33)),
        b5 + 27: lambda: b.committee(L_PERM, 4096 - 40, np.ones(128, bool)),  # across the sums' second level
        b5 + 28: lambda: b.committee(L_PERM, N_KEYS - 512, pattern("one_clear", 512, rng)),  # ends on the last entry
        3: lambda: b.explicit(rng.integers(0, N_KEYS, size=65)),
    }
    k = 0
    shared_from = None
    while len(b.src) < n:
        i = len(b.src)
        if i in special:
            special[i]()
            continue
        if i == b5 + 40:  # two sets over one bitfield, windows of two lists
            b.shared(L_SYNC, 301, 128, shared_from)
            continue
        length = LENS[k % len(LENS)]
        kind = ("ones", "one_clear", "half")[(k // len(LENS)) % 3]
        lst = (L_PERM, L_SYNC, L_PERM, L_PLAIN)[k % 4]
        room = len(lists[lst]) - length
        off = int(rng.integers(0, room + 1))
        b.committee(lst, off, pattern(kind, length, rng), align=(k % 4) if k % 5 == 0 else None)
        if length == 128 and lst == L_PERM and shared_from is None:
            shared_from = i
        k += 1
    assert shared_from is not None and shared_from < b5 + 40
    a, keys = finish(b, SIZES, lists, row_sk, ds, rng)
    a["scalars"][b5:b5 + 4] = EDGE
    a["scalars"][int(a["group_offsets"][2]):int(a["group_offsets"][3])] = 0x0123456789ABCDEF
    return a, keys


def test_parity_with_the_explicit_entry(devs, lists, parity, row_sk):
    ds, dp = devs
    a, keys = parity
    src = a["src"].tolist()
    assert a["n_sets"] == 325 and {s[2] for s in src if s[0] != X} >= set(LENS)
    assert any(s[3] % 2 == 1 for s in src if s[0] != X)  # odd bits_off
    assert len({s[3] for s in src if s[0] != X}) < sum(1 for s in src if s[0] != X)  # a shared bitfield
    want_s, want_p = want_path(a, SUMMED), [0] * a["n_sets"]
    b5 = a["n_sets"] - 130
    assert want_s[b5 + 20:b5 + 24] == [1, 0, 1, 0]
    e = expansion(a, lists)
    n_seg = sum((s + SEG - 1) // SEG for s in SIZES)
    for dev, want in ((ds, want_s), (dp, want_p)):
        ref = dev.debug_same_message_agg(e)
        assert ref["set_valid"].all() and not ref["set_code"].any()
        assert ref["stats"]["n_segments"] == n_seg and ref["stats"]["sets_retried"] == 0
        for arrays, on_device in ((a, False), (to_device(a), True)):
            out = dev.debug_same_message_bits(arrays, on_device=on_device)
            print("path stats:", on_device, dev.bits_path_stats(), stats_of(out))
            assert np.array_equal(out["set_valid"], ref["set_valid"])
            assert np.array_equal(out["set_code"], ref["set_code"])
            assert stats_of(out) == stats_of(ref)
            for key in ("pk_set", "p_group", "s_group", "h_group"):
                assert out[key].tobytes() == ref[key].tobytes(), (key, on_device)
            assert out["path"].tolist() == want
            ps = dev.bits_path_stats()
            assert ps["keys_expanded"] == e["pk_indices"].size
            if dev is ds:
                assert ps["sets_complement"] == sum(want_s) > 0 and ps["keys_gathered"] < ps["keys_expanded"]
            else:
                assert ps["sets_complement"] == 0 and ps["keys_gathered"] == ps["keys_expanded"]
    # not only device against device: PK_i = (sum_j sk_ij) G1 by the oracle's curve additions
    out = ds.debug_same_message_bits(a)
    fb = FixedBaseG1()
    k0 = set_sk(keys[0], row_sk)
    assert fb.mul(k0) == O.E1.mul(O.G1, k0)
    sample = [0, 1, 2, 3, b5 + 20, b5 + 21, b5 + 22, b5 + 23, b5 + 25, b5 + 27, b5 + 28, b5 + 40]
    sample += [i for i in range(4, a["n_sets"], 29)]
    assert {want_s[i] for i in sample} == {0, 1}
    for i in sample:
        assert out["pk_set"][i].tobytes() == H.g1_b(fb.mul(set_sk(keys[i], row_sk))), i


# ------------------------------------------------------------ 2. degenerate windows
def test_degenerate_windows(devs, lists, row_sk):
    ds, dp = devs
    assert CRAFT_HEAD[12:19] == [ROW_P, ROW_NP, ROW_P, ROW_NP, ROW_Q, ROW_NQ, ROW_R] and CRAFT_HEAD[6:8] == [ROW_P2, ROW_P]
    assert CRAFT_HEAD[8:12] == [ROW_INF] * 4
    rng = np.random.default_rng(37)
    b = Builder()
    b.committee(L_PERM, 10, np.ones(128, bool))
    b.committee(L_CRAFT, 0, np.ones(2, bool))      # 1: [P, -P], the identity (direct by the rule)
    b.committee(L_CRAFT, 12, np.ones(4, bool))     # 2: [P, -P, P, -P]: S[hi] == S[lo], the identity through the window
    b.committee(L_PERM, 300, pattern("one_clear", 65, rng))
    b.committee(L_CRAFT, 1, np.ones(4, bool))      # 4: [-P, -P, P, -P] behind S[1] = P: S[5] = -S[1], the doubling: -2 P
    absent_pair = np.ones(7, bool)
    absent_pair[:2] = False
    b.committee(L_CRAFT, 12, absent_pair)          # 5: P and -P absent (their sum is the identity): P - P + Q - Q + R = R
    b.committee(L_CRAFT, 6, np.ones(6, bool))      # 6: from the identity prefix S[6] over P, P and identity rows: 2 P
    absent_r = np.ones(7, bool)
    absent_r[6] = False
    b.committee(L_CRAFT, 12, absent_r)             # 7: the window is R, R absent: the identity
    b.committee(L_SYNC, 0, pattern("one_clear", 512, rng))
    b.explicit([5])
    a, keys = finish(b, [6, 4], lists, row_sk, ds, rng, tag=100)
    identity = [1, 2, 7]
    assert [i for i, k in enumerate(keys) if set_sk(k, row_sk) == 0] == identity
    want_ok = [i not in identity for i in range(10)]
    want_code = [PK_IS_INFINITY if i in identity else 0 for i in range(10)]
    assert want_path(a, SUMMED) == [1, 0, 1, 1, 1, 1, 1, 1, 1, 0]
    e = expansion(a, lists)
    for dev in (ds, dp):
        ref = dev.debug_same_message_agg(e)
        for arrays, on_device in ((a, False), (to_device(a), True)):
            out = dev.debug_same_message_bits(arrays, on_device=on_device)
            assert out["set_valid"].tolist() == want_ok, (dev is ds, on_device)
            assert out["set_code"].tolist() == want_code
            assert out["stats"]["sets_retried"] == 0 and out["stats"]["groups_retried"] == 0
            assert out["path"].tolist() == (want_path(a, SUMMED) if dev is ds else [0] * 10)
            for key in ("set_valid", "set_code", "pk_set", "p_group", "s_group", "h_group"):
                assert out[key].tobytes() == ref[key].tobytes(), key
        assert out["pk_set"][4].tobytes() == H.g1_b(O.E1.mul(O.G1, (O.R - 2 * row_sk[ROW_P]) % O.R))
        assert out["pk_set"][5].tobytes() == H.g1_b(O.E1.mul(O.G1, row_sk[ROW_R]))
        assert out["pk_set"][6].tobytes() == H.g1_b(O.E1.mul(O.G1, 2 * row_sk[ROW_P] % O.R))
        assert all(out["pk_set"][i].tobytes() == bytes(96) for i in identity)


# ------------------------------------------------------------ 3. faults
@pytest.fixture(scope="module")
def plain_batch(devs, lists, row_sk):
    """3 + 70 sets, 128-member windows of the permutation with one or two members absent; left unchanged"""
    ds, _ = devs
    rng = np.random.default_rng(41)
    b = Builder()
    for i in range(73):
        bits = np.ones(128, bool)
        bits[rng.permutation(128)[:1 + i % 2]] = False
        b.committee(L_PERM, 57 * i, bits)
    return finish(b, [3, 70], lists, row_sk, ds, rng, tag=200)


def test_faults_go_through_the_per_set_retry(devs, lists, plain_batch, row_sk):
    ds, _ = devs
    a, keys = plain_batch
    claimed, other_root, undecodable = 1, 3 + 10, 3 + 64 + 2  # group 0; group 1 segment 0; group 1 segment 1
    f = dict(a)
    f["bits"], f["sigs"] = a["bits"].copy(), a["sigs"].copy()
    s = a["src"][claimed]
    bo = int(s["bits_off"])
    field = np.unpackbits(f["bits"][bo:bo + 16], bitorder="little")
    j = int(np.nonzero(field == 0)[0][0])
    f["bits"][bo + j // 8] |= 1 << (j % 8)  # the bitfield claims a member who did not sign
    assert want_path(f, SUMMED)[claimed] == 1
    f["sigs"][other_root, :96] = np.frombuffer(cref.sign(set_sk(keys[other_root], row_sk), msg_of(999)), np.uint8)
    f["sigs"][undecodable, 0] &= 0x7F
    want_ok = np.ones(73, bool)
    want_ok[[claimed, other_root, undecodable]] = False
    want_code = np.zeros(73, np.int32)
    want_code[undecodable] = BAD_ENCODING
    for arrays, on_device in ((f, False), (to_device(f), True)):
        ok, code = ds.verify_same_message_bits(arrays, on_device=on_device)
        st = ds.last_sm_stats.as_dict()
        print("faults:", on_device, st, ds.bits_path_stats())
        assert (ok == want_ok).all(), np.nonzero(ok != want_ok)[0]
        assert (code == want_code).all()
        # the two failing pairings send their segments to the retry; the undecodable signature is rejected
        # before aggregation and its segment verifies without it
        assert st["groups_retried"] == 2 and st["sets_retried"] == 3 + 64
        assert st["n_segments"] == 3 and st["hashes"] == 2
    ref_ok, ref_code = ds.verify_same_message_agg(expansion(f, lists))
    assert (ref_ok == want_ok).all() and (ref_code == want_code).all()


# ------------------------------------------------------------ 4. an on-device batch that breaks the contract
def test_on_device_source_past_its_list_rejects_only_its_set(devs, lists, plain_batch):
    a, _ = plain_batch
    f = dict(a)
    src = a["src"].copy()
    bad = 3 + 5
    src[bad]["off"] = N_KEYS - 128 + 1  # off + len is one past the list (and past its sums' last window)
    f["src"] = src
    f["bits"] = a["bits"].copy()
    # padding: a 5-member window in place of set 3 + 20 whose byte carries bits above len
    pad = 3 + 20
    assert src[pad]["len"] == 128
    pad_keys = lists[L_PERM][int(src[pad]["off"]):int(src[pad]["off"]) + 5]
    src[pad]["len"] = 5
    f["bits"][int(src[pad]["bits_off"])] = 0xFF
    from tests.test_gpu_same_message_agg import sign
    f["sigs"] = a["sigs"].copy()
    ds, dp = devs
    f["sigs"][pad] = sign(ds, [pad_keys.tolist()], a["msgs"][1:2])[0]
    want_ok = np.ones(73, bool)
    want_ok[bad] = False
    want_code = np.zeros(73, np.int32)
    want_code[bad] = INDEX_RANGE
    for dev in (ds, dp):
        ok, code = dev.verify_same_message_bits(to_device(f), on_device=True)
        assert (ok == want_ok).all(), np.nonzero(ok != want_ok)[0]
        assert (code == want_code).all()
        assert dev.last_sm_stats.sets_retried == 0
        total = sum(int(np.unpackbits(a["bits"][int(s["bits_off"]):int(s["bits_off"]) + 16]).sum()) for s in a["src"])
        gone = [int(np.unpackbits(a["bits"][int(a["src"][i]["bits_off"]):int(a["src"][i]["bits_off"]) + 16]).sum()) for i in (bad, pad)]
        assert dev.bits_path_stats()["keys_expanded"] == total - sum(gone) + 1 + 5  # the broken set counts one key


# ------------------------------------------------------------ 5. library-drawn scalars
def test_library_drawn_scalars(devs, plain_batch):
    a, keys = plain_batch
    bad = 3 + 30
    f = dict(a, scalars=None)
    f["sigs"] = a["sigs"].copy()
    f["sigs"][bad] = a["sigs"][bad + 1]
    assert sorted(keys[bad]) != sorted(keys[bad + 1])
    for dev in devs:
        ok, code = dev.verify_same_message_bits(dict(a, scalars=None))
        assert ok.all() and not code.any() and dev.last_sm_stats.groups_retried == 0
        for _ in range(2):  # two different draws, the same verdicts
            ok, code = dev.verify_same_message_bits(f)
            assert np.nonzero(~ok)[0].tolist() == [bad] and not code.any()
            assert dev.last_sm_stats.groups_retried == 1 and dev.last_sm_stats.sets_retried == SEG
        # the scalars are drawn, not read from the batch: two calls weight the same keys differently
        one, two = (dev.debug_same_message_bits(dict(a, scalars=None)) for _ in range(2))
        assert np.array_equal(one["pk_set"], two["pk_set"]) and one["p_group"].any()
        assert one["p_group"].tobytes() != two["p_group"].tobytes() and one["s_group"].tobytes() != two["s_group"].tobytes()


def test_empty_batch(devs):
    from lodestar_amd import native
    a = {"n_sets": 0, "n_groups": 0, "group_offsets": np.array([0], np.uint32), "src": np.zeros(1, native.SET_SRC_DTYPE),
         "bits": np.zeros(1, np.uint8), "bits_len": 0, "pk_indices": np.zeros(1, np.uint32), "n_indices": 0,
         "msgs": np.zeros((1, 32), np.uint8), "sigs": np.zeros((1, 192), np.uint8), "sig_len": np.zeros(1, np.uint32)}
    ok, code = devs[0].verify_same_message_bits(a)
    assert len(ok) == 0 and len(code) == 0


# ------------------------------------------------------------ the Python bindings
def test_bindings_route_committee_sets(lists):
    """BlsGpuVerifier.verify_aggregate_sets_same_message: committee sets and explicit sets in merged calls go
    through the new entry, the key count comes from the device; a call without one takes the old path"""
    import asyncio

    from lodestar_amd import verifier as V
    from tests.test_gpu_same_message_agg import sign

    async def main():
        v = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1)
        try:
            for d in v._contexts():
                d.gen_keys(0, N_KEYS, SEED)
            v.set_index_list(L_PERM, lists[L_PERM], sums=True)
            d0 = v.devices[0]
            m1, m2 = msg_of(3000), msg_of(3001)
            rng = np.random.default_rng(3)

            def committee_call(n, m, base):
                sets, n_keys = [], 0
                for j in range(n):
                    bits = pattern(("ones", "one_clear", "half")[j % 3], 128, rng)
                    off = base + 130 * j
                    keys = lists[L_PERM][off:off + 128][bits].tolist()
                    sig = sign(d0, [keys], np.frombuffer(m, np.uint8).reshape(1, 32))[0, :96].tobytes()
                    sets.append((V.CommitteeKeys(V.CommitteeRef(L_PERM, off, 128), np.packbits(bits, bitorder="little").tobytes()), sig))
                    n_keys += len(keys)
                return sets, n_keys

            def explicit_call(n, m):
                keys = [[int(x) for x in rng.integers(0, N_KEYS, size=int(c))] for c in rng.choice([1, 2, 33], size=n)]
                sigs = sign(d0, keys, np.stack([np.frombuffer(m, np.uint8)] * n))
                return [(k, sigs[j, :96].tobytes()) for j, k in enumerate(keys)], sum(len(k) for k in keys)

            (a, ka), (b, kb), (c, kc) = committee_call(12, m1, 0), explicit_call(25, m1), explicit_call(5, m2)
            a[4] = (a[4][0], a[5][1])  # another committee's signature
            ra, rb = await asyncio.gather(
                v.verify_aggregate_sets_same_message(a, m1, V.VerifySignatureOpts(batchable=True)),
                v.verify_aggregate_sets_same_message(b, m1, V.VerifySignatureOpts(batchable=True)))
            assert ra == [k != 4 for k in range(12)] and rb == [True] * 25
            assert v._sma.device_calls == 1  # merged: 37 > 32 buffered signatures flush the buffer
            assert v.metrics["aggregated_pubkeys_total"] == ka + kb
            assert d0.bits_path_stats()["keys_expanded"] == ka + kb and d0.bits_path_stats()["sets_complement"] >= 8
            rc = await v.verify_aggregate_sets_same_message(c, m2)
            assert rc == [True] * 5
            assert v.metrics["aggregated_pubkeys_total"] == ka + kb + kc
            assert d0.bits_path_stats()["keys_expanded"] == ka + kb  # the explicit call left the path counters alone
            assert v.metrics["same_message_agg_sets_started"] == 42 and v.metrics["same_message_agg_retries"] == 1
            s = V.BlsGpuSingleThreadVerifier(0)
            try:
                s.device.gen_keys(0, N_KEYS, SEED)
                s.set_index_list(L_PERM, lists[L_PERM])
                assert await s.verify_aggregate_sets_same_message(a + b, m1) == ra + rb
                assert s.metrics["aggregated_pubkeys_total"] == ka + kb
            finally:
                await s.close()
        finally:
            await v.close()

    asyncio.run(main())
