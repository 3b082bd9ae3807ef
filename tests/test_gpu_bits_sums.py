"""Resident key sums for bitfield sets on the GPU (bgv_index_list_sums and the
complement path of bgv_verify_bits): the prefix sums against the oracle on a
crafted list (equal neighbours, a key beside its negation, identity rows, an
identity prefix); the aggregate keys over every tile boundary of the scan
against the existing gather; degenerate windows; a verdict differential between
a context with sums and one without under four pipelines, host and on-device;
invalidation; refusals; an on-device source that breaks the contract.
Run on an MI355X (-m gpu)."""
import hashlib

import numpy as np
import pytest

from tests.test_gpu_bits import Builder, np_expand, to_device

pytestmark = pytest.mark.gpu

SEED = 0x53554D53
N_KEYS = 4400
B = N_KEYS  # first hand-placed row
ROW_P, ROW_Q, ROW_R = 10, 11, 20
ROW_P2, ROW_NP, ROW_INF, ROW_NQ = B, B + 1, B + 2, B + 3  # P again, -P, the identity, -Q
N_ROWS = B + 4
L_PERM, L_BIG, L_CRAFT, L_SYNC, L_PLAIN, L_SPARE = 0, 1, 2, 5, 6, 7
N_BIG = 70001
X = 0xFFFFFFFF
PK_IS_INFINITY, INDEX_RANGE = 6, 9
INF96 = bytes([0x40]) + bytes(95)

# the crafted list: S[2] = S[4] = S[6] = identity, S[8] = 2 P by the doubling
# (P + P from equal neighbours, one of them row 10's duplicate), S[5] = -S[1]
CRAFT_HEAD = [ROW_P, ROW_NP, ROW_NP, ROW_P, ROW_NP, ROW_P, ROW_P2, ROW_P,
              ROW_INF, ROW_INF, ROW_INF, ROW_INF,
              ROW_P, ROW_NP, ROW_P, ROW_NP, ROW_Q, ROW_NQ, ROW_R]


def build_lists():
    rng = np.random.default_rng(21)
    tail = rng.integers(0, N_KEYS, size=200 - len(CRAFT_HEAD)).astype(np.uint32)
    tail[::17] = ROW_INF
    return {L_PERM: np.random.default_rng(1).permutation(N_KEYS).astype(np.uint32),
            L_BIG: rng.integers(0, N_KEYS, size=N_BIG).astype(np.uint32),
            L_CRAFT: np.concatenate([np.array(CRAFT_HEAD, np.uint32), tail]),
            L_SYNC: np.random.default_rng(2).permutation(N_KEYS)[:512].astype(np.uint32),
            L_PLAIN: np.random.default_rng(3).permutation(N_KEYS)[:600].astype(np.uint32)}  # never gets sums


SUMMED = (L_PERM, L_BIG, L_CRAFT, L_SYNC)


def open_device(lists, sums, **cfg):
    """a context with the generated table, the hand-placed rows and the lists (sums on all but L_PLAIN)"""
    from lodestar_amd import native
    d = native.Device(0, **cfg)
    d.gen_keys(0, N_KEYS, SEED)
    rows = np.frombuffer(d.pubkeys_get(ROW_P, 2), np.uint8).reshape(2, 96)

    def negated(row):
        y = int.from_bytes(row[48:].tobytes(), "big")
        from oracle import bls12_381 as o
        return row[:48].tobytes() + ((o.P - y) % o.P).to_bytes(48, "big")

    hand = rows[0].tobytes() + negated(rows[0]) + INF96 + negated(rows[1])
    d.pubkeys_set(B, hand, native.PK_UNCOMPRESSED_96)
    assert d.pubkeys_count() == N_ROWS
    for k, v in lists.items():
        d.index_list_set(k, v)
        if sums and k in SUMMED:
            d.index_list_sums(k, True)
    return d


@pytest.fixture(scope="module")
def lists():
    return build_lists()


@pytest.fixture(scope="module")
def devs(lists):
    """(context with sums, context without): the same table and lists; left unchanged by the tests"""
    ds, dp = open_device(lists, True), open_device(lists, False)
    yield ds, dp
    ds.close()
    dp.close()


def rule(length, pop):
    return (length - pop) + 2 < pop


def want_path(a, has_sums):
    bits = np.unpackbits(a["bits"], bitorder="little")
    return [int(lst != X and lst in has_sums and rule(ln, int(bits[8 * bo:8 * bo + ln].sum())))
            for lst, _, ln, bo in a["src"].tolist()]


def with_dummy_signatures(e):
    """arrays bgv_debug_stages insists on; the key stages do not read them"""
    n = e["n_sets"]
    e["msgs"] = np.zeros((n, 32), np.uint8)
    e["sigs"] = np.zeros((n, 192), np.uint8)
    e["sigs"][:, 0] = 0xC0  # the identity, compressed
    e["sig_len"] = np.full(n, 96, np.uint32)
    return e


def direct_keys(dev, a, lists):
    """the existing gather on the numpy expansion (bgv_debug_stages: pk_agg is all-zero for a rejected key)"""
    po, idx = np_expand(a, lists)
    e = with_dummy_signatures({"n_sets": a["n_sets"], "n_jobs": a["n_jobs"], "job_offsets": a["job_offsets"],
                               "pk_offsets": po, "pk_indices": idx if idx.size else np.zeros(1, np.uint32)})
    return dev.debug_stages(e)


# ------------------------------------------------------------ 1. prefix values
def test_prefix_sums_equal_the_oracle(devs, lists):
    from oracle import bls12_381 as o
    ds, _ = devs
    table = np.frombuffer(ds.pubkeys_get(0, N_ROWS), np.uint8).reshape(N_ROWS, 96)

    def point(row):
        if row[0] & 0x40:
            return None
        return (int.from_bytes(row[:48].tobytes(), "big"), int.from_bytes(row[48:].tobytes(), "big"))

    def ser(pt):
        return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")

    lst = lists[L_CRAFT]
    assert lst.size == 200
    acc, want = None, [bytes(96)]
    for idx in lst.tolist():
        acc = o.E1.add(acc, point(table[idx]))
        want.append(ser(acc))
    # the list is what the issue asks for: an identity prefix past S[0], equal neighbours, a key beside its negation
    assert want[2] == bytes(96) and want[6] == bytes(96) and want[8] == ser(o.E1.dbl(point(table[ROW_P])))
    assert want[9] == want[8] == want[12]  # identity rows add nothing
    got = ds.debug_index_list_sums(L_CRAFT, 0, 201)
    assert got.shape == (201, 96)
    for k in range(201):
        assert got[k].tobytes() == want[k], k
    # a window of the read-back, and its bounds
    assert ds.debug_index_list_sums(L_CRAFT, 199, 2)[1].tobytes() == want[200]
    from lodestar_amd import native
    with pytest.raises(native.BgvNativeError) as e:
        ds.debug_index_list_sums(L_CRAFT, 200, 2)
    assert e.value.status == native.BGV_E_INVALID_ARG


# ------------------------------------------------------------ 2. scan boundaries
@pytest.fixture(scope="module")
def boundary_batch():
    rng = np.random.default_rng(9)
    windows = set()
    for k in range(1, 17):
        for edge in (2**k - 1, 2**k, 2**k + 1):
            if edge + 40 <= N_BIG:
                windows.add((edge, 40))
            if edge >= 40:
                windows.add((edge - 40, 40))
    windows = sorted(windows) + [(0, 1), (0, N_BIG), (N_BIG - 1, 1)]
    b = Builder()
    for off, length in windows:  # all bits set
        b.committee(L_BIG, off, np.ones(length, bool))
    for off, length in windows:  # three random bits clear (a one-member window keeps its bit)
        bits = np.ones(length, bool)
        bits[rng.permutation(length)[:min(3, length - 1)]] = False
        b.committee(L_BIG, off, bits)
    return b.arrays(), len(windows)


def test_keys_across_every_tile_boundary_equal_the_gather(devs, lists, boundary_batch):
    ds, dp = devs
    a, n_win = boundary_batch
    assert 150 <= a["n_sets"] <= 260
    ref = direct_keys(dp, a, lists)
    assert ref["pk_agg"].any(axis=1).all()
    want = want_path(a, SUMMED)
    assert want[:n_win - 3] == [1] * (n_win - 3)  # 40 of 40 and 37 of 40 are complement sets
    assert want[n_win - 3:n_win] == [0, 1, 0] and want[-3:] == [0, 1, 0]  # a one-member window is not
    for dev_arrays, on_device in ((a, False), (to_device(a), True)):
        pk, path, code = ds.debug_bits_keys(dev_arrays, on_device=on_device)
        assert path.tolist() == want
        assert not code.any()
        assert np.array_equal(pk, ref["pk_agg"])
    # the context without sums runs the same entry on the direct path
    pk, path, code = dp.debug_bits_keys(a)
    assert not path.any() and not code.any() and np.array_equal(pk, ref["pk_agg"])


# ------------------------------------------------------------ 3. degenerate windows
def test_degenerate_windows_equal_the_direct_path(devs, lists):
    ds, dp = devs
    b = Builder()
    b.committee(L_CRAFT, 0, np.ones(2, bool))     # [P, -P]: the identity (two members: direct by the rule)
    b.committee(L_CRAFT, 12, np.ones(4, bool))    # [P, -P, P, -P]: S[hi] == S[lo]
    b.committee(L_CRAFT, 1, np.ones(2, bool))     # [-P, -P] behind S[1] = P: S[hi] = -S[lo] (direct by the rule)
    b.committee(L_CRAFT, 1, np.ones(4, bool))     # [-P, -P, P, -P]: S[5] = -S[1], the doubling in the window chunk
    present = np.ones(7, bool)
    present[6] = False
    b.committee(L_CRAFT, 12, present)             # P - P + P - P + Q - Q present, R absent: window R, key the identity
    b.committee(L_CRAFT, 8, np.ones(4, bool))     # identity rows only
    b.committee(L_CRAFT, 0, np.ones(8, bool))     # ends on the doubled prefix: 2 P
    b.committee(L_CRAFT, 5, np.ones(14, bool))    # from an identity prefix across the identity rows
    a = b.arrays()
    ref = direct_keys(dp, a, lists)
    pk_d, path_d, code_d = dp.debug_bits_keys(a)  # the direct path of the same entry
    assert code_d.tolist() == [PK_IS_INFINITY, PK_IS_INFINITY, 0, 0, PK_IS_INFINITY, PK_IS_INFINITY, 0, 0]
    assert not path_d.any() and np.array_equal(pk_d, ref["pk_agg"])
    assert ref["pk_agg"].any(axis=1).tolist() == [False, False, True, True, False, False, True, True]
    want = want_path(a, SUMMED)
    assert want == [0, 1, 0, 1, 1, 1, 1, 1]
    for arrays, on_device in ((a, False), (to_device(a), True)):
        pk, path, code = ds.debug_bits_keys(arrays, on_device=on_device)
        assert path.tolist() == want
        assert code.tolist() == code_d.tolist()
        assert np.array_equal(pk, ref["pk_agg"])
    assert ds.bits_path_stats()["keys_gathered"] == 2 + 0 + 2 + 0 + 1 + 0 + 0 + 0


# ------------------------------------------------------------ 4. verdict differential
def sign(dev, a, lists, tag):
    n = a["n_sets"]
    a["msgs"] = np.stack([np.frombuffer(hashlib.sha256(b"%s %d" % (tag, i)).digest(), np.uint8) for i in range(n)])
    po, idx = np_expand(a, lists)
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({"n_sets": n, "n_jobs": a["n_jobs"], "job_offsets": a["job_offsets"], "pk_offsets": po, "pk_indices": idx,
                  "msgs": a["msgs"]}, sigs)
    a["sigs"] = sigs
    a["sig_len"] = np.full(n, 96, np.uint32)
    return a


@pytest.fixture(scope="module")
def signed(devs, lists):
    """40 sets in 4 jobs over generated rows (the signer knows their secret keys), signed once; left unchanged"""
    ds, _ = devs
    rng = np.random.default_rng(13)
    b = Builder()
    jobs = [0]
    for j in range(4):
        b.explicit([int(rng.integers(N_KEYS))])
        b.committee(L_PERM, 128 * j, np.ones(128, bool))                      # 100%
        one = np.ones(128, bool)
        one[int(rng.integers(128))] = False
        b.committee(L_PERM, 1000 + 128 * j, one)                              # one absent
        b.committee(L_PERM, 2000 + 128 * j, rng.random(128) < 0.5)            # 50%: direct by the rule
        b.committee(L_PLAIN, 128 * j, np.ones(128, bool))                     # a list without sums
        sync = np.ones(512, bool)
        sync[rng.permutation(512)[:5]] = False
        b.committee(L_SYNC, 0, sync)                                          # sync committee, 5 absent
        b.explicit(rng.integers(0, N_KEYS, size=33))
        near = rng.random(128) < 0.97
        b.committee(L_PERM, 3000 + 100 * j, near)
        if j == 1:
            big = rng.random(2049) < 0.99
            b.committee(L_PERM, 2351, big)                                    # ends on the list's last entry
        if j == 2:
            k = len(b.src)
            b.committee(L_PERM, 64, near)
            b.shared(L_PLAIN, 300, 128, k)                                    # the same bytes, a list without sums
        while len(b.src) < 10 * (j + 1):
            b.committee(L_SYNC, int(rng.integers(0, 384)), rng.random(128) < 0.99)
        jobs.append(len(b.src))
    a = b.arrays(jobs)
    assert a["n_sets"] == 40
    a["scalars"] = rng.integers(1, 2**64 - 1, size=40, dtype=np.uint64, endpoint=True)
    return sign(ds, a, lists, b"sums set")


PIPELINES = {"auto_latency": {}, "bulk_one_lane_pk": {"split": 0}, "bulk_two_pairs_over_lines": {"split": 0, "miller": 1, "pairs": 2, "lines": 1},
             "latency_one_lane_miller": {"split": 1, "miller": 1, "msm": 0}}


@pytest.mark.parametrize("name", list(PIPELINES))
def test_verdicts_with_sums_equal_those_without(devs, lists, signed, name):
    cfg = PIPELINES[name]
    pair = devs if not cfg else (open_device(lists, True, **cfg), open_device(lists, False, **cfg))
    try:
        ds, dp = pair
        faulty = dict(signed)
        faulty["sigs"] = signed["sigs"].copy()
        jo = signed["job_offsets"].tolist()
        faulty["sigs"][jo[2] + 1] = signed["sigs"][jo[2] + 2]  # job 2: a complement set with another set's signature
        n_cmpl = sum(want_path(signed, SUMMED))
        assert 20 <= n_cmpl < 40
        for a, want_jobs in ((signed, [1, 1, 1, 1]), (faulty, [1, 1, 0, 1])):
            for on_device in (False, True):
                arrays = to_device(a) if on_device else a
                out = []
                for d in (ds, dp):
                    jr, sc = d.verify_bits(arrays, on_device=on_device)
                    out.append((jr.tolist(), sc.tolist(), int(d.last_stats.pubkeys_aggregated), d.bits_path_stats()))
                (jr_s, sc_s, agg_s, path_s), (jr_p, sc_p, agg_p, path_p) = out
                assert jr_s == jr_p == want_jobs
                assert sc_s == sc_p
                assert agg_s == agg_p == np_expand(a, lists)[1].size
                assert path_s["sets_complement"] == n_cmpl and path_s["keys_gathered"] < path_s["keys_expanded"] == agg_s
                assert path_p["sets_complement"] == 0 and path_p["keys_gathered"] == path_p["keys_expanded"] == agg_p
        if name == "bulk_one_lane_pk":
            assert ds.last_stats.split == 0
        if name == "auto_latency":
            assert ds.last_stats.split == 1
    finally:
        if cfg:
            pair[0].close()
            pair[1].close()


# ------------------------------------------------------------ 5. never stale
def test_sums_are_never_stale(lists):
    from lodestar_amd import native
    d = open_device(lists, True)
    try:
        assert all(d.index_list_has_sums(k) for k in SUMMED) and not d.index_list_has_sums(L_PLAIN)
        member, donor = int(lists[L_PERM][40]), int(lists[L_PERM][3000])
        b = Builder()
        b.committee(L_PERM, 0, np.ones(128, bool))  # holds `member`
        a_old = sign(d, b.arrays(), lists, b"stale")
        swapped = {**lists, L_PERM: lists[L_PERM].copy()}
        swapped[L_PERM][40] = donor                 # what the table says once row `member` holds the donor's key
        a_new = sign(d, b.arrays(), swapped, b"stale")
        assert d.verify_bits(a_old)[0].tolist() == [1] and d.bits_path_stats()["sets_complement"] == 1
        assert d.verify_bits(a_new)[0].tolist() == [0]
        # the rewrite: one member row gets a different key
        d.pubkeys_set(member, d.pubkeys_get(donor, 1), native.PK_UNCOMPRESSED_96)
        assert not any(d.index_list_has_sums(k) for k in range(native.MAX_INDEX_LISTS))
        assert d.verify_bits(a_old)[0].tolist() == [0]  # stale sums would still accept it
        assert d.verify_bits(a_new)[0].tolist() == [1]
        assert d.bits_path_stats()["sets_complement"] == 0
        for k in SUMMED:
            d.index_list_sums(k, True)
        assert d.verify_bits(a_old)[0].tolist() == [0]
        assert d.verify_bits(a_new)[0].tolist() == [1]
        assert d.bits_path_stats() == {"sets_complement": 1, "keys_expanded": 128, "keys_gathered": 0}
        # replacing a list drops that list's sums only
        d.index_list_set(L_SYNC, lists[L_SYNC][::-1].copy())
        assert not d.index_list_has_sums(L_SYNC) and d.index_list_has_sums(L_PERM) and d.index_list_has_sums(L_BIG)
        # an append keeps them, a rewrite by gen_keys does not
        d.gen_keys(N_ROWS, 4, SEED + 1)
        assert d.index_list_has_sums(L_PERM) and d.verify_bits(a_new)[0].tolist() == [1]
        assert d.bits_path_stats()["sets_complement"] == 1
        d.index_list_sums(L_BIG, False)  # dropped on request
        assert not d.index_list_has_sums(L_BIG) and d.index_list_has_sums(L_PERM)
        d.gen_keys(N_ROWS + 3, 2, SEED + 2)  # rewrites the last row
        assert not d.index_list_has_sums(L_PERM)
    finally:
        d.close()


# ------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_list_usable(devs, lists):
    from lodestar_amd import native
    ds, _ = devs
    with pytest.raises(native.BgvNativeError) as e:
        ds.index_list_sums(L_SPARE, True)  # not set
    assert e.value.status == native.BGV_E_INVALID_ARG
    with pytest.raises(native.BgvNativeError) as e:
        ds.index_list_sums(native.MAX_INDEX_LISTS, True)
    assert e.value.status == native.BGV_E_INVALID_ARG
    ahead = lists[L_PERM][:300].copy()
    ahead[250] = N_ROWS  # the table count: a row that does not exist yet
    ds.index_list_set(L_SPARE, ahead)
    try:
        with pytest.raises(native.BgvNativeError) as e:
            ds.index_list_sums(L_SPARE, True)
        assert e.value.status == native.BGV_E_TABLE_RANGE and str(N_ROWS) in str(e.value)
        assert not ds.index_list_has_sums(L_SPARE)
        b = Builder()
        b.committee(L_SPARE, 0, np.ones(128, bool))
        a = sign(ds, b.arrays(), {**lists, L_SPARE: ahead}, b"refused")
        assert ds.verify_bits(a)[0].tolist() == [1]
        assert ds.bits_path_stats()["sets_complement"] == 0
    finally:
        ds.index_list_set(L_SPARE, np.zeros(0, np.uint32))


# ------------------------------------------------------------ 7. device robustness
def test_on_device_source_past_its_list_rejects_only_its_job(devs, lists, signed):
    ds, _ = devs
    a = dict(signed)
    jo = a["job_offsets"].tolist()
    src = signed["src"].copy()
    k = next(i for i in range(a["n_sets"]) if src[i]["list"] == L_SYNC and src[i]["len"] == 128)
    job = int(np.searchsorted(jo, k, side="right")) - 1
    src[k]["off"] = 512 - 128 + 1  # off + len is one past the list (and past its sums' last window)
    a["src"] = src
    jr, sc = ds.verify_bits(to_device(a), on_device=True)
    want = [1] * a["n_jobs"]
    want[job] = -INDEX_RANGE
    assert jr.tolist() == want
    assert sc[k] == INDEX_RANGE
    po, idx = np_expand(signed, lists)
    assert int(ds.last_stats.pubkeys_aggregated) == idx.size - int(po[k + 1] - po[k]) + 1  # the broken set counts one key
    assert ds.bits_path_stats()["sets_complement"] == sum(want_path(signed, SUMMED)) - 1
