"""The split retry of the same-message entries (bgv_sm_retry mode 1) on the GPU.
The yardsticks are the existing code, never the new mode: mode 0 on the same
batch and context, and bgv_verify over one-set jobs.  The retry counters are
checked against the counts the rule (sm_split.h, restated here in Python) gives
for the fault positions.  Run on an MI355X (-m gpu)."""
import numpy as np
import pytest

from oracle import bls12_381 as B
from oracle import cref
from tests import gpu_util as G
from tests import test_gpu_same_message as SM
from tests import test_gpu_same_message_agg as SMA

pytestmark = pytest.mark.gpu

SEED = 0x52545259
N_KEYS = 1024
NEG_ROW, INF_ROW = N_KEYS, N_KEYS + 1  # the golden extra rows: -P_24 of the interop keys, the identity
RAW0 = 0x80000000                      # raw key 0: P_24 of the interop keys
SEG, SUB = 64, 8
SIZES = [1, 2, 8, 9, 63, 64, 65, 128, 300]  # 640 sets, 15 segments
G2, G9, G64, G300 = 1, 3, 5, 8              # groups by size
STAT_KEYS = ("n_sets", "n_groups", "n_segments", "hashes", "pairs", "groups_retried", "sets_retried")
ZERO_PATH = {"segments": 0, "subs": 0, "subs_failed": 0, "leaves": 0, "pairs": 0, "hashes": 0}
PAIRING_KINDS = ("wrong_message", "other_validator")  # the faults that reach the pairing; the others are rejected before


def msg_of(g):
    return SM.msg_of(5000 + g)


@pytest.fixture(scope="module")
def dev():
    from lodestar_amd import native
    d = native.Device(0)
    d.gen_keys(0, N_KEYS, SEED)
    d.pubkeys_set(N_KEYS, b"".join(bytes.fromhex(x) for x in G.batch_vectors()["extra_table"]), native.PK_UNCOMPRESSED_96)
    yield d
    d.close()


@pytest.fixture(scope="module")
def layout(dev):
    """the clean batch shared by the tests (left unchanged), with distinct random scalars, and one
    wrong-message signature per set (signed once: a fault is a copy of its row)"""
    rng = np.random.default_rng(77)
    n = sum(SIZES)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    idx = rng.integers(0, N_KEYS, size=n).astype(np.uint32)
    scalars = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    assert len(set(scalars.tolist())) == n
    group = np.repeat(np.arange(len(SIZES)), SIZES)
    msgs = np.stack([np.frombuffer(msg_of(g), np.uint8) for g in range(len(SIZES))])
    sigs = SM.sign(dev, idx, msgs[group])
    wrong = SM.sign(dev, idx, np.stack([np.frombuffer(msg_of(99), np.uint8)] * n))
    return {"n": n, "off": off, "idx": idx, "scalars": scalars, "group": group, "msgs": msgs, "sigs": sigs, "wrong": wrong}


def sm_arrays(L, idx=None, sigs=None, sig_len=None, scalars="layout", raw=False):
    n = L["n"]
    a = {"n_sets": n, "n_groups": len(SIZES), "group_offsets": L["off"],
         "pk_indices": np.ascontiguousarray(L["idx"] if idx is None else idx, np.uint32), "msgs": L["msgs"],
         "sigs": np.ascontiguousarray(L["sigs"] if sigs is None else sigs, np.uint8),
         "sig_len": np.full(n, 96, np.uint32) if sig_len is None else sig_len,
         "scalars": L["scalars"] if isinstance(scalars, str) else scalars}
    if raw:
        a.update(raw_pks=SMA.raw_p24(), n_raw=1)
    return a


def yardstick(dev, L, a):
    """bgv_verify over one-set jobs, the group's message replicated: (valid, code in the same-message entries' terms)"""
    n = L["n"]
    jobs = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": np.arange(n + 1, dtype=np.uint32),
            "pk_indices": a["pk_indices"], "msgs": np.ascontiguousarray(L["msgs"][L["group"]]), "sigs": a["sigs"],
            "sig_len": a["sig_len"], "scalars": L["scalars"]}
    if "raw_pks" in a:
        jobs.update(raw_pks=a["raw_pks"], n_raw=a["n_raw"])
    jr, sc = dev.verify(jobs)
    code = sc.copy()
    # include/bgv.h: an identity signature is rejected before aggregation with BGV_SET_VERIFY_FAIL
    # (bgv_verify reports such a set as a failed pairing: result 0, code 0)
    ident = (a["sigs"][:, 0] == 0xC0) & (a["sig_len"] == 96) & (jr == 0) & (sc == 0)
    code[ident] = 5
    return jr == 1, code


def stats_of(dev):
    st = dev.last_sm_stats.as_dict()
    return {k: st[k] for k in STAT_KEYS}


def run(dev, mode, a, entry="verify_same_message", **kw):
    dev.sm_retry(mode)
    try:
        ok, code = getattr(dev, entry)(a, **kw)
        return ok, code, stats_of(dev), dev.sm_retry_stats()
    finally:
        dev.sm_retry(0)


def plan(m):
    return list(range(m + 1)) if m <= SUB else list(range(0, m, SUB)) + [m]


def want_path(off, skip, bad, identity_subs=()):
    """the counters of a mode 1 call by the rule: off the group offsets, skip the sets rejected before
    aggregation, bad the surviving sets whose pairing fails; identity_subs: (segment's first set, sub) pairs
    whose P_sub is the identity (not paired, failed)"""
    p = dict(ZERO_PATH, mode=1)
    skip, bad = set(map(int, skip)), set(map(int, bad))
    for g in range(len(off) - 1):
        for s0 in range(int(off[g]), int(off[g + 1]), SEG):
            live = [i for i in range(s0, min(s0 + SEG, int(off[g + 1]))) if i not in skip]
            if not any(i in bad for i in live):
                continue
            p["segments"] += 1
            cut = plan(len(live))
            for t in range(len(cut) - 1):
                sub = live[cut[t]:cut[t + 1]]
                ident = (s0, t) in identity_subs
                failed = ident or any(i in bad for i in sub)
                p["subs"] += 1
                p["pairs"] += 0 if ident else 2
                if failed:
                    p["subs_failed"] += 1
                    if len(sub) >= 2:
                        p["leaves"] += len(sub)
                        p["pairs"] += 2 * len(sub)
    return p


def mode0_path(st):
    r = st["sets_retried"]
    return {"mode": 0, "subs": 0, "subs_failed": 0, "leaves": r, "pairs": 2 * r, "hashes": r}


def both_modes(dev, L, a, skip, bad, identity_subs=(), entry="verify_same_message"):
    """mode 0, mode 1 and the yardstick on one batch: equal verdicts, codes and bgv_sm_stats; the retry
    counters of both modes as stated; returns (valid, mode 1's counters)"""
    ok0, code0, st0, p0 = run(dev, 0, a, entry)
    ok1, code1, st1, p1 = run(dev, 1, a, entry)
    want_ok, want_code = yardstick(dev, L, a)
    print("stats:", st1, "retry 0:", p0, "retry 1:", p1)
    assert (ok0 == want_ok).all() and (code0 == want_code).all()  # the ground the comparison stands on
    assert (ok1 == want_ok).all(), np.nonzero(ok1 != want_ok)[0]
    assert (code1 == want_code).all(), np.nonzero(code1 != want_code)[0]
    assert st1 == st0
    assert set(np.nonzero(~want_ok)[0].tolist()) == set(map(int, skip)) | set(map(int, bad))
    want = want_path(L["off"], skip, bad, identity_subs)
    assert p1 == want
    segs = p0.pop("segments")
    assert p0 == mode0_path(st0) and segs == want["segments"]
    return ok1, p1


def with_wrong(L, where):
    sigs = L["sigs"].copy()
    sigs[where] = L["wrong"][where]
    return sigs


def test_clean_batch_in_mode_1(dev, layout):
    ok, code, st, p = run(dev, 1, sm_arrays(layout))
    assert ok.all() and (code == 0).all()
    assert st["groups_retried"] == 0 and st["sets_retried"] == 0 and st["hashes"] == len(SIZES)
    assert p == dict(ZERO_PATH, mode=1)


def test_one_bad_set_of_64_costs_8_subs_and_8_leaves(dev, layout):
    L = layout
    bad = int(L["off"][G64]) + 29
    ok, p = both_modes(dev, L, sm_arrays(L, sigs=with_wrong(L, [bad])), [], [bad])
    assert np.nonzero(~ok)[0].tolist() == [bad]
    assert p == {"mode": 1, "segments": 1, "subs": 8, "subs_failed": 1, "leaves": 8, "pairs": 32, "hashes": 0}
    assert dev.last_sm_stats.sets_retried == 64


PLACEMENTS = {
    # name: (group, positions inside it) -> the counters of the call
    "sub_boundary_7_and_8": (G64, [7, 8], {"segments": 1, "subs": 8, "subs_failed": 2, "leaves": 16, "pairs": 48}),
    "two_in_one_sub": (G64, [17, 22], {"segments": 1, "subs": 8, "subs_failed": 1, "leaves": 8, "pairs": 32}),
    "two_in_different_subs": (G64, [3, 60], {"segments": 1, "subs": 8, "subs_failed": 2, "leaves": 16, "pairs": 48}),
    "group_of_two_all_bad": (G2, [0, 1], {"segments": 1, "subs": 2, "subs_failed": 2, "leaves": 0, "pairs": 4}),
    "last_of_nine": (G9, [8], {"segments": 1, "subs": 2, "subs_failed": 1, "leaves": 0, "pairs": 4}),
    "full_segment_all_bad": (G64, list(range(64)), {"segments": 1, "subs": 8, "subs_failed": 8, "leaves": 64, "pairs": 144}),
}


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_fault_placements(dev, layout, name):
    L = layout
    g, pos, want = PLACEMENTS[name]
    bad = [int(L["off"][g]) + k for k in pos]
    ok, p = both_modes(dev, L, sm_arrays(L, sigs=with_wrong(L, bad)), [], bad)
    assert np.nonzero(~ok)[0].tolist() == bad
    assert p == dict(want, mode=1, hashes=0)


def test_rejected_sets_shift_the_sub_boundaries(dev, layout):
    """a bad flag byte and an index past the table in front of a wrong-message set: 62 survivors, the bad one
    (set 9 of the segment) is survivor 7, the last of sub 0, and the last sub has 6 sets"""
    L = layout
    s0 = int(L["off"][G64])
    idx, sigs, sig_len = L["idx"].copy(), with_wrong(L, [s0 + 9]), np.full(L["n"], 96, np.uint32)
    sigs[s0 + 2, 0] &= 0x7F
    idx[s0 + 5] = N_KEYS + 7
    a = sm_arrays(L, idx, sigs, sig_len)
    ok, p = both_modes(dev, L, a, [s0 + 2, s0 + 5], [s0 + 9])
    assert np.nonzero(~ok)[0].tolist() == [s0 + 2, s0 + 5, s0 + 9]
    assert p == {"mode": 1, "segments": 1, "subs": 8, "subs_failed": 1, "leaves": 8, "pairs": 32, "hashes": 0}
    _, code, _, _ = run(dev, 1, a)
    assert code[[s0 + 2, s0 + 5, s0 + 9]].tolist() == [1, 9, 0]
    # one set further and the bad one opens sub 1 instead: the boundary did move with the compaction
    sigs2 = with_wrong(L, [s0 + 10])
    sigs2[s0 + 2, 0] &= 0x7F
    assert want_path(L["off"], [s0 + 2, s0 + 5], [s0 + 10]) == p
    ok, _ = both_modes(dev, L, sm_arrays(L, idx, sigs2, sig_len), [s0 + 2, s0 + 5], [s0 + 10])
    assert np.nonzero(~ok)[0].tolist() == [s0 + 2, s0 + 5, s0 + 10]


def test_identity_sub_goes_to_the_leaves(dev, layout):
    """P and -P with equal scalars and correct signatures inside sub 2 of the 64-group, a fault in sub 5: the
    identity sub is not paired, counts as failed, and its eight sets come out valid through the leaves"""
    L = layout
    s0 = int(L["off"][G64])
    sk = B.interop_secret_key(24)
    assert dev.pubkeys_get(NEG_ROW, 1) == B.g1_serialize(B.E1.neg(B.sk_to_pk(sk)))
    idx, sigs, scalars = L["idx"].copy(), with_wrong(L, [s0 + 40]), L["scalars"].copy()
    m = msg_of(G64)
    # the other six keys of the sub also cancel in pairs: P_sub is the identity
    for k in range(0, 8, 2):
        idx[s0 + 16 + k], idx[s0 + 17 + k] = RAW0, NEG_ROW
        sigs[s0 + 16 + k, :96] = np.frombuffer(cref.sign(sk, m), np.uint8)
        sigs[s0 + 17 + k, :96] = np.frombuffer(cref.sign(B.R - sk, m), np.uint8)
        scalars[s0 + 17 + k] = scalars[s0 + 16 + k]
    a = sm_arrays(L, idx, sigs, scalars=scalars, raw=True)
    LL = dict(L, scalars=scalars)
    ok, p = both_modes(dev, LL, a, [], [s0 + 40], identity_subs={(s0, 2)})
    assert np.nonzero(~ok)[0].tolist() == [s0 + 40]
    assert ok[s0 + 16:s0 + 24].all()
    assert p == {"mode": 1, "segments": 1, "subs": 8, "subs_failed": 2, "leaves": 16, "pairs": 2 * 7 + 32, "hashes": 0}


def faulted(L):
    """32 of 640 sets (5 %) faulted, the ten kinds of test_gpu_same_message.faulted; the group of two is all bad"""
    rng = np.random.default_rng(29)
    idx, sigs, sig_len = L["idx"].copy(), L["sigs"].copy(), np.full(L["n"], 96, np.uint32)
    off = L["off"]
    where = [int(off[G2]), int(off[G2]) + 1]
    for g, count in ((4, 5), (6, 6), (G300, 19)):
        where += [int(off[g]) + int(x) for x in rng.choice(SIZES[g], size=count, replace=False)]
    kinds = {}
    for k, i in enumerate(where):
        kind = "wrong_message" if k < 2 else SM.KINDS[k % len(SM.KINDS)]
        kinds[i] = kind
        if kind == "wrong_message":
            sigs[i] = L["wrong"][i]
        elif kind == "other_validator":
            j = i + 1 if i + 1 < L["n"] and L["group"][i + 1] == L["group"][i] else i - 1
            assert L["idx"][j] != L["idx"][i]
            sigs[i] = L["sigs"][j]  # a valid signature of another validator over the same root
        elif kind == "flag_byte":
            sigs[i, 0] &= 0x7F
        elif kind == "x_ge_p":
            sigs[i, :96] = np.frombuffer(bytes([0x9F]) + b"\xff" * 95, np.uint8)
        elif kind == "not_on_curve":
            sigs[i, :96] = np.frombuffer(SM.not_on_curve_signature(rng), np.uint8)
        elif kind == "length_32":
            sig_len[i] = 32
        elif kind == "not_in_g2":
            sigs[i, :96] = np.frombuffer(SM.not_in_g2_signature(rng), np.uint8)
        elif kind == "identity_sig":
            sigs[i, :96] = np.frombuffer(bytes([0xC0]) + bytes(95), np.uint8)
        elif kind == "index_past_table":
            idx[i] = N_KEYS + 2 + k
        elif kind == "identity_row":
            idx[i] = INF_ROW
    return idx, sigs, sig_len, kinds


def test_ten_fault_kinds_at_five_percent(dev, layout):
    L = layout
    idx, sigs, sig_len, kinds = faulted(L)
    assert set(kinds.values()) == set(SM.KINDS) and len(kinds) == 32
    bad = [i for i, k in kinds.items() if k in PAIRING_KINDS]
    skip = [i for i, k in kinds.items() if k not in PAIRING_KINDS]
    a = sm_arrays(L, idx, sigs, sig_len)
    ok, p = both_modes(dev, L, a, skip, bad)
    _, code, st, _ = run(dev, 1, a)
    assert {int(c) for c in code[sorted(kinds)]} >= {0, 1, 2, 3, 5, 6, 8, 9}
    assert p["hashes"] == 0 and p["leaves"] > 0 and p["subs_failed"] < p["subs"]
    assert p["pairs"] < 2 * st["sets_retried"]  # fewer pairs than mode 0's retry
    assert st["groups_retried"] >= 3  # the group of two, and the groups of 65 and 300 hold pairing faults


# ------------------------------------------------------------ the other three entries
def test_aggregate_outputs_are_byte_equal(dev, layout):
    """bgv_verify_same_message_aggregate with take and prev set: the second pass runs over the final verdicts"""
    L = layout
    rng = np.random.default_rng(31)
    off = L["off"]
    bad = [int(off[G2]), int(off[G64]) + 7, int(off[G64]) + 8, int(off[G300]) + 100, int(off[G300]) + 299]
    sigs = with_wrong(L, bad)
    sigs[int(off[G300]) + 70, 0] &= 0x7F
    a = sm_arrays(L, sigs=sigs)
    take = (rng.random(L["n"]) < 0.8).astype(np.uint8)
    take[bad[1]] = 1
    prev = np.zeros((len(SIZES), 96), np.uint8)
    prev[:, 0] = 0xC0  # none
    for g in (G2, G64, G300):
        prev[g] = L["sigs"][int(off[g]) + 1, :96]  # any point of G2 will do as a running aggregate
    outs, paths = {}, {}
    for mode in (0, 1, 0):
        dev.sm_retry(mode)
        try:
            outs[mode] = dev.verify_same_message_aggregate(a, take=take, prev=prev)
            paths[mode] = dev.sm_retry_stats()
        finally:
            dev.sm_retry(0)
        assert paths[mode]["mode"] == mode
    o0, o1, path = outs[0], outs[1], paths[1]
    want_ok, want_code = yardstick(dev, L, a)
    assert (o1["set_valid"] == want_ok).all() and (o1["set_code"] == want_code).all()
    assert (o0["set_valid"] == want_ok).all() and (o0["set_code"] == want_code).all()
    assert {k: o1["stats"][k] for k in STAT_KEYS} == {k: o0["stats"][k] for k in STAT_KEYS}
    assert o1["agg_sig"].tobytes() == o0["agg_sig"].tobytes()
    assert o1["agg_count"].tolist() == o0["agg_count"].tolist()
    assert o1["agg_code"].tolist() == o0["agg_code"].tolist()
    want_count = [int((want_ok & (take != 0))[int(off[g]):int(off[g + 1])].sum()) for g in range(len(SIZES))]
    assert o1["agg_count"].tolist() == want_count
    assert path == want_path(off, [int(off[G300]) + 70], bad)


def test_aggregate_sets(dev):
    """bgv_verify_same_message_agg: sets of one to three keys in groups of 9, 64 and 65"""
    rng = np.random.default_rng(37)
    sizes = [9, 64, 65]
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    keys = [[int(x) for x in rng.integers(0, N_KEYS, size=int(rng.integers(1, 4)))] for _ in range(n)]
    group = np.repeat(np.arange(3), sizes)
    msgs = np.stack([np.frombuffer(msg_of(100 + g), np.uint8) for g in range(3)])
    sigs = SMA.sign(dev, keys, msgs[group])
    wrong = SMA.sign(dev, keys, np.stack([np.frombuffer(msg_of(199), np.uint8)] * n))
    bad = [8, 9 + 7, 9 + 8, 9 + 40, 73 + 64]
    sigs[bad] = wrong[bad]
    sigs[9 + 3, 0] &= 0x7F            # rejected before aggregation, in front of the faults of its segment
    keys[9 + 5] = [3, N_KEYS + 9]     # an index past the table
    skip = [9 + 3, 9 + 5]
    po, idx = SMA.flatten(keys)
    scalars = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    a = {"n_sets": n, "n_groups": 3, "group_offsets": off, "pk_offsets": po, "pk_indices": idx, "msgs": msgs, "sigs": sigs,
         "sig_len": np.full(n, 96, np.uint32), "scalars": scalars}
    jobs = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po, "pk_indices": idx,
            "msgs": np.ascontiguousarray(msgs[group]), "sigs": sigs, "sig_len": a["sig_len"], "scalars": scalars}
    jr, sc = dev.verify(jobs)
    ok0, code0, st0, p0 = run(dev, 0, a, "verify_same_message_agg")
    ok1, code1, st1, p1 = run(dev, 1, a, "verify_same_message_agg")
    print("agg stats:", st1, "retry 0:", p0, "retry 1:", p1)
    assert (ok0 == (jr == 1)).all() and (code0 == sc).all()
    assert (ok1 == (jr == 1)).all() and (code1 == sc).all()
    assert np.nonzero(~ok1)[0].tolist() == sorted(bad + skip)
    assert st1 == st0
    assert p1 == want_path(off, skip, bad)
    assert p1["subs"] == 2 + 8 + 1 and p1["hashes"] == 0 and p1["pairs"] < p0["pairs"]


@pytest.mark.parametrize("sums", [True, False], ids=["with_sums", "without_sums"])
def test_bitfield_sets(sums):
    """bgv_verify_same_message_bits: 128-member windows with one or two members absent (the complement
    path on the context with sums), groups of 3 and 70"""
    from tests.test_gpu_bits import Builder
    from tests.test_gpu_bits_sums import L_PERM, build_lists, open_device
    from tests import test_gpu_same_message_bits as SMB
    lists = build_lists()
    d = open_device(lists, sums)
    try:
        row_sk = [cref.device_sk(SMB.SEED, i) for i in range(SMB.N_KEYS)]
        rng = np.random.default_rng(41)
        b = Builder()
        for i in range(73):
            bits = np.ones(128, bool)
            bits[rng.permutation(128)[:1 + i % 2]] = False
            b.committee(L_PERM, 57 * i, bits)
        a, keys = SMB.finish(b, [3, 70], lists, row_sk, d, rng, tag=300)
        a["sigs"] = a["sigs"].copy()
        bad = [1, 3 + 7, 3 + 8, 3 + 64 + 5]
        for i in bad:
            a["sigs"][i, :96] = np.frombuffer(cref.sign(SMB.set_sk(keys[i], row_sk), SMB.msg_of(999)), np.uint8)
        a["sigs"][3 + 2, 0] &= 0x7F
        skip = [3 + 2]
        e = SMB.expansion(a, lists)
        n = a["n_sets"]
        group = np.repeat(np.arange(2), [3, 70])
        jobs = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": e["pk_offsets"],
                "pk_indices": e["pk_indices"], "raw_pks": a["raw_pks"], "n_raw": a["n_raw"],
                "msgs": np.ascontiguousarray(a["msgs"][group]), "sigs": a["sigs"], "sig_len": a["sig_len"], "scalars": a["scalars"]}
        jr, sc = d.verify(jobs)
        ok0, code0, st0, p0 = run(d, 0, a, "verify_same_message_bits")
        ok1, code1, st1, p1 = run(d, 1, a, "verify_same_message_bits")
        print("bits stats:", st1, "retry 0:", p0, "retry 1:", p1, d.bits_path_stats())
        assert (ok0 == (jr == 1)).all() and (code0 == sc).all()
        assert (ok1 == (jr == 1)).all() and (code1 == sc).all()
        assert np.nonzero(~ok1)[0].tolist() == sorted(bad + skip)
        assert st1 == st0
        assert p1 == want_path(a["group_offsets"], skip, bad)
        assert (d.bits_path_stats()["sets_complement"] > 0) == sums
    finally:
        d.close()


# ------------------------------------------------------------ resident inputs, drawn scalars, switching
def test_on_device_batch_with_library_drawn_scalars(dev, layout):
    import torch
    import bench
    L = layout
    off = L["off"]
    bad = [int(off[G9]) + 4, int(off[G300]) + 77, int(off[G300]) + 78, int(off[G300]) + 250]
    a = sm_arrays(L, sigs=with_wrong(L, bad), scalars=None)
    want_ok, want_code = yardstick(dev, L, a)
    assert np.nonzero(~want_ok)[0].tolist() == bad
    da = bench.to_device(a, torch, torch.device("cuda", 0))
    for _ in range(2):  # two draws
        ok, code, st, p = run(dev, 1, da, on_device=True)
        assert (ok == want_ok).all() and (code == want_code).all()
        assert p == want_path(off, [], bad)
    ok, code, st, p = run(dev, 1, a)  # the host batch, drawn scalars
    assert (ok == want_ok).all() and (code == want_code).all()


def test_switching_modes_between_calls(dev, layout):
    L = layout
    bad = int(L["off"][G64]) + 50
    a = sm_arrays(L, sigs=with_wrong(L, [bad]))
    seen = []
    for mode in (1, 0, 1):
        dev.sm_retry(mode)
        ok, _ = dev.verify_same_message(a)
        assert np.nonzero(~ok)[0].tolist() == [bad]
        seen.append(dev.sm_retry_stats())
    dev.sm_retry(0)
    assert [p["mode"] for p in seen] == [1, 0, 1]
    assert seen[0] == seen[2] == {"mode": 1, "segments": 1, "subs": 8, "subs_failed": 1, "leaves": 8, "pairs": 32, "hashes": 0}
    assert seen[1] == {"mode": 0, "segments": 1, "subs": 0, "subs_failed": 0, "leaves": 64, "pairs": 128, "hashes": 64}
    ok, _ = dev.verify_same_message(sm_arrays(L))  # a clean call forgets the last retry
    assert ok.all() and dev.sm_retry_stats() == dict(ZERO_PATH, mode=0)
