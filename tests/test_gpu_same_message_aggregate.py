"""bgv_verify_same_message_aggregate on the GPU: the per-group aggregate
signatures, byte for byte against the Python oracle (for the synthetic keys
sum sigma_i = (sum sk_i mod r) H(m): one multiplication per group), with the
verdicts, codes and counters of bgv_verify_same_message on the same arrays.
The batch, its group sizes and its faults are those of
tests/test_gpu_same_message.py.  Run on an MI355X (-m gpu)."""
import asyncio

import numpy as np
import pytest

from oracle import bls12_381 as B
from oracle import cref
from tests import test_gpu_same_message as T
from tests.test_gpu_same_message import dev, layout  # noqa: F401  (module-scoped fixtures, one device for this module)

pytestmark = pytest.mark.gpu

SEED, N_KEYS, SIZES, SEG = T.SEED, T.N_KEYS, T.SIZES, T.SEG
G = len(SIZES)
IDENTITY = bytes([0xC0]) + bytes(95)
# fault kinds that are rejected before aggregation (k_sm_classify): no set of them reaches the retry
FIRST_PASS_KINDS = ["flag_byte", "x_ge_p", "not_on_curve", "length_32", "not_in_g2", "identity_sig", "index_past_table",
                    "identity_row"]


class Oracle:
    """compress(k H(m_g)), one oracle multiplication per distinct (group, k); computed once, shared"""

    def __init__(self):
        self.hm = [B.hash_to_g2(T.msg_of(g)) for g in range(G)]
        self.cache = {}

    def point(self, g, k):
        k %= B.R
        if (g, k) not in self.cache:
            self.cache[(g, k)] = IDENTITY if k == 0 else B.g2_compress(B.E2.mul(self.hm[g], k))
        return self.cache[(g, k)]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def sk_sums(L, idx, include):
    """per group: (sum of the secret keys of the included sets mod r, how many)"""
    out = []
    for g in range(G):
        members = [i for i in range(int(L["off"][g]), int(L["off"][g + 1])) if include[i]]
        out.append((sum(cref.device_sk(SEED, int(idx[i])) for i in members) % B.R, len(members)))
    return out


def check_aggregates(out, oracle, L, idx, include, prev_k=None, alone=()):
    """agg_sig / agg_count of every group against the oracle; prev_k[g]: the running aggregate is prev_k[g] H(m_g);
    alone: groups whose prev did not decode"""
    for g, (k, count) in enumerate(sk_sums(L, idx, include)):
        kp = 0 if prev_k is None or g in alone else prev_k[g]
        print("group", g, "count", int(out["agg_count"][g]), "want", count, "code", int(out["agg_code"][g]))
        assert out["agg_count"][g] == count, g
        assert out["agg_sig"][g].tobytes() == oracle.point(g, k + kp), g


def same_verdicts(dev, out, arrays):
    ok, code = dev.verify_same_message(arrays)
    st = dev.last_sm_stats.as_dict()
    assert (out["set_valid"] == ok).all() and (out["set_code"] == code).all()
    assert {k: v for k, v in out["stats"].items() if k != "total_ms"} == {k: v for k, v in st.items() if k != "total_ms"}


def boundary_take(L):
    """drops sets on both sides of a segment boundary in the groups of 65, 128 and 300, and the whole group of two"""
    off = L["off"]
    take = np.ones(L["n"], np.uint8)
    for g in (4, 5, 6):
        take[int(off[g]) + SEG - 1] = take[int(off[g]) + SEG] = 0
    take[int(off[6]) + 2 * SEG - 1] = take[int(off[6]) + 2 * SEG] = take[int(off[6]) + 299] = 0
    take[int(off[1]):int(off[2])] = 0
    return take


PREV_K = [0x1111, 0, 0xABCDEF0123456789ABCDEF, 0, None, 0x5, 0x77]  # group 4: minus the new sum (below)
X_GE_P = bytes([0x9F]) + b"\xff" * 95


def make_prev(oracle, L, idx, include, bad_group=6):
    """running aggregates: present for groups 0, 2, 5, the identity for 1 and 3, minus the new sum for group 4,
    one that does not decode (x >= p) for `bad_group`"""
    sums = sk_sums(L, idx, include)
    prev_k = list(PREV_K)
    prev_k[4] = (-sums[4][0]) % B.R
    prev = np.stack([np.frombuffer(oracle.point(g, prev_k[g]), np.uint8) for g in range(G)]).copy()
    prev[bad_group] = np.frombuffer(X_GE_P, np.uint8)
    return prev, prev_k


def test_clean_batch(dev, layout, oracle):
    L = layout
    a = T.sm_arrays(L)
    out = dev.verify_same_message_aggregate(a)
    assert out["set_valid"].all() and (out["set_code"] == 0).all() and (out["agg_code"] == 0).all()
    assert out["stats"]["sets_retried"] == 0
    big = int(L["off"][6])
    assert L["idx"][big + 10] == L["idx"][big + 11]  # one validator twice: equal signatures in one segment
    assert (L["sigs"][big + 10] == L["sigs"][big + 11]).all()
    check_aggregates(out, oracle, L, L["idx"], np.ones(L["n"], bool))
    assert out["agg_count"].tolist() == SIZES
    same_verdicts(dev, out, a)


def test_take(dev, layout, oracle):
    L = layout
    a = T.sm_arrays(L)
    take = boundary_take(L)
    out = dev.verify_same_message_aggregate(a, take=take)
    check_aggregates(out, oracle, L, L["idx"], take.astype(bool))
    assert out["agg_sig"][1].tobytes() == IDENTITY and out["agg_count"][1] == 0
    assert out["set_valid"].all()  # a set that is not taken is verified and reported like any other
    same_verdicts(dev, out, a)


def test_prev(dev, layout, oracle):
    L = layout
    a = T.sm_arrays(L)
    every = np.ones(L["n"], bool)
    prev, prev_k = make_prev(oracle, L, L["idx"], every)
    out = dev.verify_same_message_aggregate(a, prev=prev)
    assert out["agg_code"].tolist() == [0, 0, 0, 0, 0, 0, B.BLST_BAD_ENCODING]
    check_aggregates(out, oracle, L, L["idx"], every, prev_k, alone={6})
    assert out["agg_sig"][4].tobytes() == IDENTITY and out["agg_count"][4] == SIZES[4]
    assert out["agg_count"].tolist() == SIZES  # prev is not counted
    same_verdicts(dev, out, a)
    # a running aggregate that is not on the curve, in another group
    rng = np.random.default_rng(41)
    prev2 = prev.copy()
    prev2[6] = np.frombuffer(oracle.point(6, prev_k[6]), np.uint8)
    prev2[3] = np.frombuffer(T.not_on_curve_signature(rng), np.uint8)
    out = dev.verify_same_message_aggregate(a, prev=prev2)
    assert out["agg_code"].tolist() == [0, 0, 0, B.BLST_POINT_NOT_ON_CURVE, 0, 0, 0]
    check_aggregates(out, oracle, L, L["idx"], every, prev_k, alone={3})


def first_pass_faults(dev, L):
    """the placement of the existing module's faulted(), with the kinds that are rejected before aggregation"""
    rng = np.random.default_rng(23)
    idx, sigs, sig_len = L["idx"].copy(), L["sigs"].copy(), np.full(L["n"], 96, np.uint32)
    off = L["off"]
    where = [int(off[1]), int(off[1]) + 1]
    for g, count in ((2, 5), (4, 6), (6, 19)):
        where += [int(off[g]) + int(x) for x in rng.choice(SIZES[g], size=count, replace=False)]
    kinds = {}
    for k, i in enumerate(where):
        kind = kinds[i] = FIRST_PASS_KINDS[k % len(FIRST_PASS_KINDS)]
        if kind == "flag_byte":
            sigs[i, 0] &= 0x7F
        elif kind == "x_ge_p":
            sigs[i, :96] = np.frombuffer(X_GE_P, np.uint8)
        elif kind == "not_on_curve":
            sigs[i, :96] = np.frombuffer(T.not_on_curve_signature(rng), np.uint8)
        elif kind == "length_32":
            sig_len[i] = 32
        elif kind == "not_in_g2":
            sigs[i, :96] = np.frombuffer(T.not_in_g2_signature(rng), np.uint8)
        elif kind == "identity_sig":
            sigs[i, :96] = np.frombuffer(IDENTITY, np.uint8)
        elif kind == "index_past_table":
            idx[i] = N_KEYS + 2 + k
        elif kind == "identity_row":
            idx[i] = N_KEYS + 1
    return idx, sigs, sig_len, kinds


def test_first_pass_rejects_are_absent_and_the_speculative_sum_stands(dev, layout, oracle):
    L = layout
    idx, sigs, sig_len, kinds = first_pass_faults(dev, L)
    assert set(kinds.values()) == set(FIRST_PASS_KINDS)
    a = T.sm_arrays(L, idx, sigs, sig_len)
    out = dev.verify_same_message_aggregate(a)
    print("stats:", out["stats"])
    assert out["stats"]["sets_retried"] == 0 and out["stats"]["groups_retried"] == 0  # no second pass ran
    good = np.ones(L["n"], bool)
    good[sorted(kinds)] = False
    assert (out["set_valid"] == good).all()
    assert (out["set_code"][sorted(kinds)] != 0).all()
    check_aggregates(out, oracle, L, idx, good)
    assert out["agg_sig"][1].tobytes() == IDENTITY and out["agg_count"][1] == 0  # the group of two: entirely bad
    same_verdicts(dev, out, a)


@pytest.fixture(scope="module")
def retry_faults(dev, layout):
    """the existing module's faults (left unchanged): every kind, wrong-message and other-validator signatures included"""
    return T.faulted(dev, layout)


def test_faults_that_reach_the_retry(dev, layout, oracle, retry_faults):
    L = layout
    idx, sigs, sig_len, kinds = retry_faults
    retried = [i for i, k in kinds.items() if k in ("wrong_message", "other_validator")]
    assert {int(L["group"][i]) for i in retried} >= {1, 4, 6}  # the group of two, the 65 and the 300 group
    a = T.sm_arrays(L, idx, sigs, sig_len)
    out = dev.verify_same_message_aggregate(a)
    print("stats:", out["stats"])
    assert out["stats"]["sets_retried"] > 0
    good = np.ones(L["n"], bool)
    good[sorted(kinds)] = False
    assert (out["set_valid"] == good).all()
    check_aggregates(out, oracle, L, idx, good)  # exactly the sets with set_valid = 1
    assert out["agg_sig"][1].tobytes() == IDENTITY and out["agg_count"][1] == 0  # every set of the group failed
    same_verdicts(dev, out, a)
    # take and prev through both passes
    take = boundary_take(L)
    inn = good & take.astype(bool)
    prev, prev_k = make_prev(oracle, L, idx, inn)
    out2 = dev.verify_same_message_aggregate(a, take=take, prev=prev)
    assert out2["stats"]["sets_retried"] > 0
    assert out2["agg_code"].tolist() == [0, 0, 0, 0, 0, 0, B.BLST_BAD_ENCODING]
    check_aggregates(out2, oracle, L, idx, inn, prev_k, alone={6})
    assert out2["agg_sig"][4].tobytes() == IDENTITY
    assert (out2["set_valid"] == good).all() and (out2["set_code"] == out["set_code"]).all()


def test_resident_batch(dev, layout, oracle, retry_faults):
    import torch
    import bench
    L = layout
    device = torch.device("cuda", 0)
    take = boundary_take(L)
    idx, sigs, sig_len, kinds = retry_faults
    good = np.ones(L["n"], bool)
    good[sorted(kinds)] = False
    for a, include, retried in ((T.sm_arrays(L), take.astype(bool), False),
                                (T.sm_arrays(L, idx, sigs, sig_len), good & take.astype(bool), True)):
        prev, prev_k = make_prev(oracle, L, a["pk_indices"], include)
        host = dev.verify_same_message_aggregate(a, take=take, prev=prev)
        res = dev.verify_same_message_aggregate(bench.to_device(a, torch, device), take=torch.from_numpy(take).to(device),
                                                prev=torch.from_numpy(prev).to(device), on_device=True)
        for k in ("set_valid", "set_code", "agg_sig", "agg_count", "agg_code"):
            assert (host[k] == res[k]).all(), k
        assert host["stats"]["sets_retried"] == res["stats"]["sets_retried"]
        assert (res["stats"]["sets_retried"] > 0) == retried
        check_aggregates(res, oracle, L, a["pk_indices"], include, prev_k, alone={6})
    # and without take and prev
    a = T.sm_arrays(L)
    res = dev.verify_same_message_aggregate(bench.to_device(a, torch, device), on_device=True)
    check_aggregates(res, oracle, L, L["idx"], np.ones(L["n"], bool))


def test_library_drawn_scalars(dev, layout, oracle):
    L = layout
    ref = dev.verify_same_message_aggregate(T.sm_arrays(L))
    for _ in range(2):
        out = dev.verify_same_message_aggregate(T.sm_arrays(L, scalars=None))
        assert out["set_valid"].all() and out["stats"]["sets_retried"] == 0
        assert (out["agg_sig"] == ref["agg_sig"]).all() and (out["agg_count"] == ref["agg_count"]).all()
    check_aggregates(out, oracle, L, L["idx"], np.ones(L["n"], bool))


def test_uncompressed_input_and_empty_batch(dev, layout, oracle):
    """192-byte signatures are aggregated like compressed ones; n_sets == 0 writes nothing"""
    L = layout
    sigs, sig_len = L["sigs"].copy(), np.full(L["n"], 96, np.uint32)
    for i in range(int(L["off"][3]), int(L["off"][4]), 3):
        code, pt = B.g2_decompress(L["sigs"][i, :96].tobytes())
        assert code == 0
        sigs[i] = np.frombuffer(B.g2_serialize(pt), np.uint8)
        sig_len[i] = 192
    out = dev.verify_same_message_aggregate(T.sm_arrays(L, sigs=sigs, sig_len=sig_len))
    assert out["set_valid"].all()
    check_aggregates(out, oracle, L, L["idx"], np.ones(L["n"], bool))
    empty = {"n_sets": 0, "n_groups": 0, "group_offsets": np.array([0], np.uint32), "pk_indices": np.zeros(1, np.uint32),
             "msgs": np.zeros((1, 32), np.uint8), "sigs": np.zeros((1, 192), np.uint8), "sig_len": np.zeros(1, np.uint32)}
    out = dev.verify_same_message_aggregate(empty)
    assert len(out["set_valid"]) == 0 and len(out["agg_sig"]) == 0


def test_bindings_two_aggregate_calls_and_a_plain_one(oracle):
    """BlsGpuVerifier.verify_and_aggregate_same_message: two concurrent calls with the same message resolve with
    their own aggregates, not the merged one; a plain call in the same flush keeps its result"""
    from lodestar_amd import verifier as V

    async def main():
        v = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1)
        try:
            for d in v._contexts():
                d.gen_keys(0, 64, SEED)
            d0 = v.devices[0]
            m = T.msg_of(0)  # group 0's message: the oracle has H(m)

            def call(idxs):
                sigs = T.sign(d0, np.array(idxs, np.uint32), np.stack([np.frombuffer(m, np.uint8)] * len(idxs)))
                return [(V.PublicKey(index=i), sigs[k, :96].tobytes()) for k, i in enumerate(idxs)]

            def want(idxs, prev_k=0):
                return oracle.point(0, sum(cref.device_sk(SEED, i) for i in idxs) + prev_k)

            ia, ib, ic = list(range(0, 9)), list(range(9, 20)), list(range(20, 25))
            a, b, c = call(ia), call(ib), call(ic)
            b[4] = (b[4][0], b[5][1])  # another validator's signature
            take_b = [k != 2 for k in range(len(ib))]
            opts = V.VerifySignatureOpts(batchable=True)
            ra, rb, rc = await asyncio.gather(
                v.verify_and_aggregate_same_message(a, m, opts),
                v.verify_and_aggregate_same_message(b, m, opts, previous=oracle.point(0, 0x1234), take=take_b),
                v.verify_signature_sets_same_message(c, m, opts))
            assert v._sm.device_calls == 1  # one flush, one merged device call
            assert ra.valid == [True] * 9 and ra.count == 9 and ra.aggregate == want(ia)
            assert rb.valid == [k != 4 for k in range(11)] and rb.count == 9
            assert rb.aggregate == want([i for k, i in enumerate(ib) if k not in (2, 4)], 0x1234)
            assert rc == [True] * 5
            assert v.metrics["same_message_aggregated_sigs"] == 18 and v.metrics["same_message_sets_started"] == 25
            # a previous that does not decode rejects that call alone
            r = await asyncio.gather(v.verify_and_aggregate_same_message(a, m, opts, previous=X_GE_P),
                                     v.verify_and_aggregate_same_message(c, m, opts), return_exceptions=True)
            assert isinstance(r[0], V.BlsError) and r[0].message == "BLST_ERROR: BLST_BAD_ENCODING"
            assert r[1].valid == [True] * 5 and r[1].aggregate == want(ic)
            s = V.BlsGpuSingleThreadVerifier(0)
            try:
                s.device.gen_keys(0, 64, SEED)
                rs = await s.verify_and_aggregate_same_message(b, m, previous=oracle.point(0, 0x1234), take=take_b)
                assert rs.valid == rb.valid and rs.aggregate == rb.aggregate and rs.count == rb.count
            finally:
                await s.close()
        finally:
            await v.close()

    asyncio.run(main())
