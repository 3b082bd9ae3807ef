"""Host logic of verify_and_aggregate_same_message (lodestar_amd/verifier.py)
against a fake device: an aggregate call always forms its own group, plain
calls still share one, take and previous reach the right sets and groups, and
a `previous` that does not decode rejects its call alone."""
import asyncio

import numpy as np
import pytest

from lodestar_amd import verifier as V

IDENTITY = bytes([0xC0]) + bytes(95)
BAD_PREV = bytes([0x9F]) + b"\xff" * 95


def _pk(i):
    return V.PublicKey(index=i)


def _sig(good, tag=0):
    return (b"ok" if good else b"no") + bytes([tag]) + bytes(93)


class FakeDevice:
    """a set is valid iff its signature starts with b"ok"; a group's aggregate is
    its prev's first byte, then the third bytes of the valid, taken signatures"""

    def __init__(self):
        self.calls = []

    def verify_same_message(self, arrays):
        self.calls.append(("plain", arrays))
        n = arrays["n_sets"]
        return np.array([arrays["sigs"][i, :2].tobytes() == b"ok" for i in range(n)], bool), np.zeros(n, np.int32)

    def verify_same_message_aggregate(self, arrays, take=None, prev=None):
        self.calls.append(("agg", arrays, take.copy(), prev.copy()))
        n, G, off = arrays["n_sets"], arrays["n_groups"], arrays["group_offsets"]
        ok = np.array([arrays["sigs"][i, :2].tobytes() == b"ok" for i in range(n)], bool)
        sig = np.zeros((G, 96), np.uint8)
        cnt, code = np.zeros(G, np.uint32), np.zeros(G, np.int32)
        for g in range(G):
            bad = prev[g].tobytes() == BAD_PREV
            code[g] = 1 if bad else 0
            tags = [int(arrays["sigs"][i, 2]) for i in range(off[g], off[g + 1]) if ok[i] and take[i]]
            body = ([] if bad else [int(prev[g, 0])]) + tags
            sig[g, :len(body)] = body
            cnt[g] = len(tags)
        return {"set_valid": ok, "set_code": np.zeros(n, np.int32), "agg_sig": sig, "agg_count": cnt, "agg_code": code}


def test_merge_rule_aggregate_calls_are_never_fused():
    m1, m2 = b"\x01" * 32, b"\x02" * 32
    agg = V.AggregateRequest()
    calls = [([(_pk(0), b"a")], m1), ([(_pk(1), b"b")], m1, agg), ([(_pk(2), b"c")], m1, agg), ([(_pk(3), b"d")], m1),
             ([(_pk(4), b"e")], m2, None)]
    groups, where, group_of = V.merge_same_message_groups(calls)
    assert [g[0] for g in groups] == [m1, m1, m1, m2]
    assert [[pk.index for pk, _ in g[1]] for g in groups] == [[0, 3], [1], [2], [4]]
    assert group_of == [0, 1, 2, 0, 3]
    flat = [pk.index for g in groups for pk, _ in g[1]]
    assert [flat[w] for w in where] == [[0], [1], [2], [3], [4]]
    # without aggregate calls: the rule of merge_same_message, unchanged
    assert V.merge_same_message(calls[:1] + calls[3:]) == V.merge_same_message_groups(calls[:1] + calls[3:])[:2]


def test_three_calls_in_one_flush_keep_their_own_results():
    dev = FakeDevice()
    metrics = {}

    async def main():
        q = V.SameMessageQueue(lambda calls: V.run_same_message_calls(dev, calls, None, metrics))
        m = b"\x07" * 32
        a = [(_pk(i), _sig(True, 10 + i)) for i in range(3)]
        b = [(_pk(10), _sig(True, 20)), (_pk(11), _sig(False, 21)), (_pk(12), _sig(True, 22))]
        c = [(_pk(20), _sig(True, 30)), (_pk(21), _sig(False, 31))]
        prev_b = bytes([0x85]) + bytes(95)
        ra, rb, rc = await asyncio.gather(
            q.submit(a, m, True, V.AggregateRequest()),
            q.submit(b, m, True, V.AggregateRequest(previous=prev_b, take=(True, True, False))),
            q.submit(c, m, True))
        assert len(dev.calls) == 1 and dev.calls[0][0] == "agg"
        _, arrays, take, prev = dev.calls[0]
        assert arrays["n_groups"] == 3 and arrays["group_offsets"].tolist() == [0, 3, 6, 8]
        assert take.tolist() == [1, 1, 1, 1, 1, 0, 0, 0]  # the plain call adds nothing to an aggregate
        assert prev[0].tobytes() == IDENTITY and prev[1].tobytes() == prev_b and prev[2].tobytes() == IDENTITY
        assert ra.valid == [True] * 3 and ra.count == 3 and ra.aggregate[:4] == bytes([0xC0, 10, 11, 12])
        assert rb.valid == [True, False, True] and rb.count == 1 and rb.aggregate[:3] == bytes([0x85, 20, 0])
        assert rc == [True, False]
        # a previous that does not decode rejects that call alone
        r = await asyncio.gather(q.submit(a, m, True, V.AggregateRequest(previous=BAD_PREV)),
                                 q.submit(b, m, True, V.AggregateRequest()), q.submit(c, m, True), return_exceptions=True)
        assert isinstance(r[0], V.BlsError) and r[0].message == "BLST_ERROR: BLST_BAD_ENCODING" and r[0].code == 1
        assert r[1].valid == [True, False, True] and r[1].count == 2
        assert r[2] == [True, False]
        # only plain calls: the plain entry, as before
        assert await q.submit(c, m, False) == [True, False]
        assert dev.calls[-1][0] == "plain"

    asyncio.run(main())
    assert metrics["same_message_aggregated_sigs"] == 3 + 1 + 2
    assert metrics["same_message_sets_started"] == 8 + 8 + 2


def test_argument_checks_and_the_empty_call():
    s = object.__new__(V.BlsGpuSingleThreadVerifier)  # no device: none of these reaches one
    s._closed = False
    m = b"\x00" * 32
    r = asyncio.run(s.verify_and_aggregate_same_message([], m))
    assert r.valid == [] and r.aggregate == IDENTITY and r.count == 0
    prev = bytes([0x85]) + bytes(95)
    assert asyncio.run(s.verify_and_aggregate_same_message([], m, previous=prev)).aggregate == prev
    with pytest.raises(V.BlsError):
        asyncio.run(s.verify_and_aggregate_same_message([(_pk(1), b"")], m, previous=bytes(95)))
    with pytest.raises(V.BlsError):
        asyncio.run(s.verify_and_aggregate_same_message([(_pk(1), b"")], m, take=[True, False]))
    v = object.__new__(V.BlsGpuVerifier)
    v._closed = False
    assert asyncio.run(v.verify_and_aggregate_same_message([], m)).count == 0
