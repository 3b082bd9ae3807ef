"""The weighted G1 sum of same-message verification (lodestar_amd/csrc/
msm_g1.h) compiled for the host and compared, byte for byte, with the Python
oracle (E1.mul / E1.add), plus the host logic of the verifier's
same-message entry: encoding, merging, buffering (against a fake device)."""
import asyncio
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as B
from lodestar_amd import verifier as V

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_sm.cpp")
LIB = os.path.join(HERE, "native", "libhostcheck_sm.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")


@pytest.fixture(scope="module")
def hc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.hc_sm_seg_max.restype = ctypes.c_uint32
    lib.hc_sm_g1_segment.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.hc_sm_bucket_pair.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def keys():
    pks = json.load(open(os.path.join(HERE, "golden", "interop-pubkeys.json")))
    out = []
    for p in pks:
        code, pt = B.g1_decompress(bytes.fromhex(p[2:]))
        assert code == 0
        out.append(pt)
    return out


def g1_b(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def oracle_sum(rows, scalars, skip=None):
    acc = None
    for i, (p, k) in enumerate(zip(rows, scalars)):
        if skip is not None and skip[i]:
            continue
        acc = B.E1.add(acc, B.E1.mul(p, int(k)))
    return acc


def device_sum(hc, rows, scalars, skip=None):
    n = len(rows)
    sc = np.array(list(scalars) or [1], np.uint64)
    sk = np.array(list(skip) or [0], np.uint32) if skip is not None else None
    out = ctypes.create_string_buffer(96)
    finite = hc.hc_sm_g1_segment(b"".join(g1_b(p) for p in rows) or bytes(96), sc.ctypes.data,
                                 sk.ctypes.data if sk is not None else None, n, out)
    return finite, out.raw


EDGE_SCALARS = [1, 2**64 - 1, 0x1000000000000000, 0xF]


def test_segment_maximum_is_recorded(hc):
    assert hc.hc_sm_seg_max() == 64


def test_segment_sizes_against_the_oracle(hc, keys):
    seg = hc.hc_sm_seg_max()
    rng = np.random.default_rng(11)
    for n in (1, 2, 15, 16, 17, seg, seg + 1):
        rows = [keys[(3 * i + n) % len(keys)] for i in range(n)]
        scalars = [int(x) for x in rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)]
        for k, e in enumerate(EDGE_SCALARS):  # the edge scalars ride along in every size they fit
            if k < n:
                scalars[k] = e
        finite, got = device_sum(hc, rows, scalars)
        assert finite == 1
        assert got == g1_b(oracle_sum(rows, scalars)), n


@pytest.mark.parametrize("scalar", EDGE_SCALARS + [0xDEADBEEFCAFEF00D])
def test_all_equal_scalars(hc, keys, scalar):
    rows = keys[:17]
    finite, got = device_sum(hc, rows, [scalar] * 17)
    assert finite == 1 and got == g1_b(oracle_sum(rows, [scalar] * 17))


def test_same_key_twice_doubles_in_the_bucket(hc, keys):
    p = keys[5]
    out = ctypes.create_string_buffer(96)
    assert hc.hc_sm_bucket_pair(g1_b(p), g1_b(p), out) == 1
    assert out.raw == g1_b(B.E1.dbl(p))
    for k in (1, 0xF, 0x1234567890ABCDEF):
        rows, scalars = [keys[1], p, keys[2], p], [7, k, 9, k]
        finite, got = device_sum(hc, rows, scalars)
        assert finite == 1 and got == g1_b(oracle_sum(rows, scalars))


def test_key_and_its_negation_sum_to_the_identity(hc, keys):
    p = keys[24]
    out = ctypes.create_string_buffer(96)
    assert hc.hc_sm_bucket_pair(g1_b(p), g1_b(B.E1.neg(p)), out) == 0
    assert out.raw == bytes(96)
    finite, got = device_sum(hc, [p, B.E1.neg(p)], [0xABCDEF0123456789] * 2)
    assert finite == 0 and got == bytes(96)
    # beside other rows the pair cancels and the rest remains
    rows, scalars = [p, keys[3], B.E1.neg(p)], [0x55, 0x1F, 0x55]
    finite, got = device_sum(hc, rows, scalars)
    assert finite == 1 and got == g1_b(B.E1.mul(keys[3], 0x1F))


def test_identity_row_and_skipped_rows_add_nothing(hc, keys):
    rows, scalars = [keys[0], None, keys[1]], [3, 0xFFFFFFFFFFFFFFFF, 5]
    finite, got = device_sum(hc, rows, scalars)
    assert finite == 1 and got == g1_b(oracle_sum([keys[0], keys[1]], [3, 5]))
    finite, got = device_sum(hc, [None], [9])
    assert finite == 0 and got == bytes(96)
    rows, scalars, skip = keys[:5], [2, 3, 4, 5, 6], [0, 1, 0, 0, 1]
    finite, got = device_sum(hc, rows, scalars, skip)
    assert finite == 1 and got == g1_b(oracle_sum(rows, scalars, skip))


# ------------------------------------------------------------ host logic
def _pk(i):
    return V.PublicKey(index=i)


def test_encode_same_message_offsets_and_shapes():
    raw = bytes(range(96))
    groups = [(b"\x01" * 32, [(_pk(3), b"\xaa" * 96), (_pk(4), b"\xbb" * 192)]),
              (b"\x02" * 32, [(V.PublicKey(raw=raw), b"\xcc" * 96), (V.PublicKey(raw=raw), b"\xdd" * 7), (_pk(9), b"\xee" * 96)])]
    a = V.encode_same_message(groups, np.arange(1, 6, dtype=np.uint64))
    assert a["n_sets"] == 5 and a["n_groups"] == 2
    assert a["group_offsets"].dtype == np.uint32 and a["group_offsets"].tolist() == [0, 2, 5]
    assert a["pk_indices"].tolist() == [3, 4, 0x80000000, 0x80000000, 9]
    assert a["n_raw"] == 1 and a["raw_pks"].tobytes() == raw
    assert a["msgs"].shape == (2, 32) and a["msgs"][1].tobytes() == b"\x02" * 32
    assert a["sigs"].shape == (5, 192) and a["sig_len"].tolist() == [96, 192, 96, 7, 96]
    assert a["sigs"][1].tobytes() == b"\xbb" * 192 and a["sigs"][3].tobytes() == bytes(192)
    with pytest.raises(V.BlsError):
        V.encode_same_message([(b"\x01" * 32, [])])
    with pytest.raises(V.BlsError):
        V.encode_same_message([(b"\x01" * 31, [(_pk(0), b"\xaa" * 96)])])


def test_merge_rule_one_group_per_call_equal_messages_share():
    m1, m2 = b"\x01" * 32, b"\x02" * 32
    calls = [([(_pk(0), b"a")], m1), ([(_pk(1), b"b"), (_pk(2), b"c")], m2), ([(_pk(3), b"d")], m1)]
    groups, where = V.merge_same_message(calls)
    assert [g[0] for g in groups] == [m1, m2]
    assert [[pk.index for pk, _ in g[1]] for g in groups] == [[0, 3], [1, 2]]
    flat = [pk.index for g in groups for pk, _ in g[1]]
    assert [flat[w] for w in where] == [[0], [1, 2], [3]]


class FakeDevice:
    """Device.verify_same_message: a set is valid iff its signature starts with b"ok" """

    def __init__(self):
        self.calls = []

    def verify_same_message(self, arrays):
        self.calls.append(arrays)
        n = arrays["n_sets"]
        ok = np.array([arrays["sigs"][i, :2].tobytes() == b"ok" for i in range(n)], bool)
        return ok, np.zeros(n, np.int32)


def _sig(good):
    return (b"ok" if good else b"no") + bytes(94)


def test_buffering_and_merge_against_a_fake_device():
    dev = FakeDevice()
    metrics = {}

    async def main():
        q = V.SameMessageQueue(lambda calls: V.run_same_message_calls(dev, calls, None, metrics))
        m1, m2 = b"\x01" * 32, b"\x02" * 32
        a = [(_pk(i), _sig(True)) for i in range(3)]
        b = [(_pk(10), _sig(True)), (_pk(11), _sig(False))]
        c = [(_pk(20), _sig(False))]
        # two batchable calls wait in the buffer; the non-batchable one goes out at once
        t_a = asyncio.ensure_future(q.submit(a, m1, True))
        t_b = asyncio.ensure_future(q.submit(b, m1, True))
        await asyncio.sleep(0)
        assert q.pending_jobs() == 2 and len(dev.calls) == 0
        r_c = await q.submit(c, m2, False)
        assert r_c == [False] and len(dev.calls) == 1 and q.pending_jobs() == 2
        # more than MAX_BUFFERED_SIGS signatures waiting flush the buffer without the timer
        big = [(_pk(100 + i), _sig(i != 7)) for i in range(V.MAX_BUFFERED_SIGS)]
        r_big, r_a, r_b = await asyncio.gather(q.submit(big, m2, True), t_a, t_b)
        assert r_a == [True] * 3 and r_b == [True, False]
        assert r_big == [i != 7 for i in range(V.MAX_BUFFERED_SIGS)]
        assert len(dev.calls) == 2
        merged = dev.calls[1]
        assert merged["n_groups"] == 2 and merged["group_offsets"].tolist() == [0, 5, 5 + V.MAX_BUFFERED_SIGS]
        # a lone batchable call goes out when the timer fires
        r = await q.submit([(_pk(1), _sig(True))], m1, True)
        assert r == [True] and len(dev.calls) == 3
        q.abort()
        with pytest.raises(V.QueueError):
            await q.submit(a, m1, False)

    asyncio.run(main())
    assert metrics["same_message_sets_started"] == 1 + 5 + V.MAX_BUFFERED_SIGS + 1


def test_empty_sets_return_an_empty_list_without_a_device_call():
    v = object.__new__(V.BlsGpuVerifier)  # no device: the empty call must not reach one
    v._closed = False
    assert asyncio.run(v.verify_signature_sets_same_message([], b"\x00" * 32)) == []
    s = object.__new__(V.BlsGpuSingleThreadVerifier)
    s._closed = False
    assert asyncio.run(s.verify_signature_sets_same_message([], b"\x00" * 32)) == []


def test_raw_keys_are_checked_as_check_sets_does():
    with pytest.raises(V.BlsError):
        V.check_same_message([(V.PublicKey(raw=bytes(48)), b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_same_message([(_pk(1 << 31), b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_same_message([(_pk(1), b"")], b"\x00" * 31)
    V.check_same_message([(_pk(1), b""), (V.PublicKey(raw=bytes(96)), b"")], b"\x00" * 32)
