"""The weighted G1 sum over aggregated keys (lodestar_amd/csrc/msm_g1.h
msm_g1_segment_jac) compiled for the host and compared, byte for byte, with the
Python oracle, the same header under AddressSanitizer and UBSan in a
stand-alone program, and the host logic of the verifier's entry for aggregate
sets: encoding, merging, buffering (against a fake device)."""
import asyncio
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as B
from lodestar_amd import verifier as V

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_sma.cpp")
LIB = os.path.join(HERE, "native", "libhostcheck_sma.so")
SAN = os.path.join(HERE, "native", "hostcheck_sma_san")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
P = B.P


def _stale(target):
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def hc():
    if _stale(LIB):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.hc_sma_g1_segment.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.hc_sma_sum_rows.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.hc_sma_bucket_pair.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
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


def jac_b(pt, z):
    """the Jacobian representation (x z^2, y z^3, z) of an affine point; the identity has Z = 0"""
    if pt is None:
        return (1).to_bytes(48, "big") * 2 + bytes(48)
    z %= P
    assert z != 0
    return b"".join(v.to_bytes(48, "big") for v in (pt[0] * z * z % P, pt[1] * z * z * z % P, z))


def jac_point(raw144):
    """the affine point of 144 Jacobian bytes"""
    x, y, z = (int.from_bytes(raw144[k:k + 48], "big") for k in (0, 48, 96))
    if z == 0:
        return None
    zi = pow(z, P - 2, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def sum_rows(hc, rows, order):
    """rows summed in `order` by the gather's mixed additions: a Jacobian point whose Z depends on the order"""
    o = np.array(order, np.uint32)
    out = ctypes.create_string_buffer(144)
    hc.hc_sma_sum_rows(b"".join(g1_b(p) for p in rows), o.ctypes.data, len(order), out)
    return out.raw


def oracle_sum(points, scalars, skip=None):
    acc = None
    for i, (p, k) in enumerate(zip(points, scalars)):
        if skip is not None and skip[i]:
            continue
        acc = B.E1.add(acc, B.E1.mul(p, int(k)))
    return acc


def segment(hc, jacs, scalars, skip=None):
    n = len(jacs)
    sc = np.array(list(scalars) or [1], np.uint64)
    sk = np.array(list(skip) or [0], np.uint32) if skip is not None else None
    out = ctypes.create_string_buffer(96)
    finite = hc.hc_sma_g1_segment(b"".join(jacs) or bytes(144), sc.ctypes.data, sk.ctypes.data if sk is not None else None, n, out)
    return finite, out.raw


EDGE_SCALARS = [1, 2**64 - 1, 2**60, 0xF]


def _case(hc, keys, n, seed):
    """n aggregated keys with non-trivial Z: sums of 2..5 rows built by the gather's additions in a shuffled order"""
    rng = np.random.default_rng(seed)
    jacs, points = [], []
    for i in range(n):
        k = int(rng.integers(2, 6))
        rows = [keys[int(j)] for j in rng.choice(len(keys), size=k, replace=False)]
        raw = sum_rows(hc, rows, [int(j) for j in rng.permutation(k)])
        assert raw[96:] != (1).to_bytes(48, "big")  # Z is not 1
        pt = None
        for r in rows:
            pt = B.E1.add(pt, r)
        assert jac_point(raw) == pt
        jacs.append(raw)
        points.append(pt)
    scalars = [int(x) for x in rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)]
    for k, e in enumerate(EDGE_SCALARS):  # the edge scalars ride along in every size they fit
        if k < n:
            scalars[k] = e
    return jacs, points, scalars


@pytest.mark.parametrize("n", [1, 2, 63, 64])
def test_segment_sizes_against_the_oracle(hc, keys, n):
    jacs, points, scalars = _case(hc, keys, n, 100 + n)
    finite, got = segment(hc, jacs, scalars)
    assert finite == 1
    assert got == g1_b(oracle_sum(points, scalars)), n


def test_one_point_in_two_representations_doubles_in_the_bucket(hc, keys):
    rows = keys[3:7]
    a = sum_rows(hc, rows, [0, 1, 2, 3])
    b = sum_rows(hc, rows, [3, 1, 0, 2])
    assert a != b and jac_point(a) == jac_point(b)  # same point, different Jacobian coordinates
    pt = jac_point(a)
    out = ctypes.create_string_buffer(96)
    assert hc.hc_sma_bucket_pair(a, b, out) == 1
    assert out.raw == g1_b(B.E1.dbl(pt))
    c = jac_b(pt, 0x1234567)  # and a third one, rescaled
    for k in EDGE_SCALARS + [0x1234567890ABCDEF]:
        others = [jac_b(keys[1], 7), jac_b(keys[2], 11)]
        jacs, points, scalars = [others[0], a, others[1], b, c], [keys[1], pt, keys[2], pt, pt], [7, k, 9, k, k]
        finite, got = segment(hc, jacs, scalars)
        assert finite == 1 and got == g1_b(oracle_sum(points, scalars)), hex(k)


def test_point_beside_its_negation_is_the_identity(hc, keys):
    rows = keys[8:11]
    a = sum_rows(hc, rows, [0, 1, 2])
    pt = jac_point(a)
    neg = jac_b(B.E1.neg(pt), 0xABCDEF)  # -P in another representation
    out = ctypes.create_string_buffer(96)
    assert hc.hc_sma_bucket_pair(a, neg, out) == 0 and out.raw == bytes(96)
    finite, got = segment(hc, [a, neg], [0xABCDEF0123456789] * 2)
    assert finite == 0 and got == bytes(96)
    # beside other entries the pair cancels and the rest remains
    finite, got = segment(hc, [a, jac_b(keys[3], 5), neg], [0x55, 0x1F, 0x55])
    assert finite == 1 and got == g1_b(B.E1.mul(keys[3], 0x1F))


def test_identity_and_skipped_entries_add_nothing(hc, keys):
    jacs = [jac_b(keys[0], 3), jac_b(None, 1), jac_b(keys[1], 5)]
    finite, got = segment(hc, jacs, [3, 2**64 - 1, 5])
    assert finite == 1 and got == g1_b(oracle_sum([keys[0], keys[1]], [3, 5]))
    finite, got = segment(hc, [jac_b(None, 1)], [9])
    assert finite == 0 and got == bytes(96)
    jacs, points, scalars = _case(hc, keys, 9, 7)
    skip = [0, 1, 0, 0, 1, 0, 0, 0, 1]
    finite, got = segment(hc, jacs, scalars, skip)
    assert finite == 1 and got == g1_b(oracle_sum(points, scalars, skip))
    finite, got = segment(hc, jacs, scalars, [1] * 9)
    assert finite == 0 and got == bytes(96)


def test_stand_alone_program_under_the_sanitizers(hc, keys):
    """the header's code for n = 64 in a program of its own, built with
    -fsanitize=address,undefined (runtimes linked statically): a finding aborts the program"""
    if _stale(SAN):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-DHOSTCHECK_SMA_MAIN", "-o", SAN, SRC])
    jacs, points, scalars = _case(hc, keys, 64, 164)
    skip = [1 if i in (5, 40) else 0 for i in range(64)]
    blob = struct.pack("<I", 64) + b"".join(jacs) + struct.pack("<64Q", *scalars) + struct.pack("<64I", *skip)
    r = subprocess.run([SAN], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    finite, hexout = r.stdout.decode().split()
    assert finite == "1" and bytes.fromhex(hexout) == g1_b(oracle_sum(points, scalars, skip))


# ------------------------------------------------------------ host logic
def _pk(i):
    return V.PublicKey(index=i)


def test_encode_same_message_agg_offsets_and_shapes():
    raw = bytes(range(96))
    groups = [(b"\x01" * 32, [([_pk(3), _pk(7)], b"\xaa" * 96), ([4], b"\xbb" * 192)]),
              (b"\x02" * 32, [([V.PublicKey(raw=raw), _pk(1), V.PublicKey(raw=raw)], b"\xcc" * 96),
                              (np.array([9, 8, 7, 6]), b"\xdd" * 7)])]
    a = V.encode_same_message_agg(groups, np.arange(1, 5, dtype=np.uint64))
    assert a["n_sets"] == 4 and a["n_groups"] == 2
    assert a["group_offsets"].dtype == np.uint32 and a["group_offsets"].tolist() == [0, 2, 4]
    assert a["pk_offsets"].dtype == np.uint32 and a["pk_offsets"].tolist() == [0, 2, 3, 6, 10]
    assert a["pk_indices"].tolist() == [3, 7, 4, 0x80000000, 1, 0x80000000, 9, 8, 7, 6]
    assert a["n_raw"] == 1 and a["raw_pks"].tobytes() == raw
    assert a["msgs"].shape == (2, 32) and a["msgs"][1].tobytes() == b"\x02" * 32
    assert a["sigs"].shape == (4, 192) and a["sig_len"].tolist() == [96, 192, 96, 7]
    assert a["sigs"][1].tobytes() == b"\xbb" * 192 and a["sigs"][3].tobytes() == bytes(192)
    with pytest.raises(V.BlsError):
        V.encode_same_message_agg([(b"\x01" * 32, [])])
    with pytest.raises(V.BlsError):
        V.encode_same_message_agg([(b"\x01" * 32, [([], b"\xaa" * 96)])])
    with pytest.raises(V.BlsError):
        V.encode_same_message_agg([(b"\x01" * 31, [([_pk(0)], b"\xaa" * 96)])])


def test_single_key_sets_encode_as_the_single_key_entry_does():
    groups1 = [(b"\x05" * 32, [(_pk(3), b"\xaa" * 96), (_pk(4), b"\xbb" * 96)]), (b"\x06" * 32, [(_pk(9), b"\xcc" * 96)])]
    groupsA = [(m, [([pk], sig) for pk, sig in sets]) for m, sets in groups1]
    a1, aA = V.encode_same_message(groups1), V.encode_same_message_agg(groupsA)
    assert aA["pk_offsets"].tolist() == [0, 1, 2, 3]
    for k in ("n_sets", "n_groups", "n_raw"):
        assert a1[k] == aA[k]
    for k in ("group_offsets", "pk_indices", "msgs", "sigs", "sig_len"):
        assert np.array_equal(a1[k], aA[k]), k


def test_caller_side_checks():
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([([], b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([([_pk(1), None], b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([([V.PublicKey(raw=bytes(48))], b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([([1 << 31], b"")], b"\x00" * 32)
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([([_pk(1)], b"")], b"\x00" * 31)
    V.check_aggregate_same_message([([_pk(1), 2, V.PublicKey(raw=bytes(96))], b"")], b"\x00" * 32)


class FakeDevice:
    """Device.verify_same_message_agg: a set is valid iff its signature starts with b"ok" """

    def __init__(self):
        self.calls = []

    def verify_same_message_agg(self, arrays):
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
        q = V.SameMessageQueue(lambda calls: V.run_same_message_agg_calls(dev, calls, None, metrics))
        m1, m2 = b"\x01" * 32, b"\x02" * 32
        a = [([i, i + 1], _sig(True)) for i in range(3)]
        b = [([10, 11, 12], _sig(True)), ([_pk(13)], _sig(False))]
        c = [([20, 21], _sig(False))]
        # two batchable calls wait in the buffer; the non-batchable one goes out at once
        t_a = asyncio.ensure_future(q.submit(a, m1, True))
        t_b = asyncio.ensure_future(q.submit(b, m1, True))
        await asyncio.sleep(0)
        assert q.pending_jobs() == 2 and len(dev.calls) == 0
        r_c = await q.submit(c, m2, False)
        assert r_c == [False] and len(dev.calls) == 1 and q.pending_jobs() == 2
        # more than MAX_BUFFERED_SIGS signatures waiting flush the buffer without the timer
        big = [([100 + i, 7], _sig(i != 7)) for i in range(V.MAX_BUFFERED_SIGS)]
        r_big, r_a, r_b = await asyncio.gather(q.submit(big, m2, True), t_a, t_b)
        assert r_a == [True] * 3 and r_b == [True, False]
        assert r_big == [i != 7 for i in range(V.MAX_BUFFERED_SIGS)]
        assert len(dev.calls) == 2
        merged = dev.calls[1]
        assert merged["n_groups"] == 2 and merged["group_offsets"].tolist() == [0, 5, 5 + V.MAX_BUFFERED_SIGS]
        assert merged["pk_offsets"][:6].tolist() == [0, 2, 4, 6, 9, 10]
        assert merged["pk_indices"][:10].tolist() == [0, 1, 1, 2, 2, 3, 10, 11, 12, 13]
        q.abort()
        with pytest.raises(V.QueueError):
            await q.submit(a, m1, False)

    asyncio.run(main())
    assert metrics["same_message_agg_sets_started"] == 1 + 5 + V.MAX_BUFFERED_SIGS
    assert metrics["aggregated_pubkeys_total"] == 2 + 10 + 2 * V.MAX_BUFFERED_SIGS


def test_empty_sets_return_an_empty_list_without_a_device_call():
    v = object.__new__(V.BlsGpuVerifier)  # no device: the empty call must not reach one
    v._closed = False
    assert asyncio.run(v.verify_aggregate_sets_same_message([], b"\x00" * 32)) == []
    s = object.__new__(V.BlsGpuSingleThreadVerifier)
    s._closed = False
    assert asyncio.run(s.verify_aggregate_sets_same_message([], b"\x00" * 32)) == []
