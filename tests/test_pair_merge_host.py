"""The pair classes of bgv_pair_merge (lodestar_amd/csrc/pair_merge.h) compiled for
the host and compared with the Python oracle: the class sum over a member list
(sizes, the doubling case, a key beside its negation, identity members, rejected
members, two member orders), the slot mix and the job search."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as B
from tests import hostcheck as H

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_pair_merge.cpp")
LIB = os.path.join(HERE, "native", "libhostcheck_pair_merge.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
K0, KD = 0x2B7E1D5A9F3C, 0x9E3779B97F4A7C15  # point i is (K0 + i KD) G1
N_POINTS = 70
PK_IS_INFINITY, INDEX_RANGE = 6, 9
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def hc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.hc_pm_slot_mix.restype = ctypes.c_uint64
    lib.hc_pm_slot_mix.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    lib.hc_pm_job_of.restype = ctypes.c_uint32
    lib.hc_pm_job_of.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    lib.hc_pm_class_sum.restype = ctypes.c_int32
    lib.hc_pm_class_sum.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                    ctypes.c_char_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def pts():
    """(scalar, point) pairs, left unchanged: point i = (K0 + i KD) G1 by repeated addition"""
    d = B.E1.mul(B.G1, KD)
    out = [(K0, B.E1.mul(B.G1, K0))]
    for i in range(1, N_POINTS):
        out.append((K0 + i * KD, B.E1.add(out[-1][1], d)))
    return out


def g1_b(pt):
    return bytes(96) if pt is None else H.g1_b(pt)


def class_sum(hc, points, order, codes=None):
    """the class whose members are points[order[0]], points[order[1]], ...: (P_c bytes, code, identity flag)"""
    n = len(points)
    cd = np.zeros(max(n, 1), np.int32) if codes is None else np.array(codes, np.int32)
    od = np.array(order, np.uint32)
    out = H.buf(96)
    ident = ctypes.c_uint32(7)
    code = hc.hc_pm_class_sum(b"".join(g1_b(p) for p in points) or bytes(96), cd.ctypes.data, n, od.ctypes.data, len(order),
                              out, ctypes.addressof(ident))
    return out.raw, code, ident.value


def expected(k):
    k %= B.R
    return bytes(96) if k == 0 else H.g1_b(B.E1.mul(B.G1, k))


@pytest.mark.parametrize("m", [1, 2, 3, 64, 65])
def test_class_sizes(hc, pts, m):
    """members spread over a larger batch: every third set from set 2 on while they last, then the rest"""
    points = [p for _, p in pts]
    order = [(2 + 3 * k) % N_POINTS for k in range(min(m, 23))]
    order += [i for i in range(N_POINTS) if i not in order][: m - len(order)]
    assert len(set(order)) == m
    got, code, ident = class_sum(hc, points, order)
    assert (code, ident) == (0, 0)
    assert got == expected(sum(pts[i][0] for i in order))
    if m == 1:
        assert got == H.g1_b(points[order[0]])  # a lone member is copied


def test_equal_key_and_scalar_twice_doubles(hc, pts):
    k, p = pts[5]
    assert class_sum(hc, [p, p], [0, 1]) == (expected(2 * k), 0, 0)
    k2, q = pts[9]
    for order in ([0, 1, 2], [0, 2, 1], [2, 0, 1]):  # the equal pair first, split, last
        assert class_sum(hc, [p, p, q], order) == (expected(2 * k + k2), 0, 0)


def test_key_beside_its_negation_is_the_identity_and_flagged(hc, pts):
    k, p = pts[7]
    got, code, ident = class_sum(hc, [p, B.E1.neg(p)], [0, 1])
    assert got == bytes(96) and ident == 1 and code == PK_IS_INFINITY
    # cancelling inside a larger class is no identity
    k2, q = pts[8]
    assert class_sum(hc, [p, B.E1.neg(p), q], [0, 1, 2]) == (expected(k2), 0, 0)
    assert class_sum(hc, [p, q, B.E1.neg(p)], [0, 1, 2]) == (expected(k2), 0, 0)
    # three members that sum to the identity: (k) + (k2) + (-(k + k2))
    r = B.E1.neg(B.E1.add(p, q))
    got, code, ident = class_sum(hc, [p, q, r], [2, 0, 1])
    assert got == bytes(96) and ident == 1


def test_identity_members_add_nothing(hc, pts):
    (k0, p), (k1, q) = pts[1], pts[2]
    assert class_sum(hc, [None, p, None, q, None], [0, 1, 2, 3, 4]) == (expected(k0 + k1), 0, 0)
    assert class_sum(hc, [p, None], [1, 0]) == (expected(k0), 0, 0)
    got, code, ident = class_sum(hc, [None, None], [0, 1])  # nothing but identities
    assert got == bytes(96) and ident == 1
    got, code, ident = class_sum(hc, [None], [0])
    assert got == bytes(96) and ident == 1


def test_rejected_member_makes_the_class_inert(hc, pts):
    points = [p for _, p in pts[:4]]
    for codes, want in (([0, INDEX_RANGE, 0, 0], INDEX_RANGE), ([PK_IS_INFINITY, 0, INDEX_RANGE, 0], INDEX_RANGE),
                        ([0, 0, 0, PK_IS_INFINITY], PK_IS_INFINITY)):
        for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
            assert class_sum(hc, points, order, codes) == (bytes(96), want, 0)  # no identity flag: the job is rejected
    # a rejected set outside the class does not touch it
    assert class_sum(hc, points, [0, 2], [0, INDEX_RANGE, 0, 0]) == (expected(pts[0][0] + pts[2][0]), 0, 0)


def test_member_order_does_not_change_the_bytes(hc, pts):
    points = [p for _, p in pts]
    rng = np.random.default_rng(11)
    members = rng.choice(N_POINTS, size=40, replace=False).tolist()
    a = class_sum(hc, points, members)
    b = class_sum(hc, points, members[::-1])
    c = class_sum(hc, points, rng.permutation(members).tolist())
    assert a == b == c == (expected(sum(pts[i][0] for i in members)), 0, 0)


def test_a_list_that_loops_ends(hc, pts):
    """next[] is device memory: a walk is bounded by the batch's sets whatever it holds"""
    points = [p for _, p in pts[:3]]
    got, code, ident = class_sum(hc, points, [0, 1, 0])  # 0 -> 1 -> 0 -> ...
    assert code == 0 and len(got) == 96


def mix(job, rep, key):
    h = key ^ ((job << 32) | rep)
    h = (h * 0xff51afd7ed558ccd) & M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 29
    return h


def test_slot_mix(hc):
    rng = np.random.default_rng(12)
    seen = set()
    for _ in range(200):
        job, rep = int(rng.integers(0, 2**32)), int(rng.integers(0, 2**30))
        key = int(rng.integers(0, 2**64, dtype=np.uint64))
        assert hc.hc_pm_slot_mix(job, rep, key) == mix(job, rep, key)
        seen.add(hc.hc_pm_slot_mix(job, rep, key) & 1023)
    assert len(seen) > 150  # the low bits spread
    # the job is part of the key: one representative in two jobs, two slots; and the per-call key moves both
    assert hc.hc_pm_slot_mix(0, 5, 1) != hc.hc_pm_slot_mix(1, 5, 1) != hc.hc_pm_slot_mix(1, 5, 2)
    assert hc.hc_pm_slot_mix(5, 0, 1) != hc.hc_pm_slot_mix(0, 5, 1)


def test_job_of_steps_over_empty_jobs(hc):
    off = np.array([0, 3, 3, 3, 10, 11, 11], np.uint32)  # jobs 1, 2 and 5 are empty
    want = [0, 0, 0, 3, 3, 3, 3, 3, 3, 3, 4]
    assert [hc.hc_pm_job_of(off.ctypes.data, 6, i) for i in range(11)] == want
    one = np.array([0, 4], np.uint32)
    assert [hc.hc_pm_job_of(one.ctypes.data, 1, i) for i in range(4)] == [0] * 4
