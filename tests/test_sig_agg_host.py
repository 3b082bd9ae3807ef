"""The unweighted per-group signature sums of bgv_verify_same_message_aggregate
(lodestar_amd/csrc/sig_agg.h) compiled for the host and compared, byte for
byte, with the Python oracle: the sixteen sub-lane walks and the tree of one
segment, the group fold with the running aggregate, and the compression."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as B
from tests import hostcheck as H

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_sig_agg.cpp")
LIB = os.path.join(HERE, "native", "libhostcheck_sig_agg.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
IDENTITY = bytes([0xC0]) + bytes(95)
K0, KD = 0x1D5A9F3C2B7E, 0x9E3779B97F4A7C15  # point i is (K0 + i KD) G2
N_POINTS = 160


@pytest.fixture(scope="module")
def hc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.hc_sag_seg_max.restype = ctypes.c_uint32
    lib.hc_sag_lanes.restype = ctypes.c_uint32
    lib.hc_sag_group.restype = ctypes.c_uint32
    lib.hc_sag_group.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def pts():
    """(scalar, point) pairs, left unchanged: point i = (K0 + i KD) G2 by repeated addition"""
    d = B.E2.mul(B.G2, KD)
    out = [(K0, B.E2.mul(B.G2, K0))]
    for i in range(1, N_POINTS):
        out.append((K0 + i * KD, B.E2.add(out[-1][1], d)))
    return out


def run(hc, points, skip=None, take=None, valid=None, prev=None):
    n = len(points)
    sk = np.zeros(max(n, 1), np.uint32) if skip is None else np.array(skip, np.uint32)
    tk = None if take is None else np.array(take, np.uint8)
    va = None if valid is None else np.array(valid, np.uint8)
    out, seg0 = H.buf(96), H.buf(192)
    cnt, code = ctypes.c_uint32(0), ctypes.c_int32(0)
    segs = hc.hc_sag_group(b"".join(H.g2_b(p) for p in points) or bytes(192), n, sk.ctypes.data,
                           None if tk is None else tk.ctypes.data, None if va is None else va.ctypes.data, prev, out,
                           ctypes.addressof(cnt), ctypes.addressof(code), seg0)
    return {"sig": out.raw, "count": cnt.value, "code": code.value, "seg0": seg0.raw, "segs": segs}


def compressed(k):
    k %= B.R
    return IDENTITY if k == 0 else B.g2_compress(B.E2.mul(B.G2, k))


def test_layout_constants(hc):
    assert hc.hc_sag_seg_max() == 64 and hc.hc_sag_lanes() == 16


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64])
def test_segment_sizes(hc, pts, n):
    sel = pts[3:3 + n]
    r = run(hc, [p for _, p in sel])
    k = sum(s for s, _ in sel)
    assert r["segs"] == 1 and r["count"] == n and r["code"] == 0
    assert r["seg0"] == H.g2_b(B.E2.mul(B.G2, k % B.R))
    assert r["sig"] == compressed(k)


@pytest.mark.parametrize("n", [65, 128, 150])
def test_group_fold_over_segments(hc, pts, n):
    sel = pts[:n]
    r = run(hc, [p for _, p in sel])
    assert r["segs"] == (n + 63) // 64 and r["count"] == n
    assert r["seg0"] == H.g2_b(B.E2.mul(B.G2, sum(s for s, _ in sel[:64]) % B.R))
    assert r["sig"] == compressed(sum(s for s, _ in sel))


def test_predicate_skip_take_valid(hc, pts):
    n = 70
    sel = pts[:n]
    rng = np.random.default_rng(3)
    skip, take, valid = (rng.integers(0, 2, n) for _ in range(3))
    take[[15, 16, 63, 64]] = 0  # both sides of a sub-lane and of a segment boundary
    r = run(hc, [p for _, p in sel], skip, take, valid)
    inn = [i for i in range(n) if not skip[i] and take[i] and valid[i]]
    assert 0 < len(inn) < n
    assert r["count"] == len(inn) and r["sig"] == compressed(sum(sel[i][0] for i in inn))
    # take = NULL and valid = NULL take every set that is not skipped
    r = run(hc, [p for _, p in sel], skip)
    assert r["sig"] == compressed(sum(sel[i][0] for i in range(n) if not skip[i]))


def test_mask_that_leaves_nothing(hc, pts):
    sel = [p for _, p in pts[:17]]
    for kw in ({"skip": [1] * 17}, {"take": [0] * 17}, {"valid": [0] * 17}):
        r = run(hc, sel, **kw)
        assert r["sig"] == IDENTITY and r["count"] == 0 and r["code"] == 0 and r["seg0"] == bytes(192)
    # and then prev alone comes back
    prev = compressed(77)
    r = run(hc, sel, take=[0] * 17, prev=prev)
    assert r["sig"] == prev and r["count"] == 0


def test_two_equal_points_double(hc, pts):
    k, p = pts[9]
    # in one sub-lane (sets 0 and 16: the mixed addition doubles) and in two (sets 0 and 1: the tree doubles)
    for pos in (16, 1):
        sel = [pts[20 + i] for i in range(18)]
        sel[0], sel[pos] = (k, p), (k, p)
        r = run(hc, [q for _, q in sel])
        assert r["count"] == 18 and r["sig"] == compressed(sum(s for s, _ in sel))
    r = run(hc, [p, p])
    assert r["sig"] == B.g2_compress(B.E2.dbl(p))


def test_point_beside_its_negation_is_the_identity(hc, pts):
    k, p = pts[4]
    r = run(hc, [p, B.E2.neg(p)])  # in two sub-lanes: the tree cancels
    assert r["sig"] == IDENTITY and r["count"] == 2 and r["seg0"] == bytes(192)
    # in one sub-lane (sets 0 and 16, the fifteen between them skipped): the mixed addition cancels
    r = run(hc, [p] + [q for _, q in pts[100:115]] + [B.E2.neg(p)], skip=[0] + [1] * 15 + [0])
    assert r["sig"] == IDENTITY and r["count"] == 2 and r["seg0"] == bytes(192)
    # beside other points the pair cancels and the rest remains
    r = run(hc, [p, pts[5][1], B.E2.neg(p)])
    assert r["sig"] == compressed(pts[5][0]) and r["count"] == 3


def test_prev_is_added_and_minus_the_sum_gives_the_identity(hc, pts):
    sel = pts[30:30 + 20]
    k = sum(s for s, _ in sel)
    r = run(hc, [p for _, p in sel], prev=compressed(12345))
    assert r["sig"] == compressed(k + 12345) and r["count"] == 20 and r["code"] == 0
    r = run(hc, [p for _, p in sel], prev=IDENTITY)
    assert r["sig"] == compressed(k) and r["code"] == 0
    r = run(hc, [p for _, p in sel], prev=compressed(-k))
    assert r["sig"] == IDENTITY and r["count"] == 20 and r["code"] == 0
    r = run(hc, [p for _, p in sel], prev=compressed(k))  # prev equals the sum: the last addition doubles
    assert r["sig"] == compressed(2 * k)


def not_on_curve(rng):
    while True:
        b = bytearray(rng.integers(0, 256, size=96, dtype=np.uint8).tobytes())
        b[0] = 0x80 | (b[0] & 0x0F)
        b[48] &= 0x0F
        if B.g2_decompress(bytes(b))[0] == B.BLST_POINT_NOT_ON_CURVE:
            return bytes(b)


def outside_g2(rng):
    while True:
        b = bytearray(rng.integers(0, 256, size=96, dtype=np.uint8).tobytes())
        b[0] = 0x80 | (b[0] & 0x0F)
        b[48] &= 0x0F
        code, pt = B.g2_decompress(bytes(b))
        if code == 0 and not B.g2_in_subgroup(pt):
            return bytes(b), pt


def test_prev_that_does_not_decode(hc, pts):
    rng = np.random.default_rng(17)
    sel = pts[50:50 + 5]
    alone = compressed(sum(s for s, _ in sel))
    good = bytearray(compressed(99))
    flag = bytes([good[0] & 0x7F]) + bytes(good[1:])  # compression flag cleared
    inf_junk = bytes([0xC0]) + bytes(94) + b"\x01"  # infinity flag with other bits set
    x_ge_p = bytes([0x9F]) + b"\xff" * 95
    for prev, code in ((flag, B.BLST_BAD_ENCODING), (inf_junk, B.BLST_BAD_ENCODING), (x_ge_p, B.BLST_BAD_ENCODING),
                       (not_on_curve(rng), B.BLST_POINT_NOT_ON_CURVE)):
        r = run(hc, [p for _, p in sel], prev=prev)
        assert r["code"] == code and r["sig"] == alone and r["count"] == 5, prev.hex()


def test_prev_outside_g2_is_accepted(hc, pts):
    """signatureFromBytesNoCheck: no subgroup check; the expected bytes are the oracle's plain curve addition"""
    rng = np.random.default_rng(29)
    prev, pt = outside_g2(rng)
    sel = pts[60:60 + 3]
    total = B.E2.mul(B.G2, sum(s for s, _ in sel) % B.R)
    r = run(hc, [p for _, p in sel], prev=prev)
    assert r["code"] == 0 and r["count"] == 3
    assert r["sig"] == B.g2_compress(B.E2.add(total, pt))


def test_y_sign_bit_for_both_signs(hc, pts):
    k, p = pts[7]
    a, b = run(hc, [p])["sig"], run(hc, [B.E2.neg(p)])["sig"]
    assert a == B.g2_compress(p) and b == B.g2_compress(B.E2.neg(p))
    assert (a[0] & 0x20) != (b[0] & 0x20) and a[0] & 0x80 and b[0] & 0x80
    assert bytes([a[0] & 0x1F]) + a[1:] == bytes([b[0] & 0x1F]) + b[1:]
