"""The rule of the split retry (lodestar_amd/csrc/sm_split.h) compiled for the
host and compared with a few lines of Python: the subs of a retried segment,
their offsets over several segments planned back to back, and the counters
(subs, subs_failed, leaves, pairs) that hand-made sub verdicts lead to; and
sm_collect, the host fold of the first pass's results that plans those subs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_sm_split.cpp")
LIB = os.path.join(HERE, "native", "libhostcheck_sm_split.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
SUB = 8
FAIL = 0xFFFFFFFF
RETRY = -11  # a sub whose P_sub is the identity: its pair is skipped (C_SEG_RETRY)


@pytest.fixture(scope="module")
def hc():
    deps = [SRC, os.path.join(CSRC, "sm_split.h"), os.path.join(CSRC, "bls_types.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for f in ("hc_sm_sub", "hc_sm_sub_count", "hc_sm_sub_begin", "hc_sm_split_plan", "hc_sm_retry_counts", "hc_sm_collect"):
        getattr(lib, f).restype = ctypes.c_uint32
    lib.hc_sm_sub_count.argtypes = [ctypes.c_uint32]
    lib.hc_sm_sub_begin.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.hc_sm_split_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    lib.hc_sm_retry_counts.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                       ctypes.c_void_p]
    lib.hc_sm_collect.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32] + [ctypes.c_void_p] * 7
    return lib


def rule(m):
    """the sub offsets of a segment with m surviving sets"""
    if m <= SUB:
        return list(range(m + 1))
    return list(range(0, m, SUB)) + [m]


def counts(sizes, jr):
    """the counters, from the sub sizes and their verdicts"""
    failed = [j != 1 for j in jr]
    opened = [s for s, f in zip(sizes, failed) if f and s >= 2]
    paired = sum(1 for j in jr if j >= 0)
    return [len(sizes), sum(failed), sum(opened), 2 * paired + 2 * sum(opened)]


def test_sub_size_is_the_abi_constant(hc):
    assert hc.hc_sm_sub() == SUB


@pytest.mark.parametrize("m", list(range(0, 20)) + [31, 32, 33, 56, 57, 63, 64])
def test_plan_of_one_segment(hc, m):
    want = rule(m)
    assert hc.hc_sm_sub_count(m) == len(want) - 1
    assert [hc.hc_sm_sub_begin(m, t) for t in range(len(want))] == want
    for base in (0, 1000):
        buf = np.full(len(want) + 2, 0xA5A5A5A5, np.uint32)
        assert hc.hc_sm_split_plan(m, base, buf.ctypes.data, len(want)) == len(want) - 1
        assert buf.tolist() == [base + x for x in want] + [0xA5A5A5A5] * 2
        buf[:] = 0xA5A5A5A5
        assert hc.hc_sm_split_plan(m, base, buf.ctypes.data, len(want) - 1) == FAIL  # one entry short
        assert (buf == 0xA5A5A5A5).all()


def run_counts(hc, ms, jr):
    m = np.array(ms if ms else [0], np.uint32)
    j = np.array(jr if jr else [0], np.int32)
    off = np.zeros(sum(ms) + 2, np.uint32)
    out = np.zeros(4, np.uint32)
    T = hc.hc_sm_retry_counts(m.ctypes.data, len(ms), j.ctypes.data, off.ctypes.data, len(off), out.ctypes.data)
    return T, off[: T + 1].tolist() if T != FAIL else None, out.tolist()


def offsets(ms):
    off, base = [], 0
    for m in ms:
        off += [base + x for x in rule(m)[:-1]]
        base += m
    return off + [base]


# (surviving sets per retried segment, verdict per sub, what it stands for)
PATTERNS = [
    ([64], [1, 1, 0, 1, 1, 1, 1, 1], "one bad set in a full segment: 8 subs, 8 leaves, 32 pairs"),
    ([64], [0] * 8, "a full segment all bad"),
    ([2], [0, 0], "the group of two all bad: no leaves"),
    ([9], [1, 0], "the last set of nine bad: a one-set tail sub, final without a leaf"),
    ([9], [0, 1], "the first sub of nine"),
    ([64], [RETRY, 1, 0, 1, 1, 1, 1, 1], "an identity sub is not paired, counts as failed and is opened"),
    ([1], [RETRY], "cannot happen on the device (one key, r != 0), but the rule holds: failed, no leaf, no pair"),
    ([63, 5, 17], [1] * 7 + [0] + [1, 0, 1, 1, 0] + [0, 1, 0], "three segments back to back"),
    ([8], [1, 1, 1, 0, 1, 1, 1, 1], "eight survivors: eight subs of one"),
    ([], [], "nothing retried"),
]


@pytest.mark.parametrize("ms,jr,what", PATTERNS, ids=[p[2].split(":")[0] for p in PATTERNS])
def test_counts_of_handmade_verdicts(hc, ms, jr, what):
    want_off = offsets(ms)
    assert len(jr) == len(want_off) - 1
    T, off, got = run_counts(hc, ms, jr)
    assert T == len(jr)
    if ms:
        assert off == want_off
    assert got == counts(np.diff(want_off).tolist(), jr), what


def test_the_issue_figures(hc):
    """the counts the issue states: one bad set of 64 costs 32 pairs, a full bad segment 8 subs and 64 leaves"""
    assert run_counts(hc, [64], [1, 1, 1, 1, 1, 0, 1, 1])[2] == [8, 1, 8, 32]
    assert run_counts(hc, [64], [0] * 8)[2] == [8, 8, 64, 16 + 128]
    assert run_counts(hc, [2], [0, 0])[2] == [2, 2, 0, 4]
    assert run_counts(hc, [9], [1, 0])[2] == [2, 1, 0, 4]


def test_random_patterns(hc):
    rng = np.random.default_rng(41)
    for _ in range(200):
        ms = rng.integers(1, 65, size=int(rng.integers(1, 6))).tolist()
        off = offsets(ms)
        jr = rng.choice([1, 1, 1, 0, RETRY], size=len(off) - 1).tolist()
        T, got_off, got = run_counts(hc, ms, jr)
        assert T == len(jr) and got_off == off
        assert got == counts(np.diff(off).tolist(), jr)


# ---- sm_collect: the host fold of the first pass's results that feeds the retries
def collect(hc, seg_off, seg_group, jr, sk, jr1, split=True):
    """(set_valid, list, list_group, sub_off, [pairs, groups_retried, segments], tally of jr1 over the subs)"""
    S, n = len(jr), seg_off[-1]
    a = lambda x, t: np.array(x if len(x) else [0], t)
    so, sgp, j, k, j1 = a(seg_off, np.uint32), a(seg_group, np.uint32), a(jr, np.int32), a(sk, np.uint32), a(jr1, np.int32)
    sc = np.arange(n, dtype=np.int32) % 7
    valid, code = np.full(n, 9, np.uint8), np.full(n, -1, np.int32)
    lst, grp, sub = (np.zeros(n + 1, np.uint32) for _ in range(3))
    cnt = np.zeros(8, np.uint32)
    nr = hc.hc_sm_collect(S, so.ctypes.data, sgp.ctypes.data, j.ctypes.data, sc.ctypes.data, k.ctypes.data, int(split),
                          valid.ctypes.data, code.ctypes.data, j1.ctypes.data, lst.ctypes.data, grp.ctypes.data,
                          sub.ctypes.data, cnt.ctypes.data)
    assert code.tolist() == sc.tolist()
    T = int(cnt[3])
    return valid.tolist(), lst[:nr].tolist(), grp[:nr].tolist(), sub[: T + 1].tolist(), cnt[:3].tolist(), cnt[4:].tolist()


def test_collect_a_retried_segment_after_a_clean_one_of_its_group(hc):
    """group 0 spans two segments, 64 + 6 sets; the first passes, the second fails with one set skipped;
    group 1 (one segment of 10) passes.  The subs and their counts are the ones the rule gives for 5 survivors."""
    sk = [0] * 80
    sk[66] = sk[75] = 1
    jr1 = [1, 1, 0, 1, 1]
    valid, lst, grp, sub, first, tally = collect(hc, [0, 64, 70, 80], [0, 0, 1], [1, 0, 1], sk, jr1)
    assert lst == [64, 65, 67, 68, 69] and grp == [0] * 5
    assert sub == offsets([5]) and first == [6, 1, 1]
    assert valid == [1] * 64 + [0] * 6 + [1] * 5 + [0] + [1] * 4
    assert tally == counts(np.diff(sub).tolist(), jr1) == run_counts(hc, [5], jr1)[2]
    # the per-set retry takes the same list and plans no sub
    assert collect(hc, [0, 64, 70, 80], [0, 0, 1], [1, 0, 1], sk, [], split=False)[1:5] == (lst, grp, [5], first)


def test_collect_a_segment_with_fewer_survivors_than_one_sub(hc):
    """61 of 64 sets were rejected before the pairing: 3 survivors, three subs of one, no leaf whatever fails;
    beside it a segment whose weighted key sum was the identity (not paired) and a dead one (not retried)"""
    sk = [1] * 64 + [0] * 12 + [1] * 4
    for i in (3, 30, 63):
        sk[i] = 0
    jr1 = [0, 1, 0] + [1, 0]
    valid, lst, grp, sub, first, tally = collect(hc, [0, 64, 76, 80], [0, 1, 2], [0, RETRY, -10], sk, jr1)
    assert lst == [3, 30, 63] + list(range(64, 76)) and grp == [0] * 3 + [1] * 12
    assert sub == offsets([3, 12]) and first == [2, 2, 2]
    assert valid == [0] * 80
    assert tally == counts(np.diff(sub).tolist(), jr1) == run_counts(hc, [3, 12], jr1)[2]
    assert tally == [5, 3, 4, 2 * 5 + 2 * 4]


def test_collect_stand_alone_under_the_sanitizers(tmp_path):
    """the same two shapes in a program of its own, built with -fsanitize=address,undefined (runtimes linked
    statically) over heap arrays of exactly their size: a finding aborts the program"""
    exe = tmp_path / "hostcheck_sm_split_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DHOSTCHECK_SM_SPLIT_MAIN", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hostcheck sm split OK 2" in r.stdout, r.stdout + r.stderr[-3000:]
