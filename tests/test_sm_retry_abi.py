"""C ABI of the split retry of the same-message entries (include/bgv.h
bgv_sm_retry, bgv_sm_retry_path, bgv_sm_retry_stats, bgv_sm_split_plan): the
exported symbols, the struct's layout against a compiled sizeof / offsetof, the
null arguments refused before any device call, the host-only plan of a
segment's subs and (on a device) the modes outside 0 .. 1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bgv_sm_retry", "bgv_sm_retry_stats", "bgv_sm_split_plan")
FIELDS = ["mode", "segments", "subs", "subs_failed", "leaves", "pairs", "hashes"]
SUB = 8
FAIL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    from tools import build
    build.build()
    from lodestar_amd import native
    return native.load_library()


def rule(m):
    """the issue's rule, restated: m subs of one set up to 8 sets, else subs of 8 with a shorter last one"""
    if m <= SUB:
        return list(range(m + 1))
    return list(range(0, m, SUB)) + [m]


def plan(lib, m, cap, guard=4):
    """(result, the cap entries, the guard words behind them)"""
    buf = np.full(cap + guard, 0xA5A5A5A5, np.uint32)
    got = lib.bgv_sm_split_plan(m, buf.ctypes.data, cap)
    return got, buf[:cap].tolist(), buf[cap:].tolist()


def test_symbols_are_exported(lib):
    from lodestar_amd import native
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "lodestar_amd", "libbgv.so")]).decode()
    for s in SYMBOLS:
        assert f" T {s}\n" in out
        assert s in native.EXPORTS + native.EXPORTS_U32
    assert lib.bgv_sm_retry.restype is ctypes.c_int and lib.bgv_sm_retry_stats.restype is ctypes.c_int
    assert lib.bgv_sm_split_plan.restype is ctypes.c_uint32
    assert lib.bgv_abi_version() == 4  # additive: the ABI version stays
    assert native.SM_SUB == SUB


def test_cfg_did_not_grow():
    from lodestar_amd import native
    assert [f for f, _ in native.BgvCfg._fields_][-1] == "hash_dedup"  # the switch is a context call
    assert "sm_retry" not in native.BgvCfg.AUTO


def test_retry_path_layout_matches_ctypes(tmp_path):
    from lodestar_amd import native
    assert [f for f, _ in native.BgvSmRetryPath._fields_] == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu\\n", sizeof(bgv_sm_retry_path));', 'printf("%d\\n", BGV_SM_SUB);']
    lines += [f'printf("%zu\\n", offsetof(bgv_sm_retry_path, {f}));' for f in FIELDS]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == 28 == ctypes.sizeof(native.BgvSmRetryPath)
    assert vals[1] == SUB
    assert vals[2:] == [getattr(native.BgvSmRetryPath, f).offset for f in FIELDS] == [4 * k for k in range(7)]


def test_null_arguments_are_refused(lib):
    from lodestar_amd import native
    for mode in (-1, 0, 1, 2):
        assert lib.bgv_sm_retry(None, mode) == native.BGV_E_INVALID_ARG
    out = native.BgvSmRetryPath()
    assert lib.bgv_sm_retry_stats(None, ctypes.byref(out)) == native.BGV_E_INVALID_ARG
    assert lib.bgv_sm_retry_stats(None, None) == native.BGV_E_INVALID_ARG


@pytest.mark.parametrize("m", [0, 1, 2, 7, 8, 9, 16, 17, 63, 64])
def test_split_plan_follows_the_rule(lib, m):
    want = rule(m)
    subs = len(want) - 1
    assert subs == (m if m <= SUB else -(-m // SUB))
    got, off, guard = plan(lib, m, 70)
    assert got == subs
    assert off[: subs + 1] == want
    assert off[subs + 1:] == [0xA5A5A5A5] * (70 - subs - 1)  # nothing behind the offsets
    assert guard == [0xA5A5A5A5] * 4
    sizes = np.diff(want)
    assert sizes.sum() == m and (sizes >= 1).all()
    if m > SUB:
        assert (sizes[:-1] == SUB).all() and 1 <= sizes[-1] <= SUB
    # the exact fit
    got, off, guard = plan(lib, m, subs + 1)
    assert got == subs and off == want and guard == [0xA5A5A5A5] * 4


@pytest.mark.parametrize("m", [0, 1, 8, 9, 64])
def test_split_plan_with_too_small_a_cap_writes_nothing(lib, m):
    subs = len(rule(m)) - 1
    for cap in sorted({0, subs // 2, subs}):
        got, off, guard = plan(lib, m, cap)
        assert got == FAIL
        assert off == [0xA5A5A5A5] * cap and guard == [0xA5A5A5A5] * 4
    assert lib.bgv_sm_split_plan(m, None, 100) == FAIL


@pytest.mark.gpu
def test_modes_outside_the_range_are_refused():
    from lodestar_amd import native
    d = native.Device(0)
    try:
        for mode in (0, 1, 0):
            d.sm_retry(mode)
        for mode in (-1, 2, 7):
            assert d.lib.bgv_sm_retry(d.h, mode) == native.BGV_E_INVALID_ARG
            assert b"bgv_sm_retry mode" in d.lib.bgv_last_error()
        out = native.BgvSmRetryPath()
        assert d.lib.bgv_sm_retry_stats(d.h, None) == native.BGV_E_INVALID_ARG
        assert d.lib.bgv_sm_retry_stats(d.h, ctypes.byref(out)) == native.BGV_OK
        assert [getattr(out, f) for f in FIELDS] == [0] * 7
        d2 = native.Device(0, sm_retry=1)  # the cfg key is a context call, like pair_merge
        d2.close()
    finally:
        d.close()
