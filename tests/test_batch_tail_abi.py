"""C ABI of the batch-first tail (include/bgv.h bgv_batch_tail, bgv_tail_path,
bgv_tail_stats): the exported symbols, the struct's layout against a compiled
sizeof / offsetof, the null arguments refused before any device call, and (on
a device) the modes outside -1 .. 1."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bgv_batch_tail", "bgv_tail_stats")


@pytest.fixture(scope="module")
def lib():
    from tools import build
    build.build()
    from lodestar_amd import native
    return native.load_library()


def test_symbols_are_exported(lib):
    from lodestar_amd import native
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "lodestar_amd", "libbgv.so")]).decode()
    for s in SYMBOLS:
        assert f" T {s}\n" in out
        assert s in native.EXPORTS
        assert getattr(lib, s).restype is ctypes.c_int
    assert lib.bgv_abi_version() == 4  # additive: the ABI version stays


def test_cfg_did_not_grow():
    from lodestar_amd import native
    assert [f for f, _ in native.BgvCfg._fields_][-1] == "hash_dedup"  # the switch is a context call
    assert "batch_tail" not in native.BgvCfg.AUTO


def test_tail_path_layout_matches_ctypes(tmp_path):
    from lodestar_amd import native
    fields = [f for f, _ in native.BgvTailPath._fields_]
    assert fields == ["batch_first", "retried"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu\\n", sizeof(bgv_tail_path));']
    lines += [f'printf("%zu\\n", offsetof(bgv_tail_path, {f}));' for f in fields]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == 8 == ctypes.sizeof(native.BgvTailPath)
    assert vals[1:] == [getattr(native.BgvTailPath, f).offset for f in fields] == [0, 4]


def test_null_arguments_are_refused(lib):
    from lodestar_amd import native
    for mode in (-1, 0, 1, 2):
        assert lib.bgv_batch_tail(None, mode) == native.BGV_E_INVALID_ARG
    out = native.BgvTailPath()
    assert lib.bgv_tail_stats(None, ctypes.byref(out)) == native.BGV_E_INVALID_ARG
    assert lib.bgv_tail_stats(None, None) == native.BGV_E_INVALID_ARG


@pytest.mark.gpu
def test_modes_outside_the_range_are_refused():
    from lodestar_amd import native
    d = native.Device(0)
    try:
        for mode in (-1, 0, 1):
            d.batch_tail(mode)
        for mode in (-2, 2, 7):
            assert d.lib.bgv_batch_tail(d.h, mode) == native.BGV_E_INVALID_ARG
            assert b"bgv_batch_tail mode" in d.lib.bgv_last_error()
        out = native.BgvTailPath()
        assert d.lib.bgv_tail_stats(d.h, None) == native.BGV_E_INVALID_ARG
        assert d.lib.bgv_tail_stats(d.h, ctypes.byref(out)) == native.BGV_OK
        assert (out.batch_first, out.retried) == (0, 0)
    finally:
        d.close()
