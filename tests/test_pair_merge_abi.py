"""C ABI of the pair classes (include/bgv.h bgv_pair_merge, bgv_pair_path,
bgv_pair_stats, bgv_debug_pair_classes): the exported symbols, the struct's
size and offsets against a compiled sizeof / offsetof, and the calls refused
before any device call.  No compute calls here (no GPU needed)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bgv_pair_merge", "bgv_pair_stats", "bgv_debug_pair_classes")


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
    assert "pair_merge" not in native.BgvCfg.AUTO


def test_pair_path_layout_matches_ctypes(tmp_path):
    from lodestar_amd import native
    fields = [f for f, _ in native.BgvPairPath._fields_]
    assert fields == ["sets", "pairs", "merged", "fallback"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu\\n", sizeof(bgv_pair_path));']
    lines += [f'printf("%zu\\n", offsetof(bgv_pair_path, {f}));' for f in fields]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == 16 == ctypes.sizeof(native.BgvPairPath)
    assert vals[1:] == [getattr(native.BgvPairPath, f).offset for f in fields] == [0, 4, 8, 12]


def test_null_context_is_refused(lib):
    from lodestar_amd import native
    assert lib.bgv_pair_merge(None, 1) == native.BGV_E_INVALID_ARG
    out = native.BgvPairPath()
    assert lib.bgv_pair_stats(None, ctypes.byref(out)) == native.BGV_E_INVALID_ARG
    assert lib.bgv_debug_pair_classes(None, None, None, None, None, None, None, None, None) == native.BGV_E_INVALID_ARG
