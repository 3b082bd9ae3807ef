"""C ABI of the message-class pass (include/bgv.h bgv_cfg.hash_dedup,
bgv_hash_path, bgv_hash_stats): the exported symbol, the struct's size and
offsets against a compiled sizeof / offsetof, the cfg default and the values
refused before any device call.  No compute calls here (no GPU needed)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tools import build
    build.build()
    from lodestar_amd import native
    return native.load_library()


def test_hash_stats_is_exported(lib):
    from lodestar_amd import native
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "lodestar_amd", "libbgv.so")]).decode()
    assert " T bgv_hash_stats\n" in out
    assert "bgv_hash_stats" in native.EXPORTS
    assert lib.bgv_hash_stats.restype is ctypes.c_int
    assert lib.bgv_abi_version() == 4  # additive: the ABI version stays
    out = native.BgvHashPath()
    assert lib.bgv_hash_stats(None, ctypes.byref(out)) == native.BGV_E_INVALID_ARG  # no context


def test_hash_path_and_cfg_layout_match_ctypes(tmp_path):
    from lodestar_amd import native
    fields = [f for f, _ in native.BgvHashPath._fields_]
    assert fields == ["sets", "hashes", "dedup"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu %zu %zu\\n", sizeof(bgv_hash_path), sizeof(bgv_cfg), offsetof(bgv_cfg, hash_dedup));']
    lines += [f'printf("%zu\\n", offsetof(bgv_hash_path, {f}));' for f in fields]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == 12 == ctypes.sizeof(native.BgvHashPath)
    assert vals[1] == ctypes.sizeof(native.BgvCfg)
    assert vals[2] == native.BgvCfg.hash_dedup.offset == ctypes.sizeof(native.BgvCfg) - 4  # the last field
    assert vals[3:] == [getattr(native.BgvHashPath, f).offset for f in fields]


def test_cfg_default_and_refused_values(lib):
    from lodestar_amd import native
    c = native.BgvCfg()
    lib.bgv_cfg_default(ctypes.byref(c))
    assert c.hash_dedup == -1 == native.BgvCfg.AUTO["hash_dedup"]
    assert native.BgvCfg.make(hash_dedup=0).hash_dedup == 0
    h = ctypes.c_void_p()
    for bad in (2, -2):  # refused before any device call (no GPU needed)
        st = lib.bgv_open_cfg(0, ctypes.byref(native.BgvCfg.make(hash_dedup=bad)), ctypes.byref(h))
        assert st == native.BGV_E_INVALID_ARG and not h.value
        assert b"hash_dedup" in lib.bgv_last_error()
