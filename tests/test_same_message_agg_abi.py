"""C ABI of same-message batch verification of aggregate sets (include/bgv.h
bgv_sma_batch, bgv_verify_same_message_agg): exported symbols, the struct
layout against the ctypes mirror, every refusal of the host-side contract
check, and the addon's entry points.  No compute calls here (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_verify_same_message_agg", "bgv_sma_check", "bgv_debug_same_message_agg")


@pytest.fixture(scope="module")
def lib():
    from tools import build
    build.build()
    from lodestar_amd import native
    return native.load_library()


def test_new_functions_are_exported(lib):
    from lodestar_amd import native
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "lodestar_amd", "libbgv.so")]).decode()
    for name in NEW:
        assert f" T {name}\n" in out, name
        assert name in native.EXPORTS
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.bgv_abi_version() == 4  # additive: the ABI version stays


def test_struct_layout_matches_ctypes(tmp_path):
    from lodestar_amd import native
    fb = [f for f, _ in native.BgvSmaBatch._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu\\n", sizeof(bgv_sma_batch));']
    lines += [f'printf("%zu\\n", offsetof(bgv_sma_batch, {f}));' for f in fb]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == ctypes.sizeof(native.BgvSmaBatch)
    assert vals[1:] == [getattr(native.BgvSmaBatch, f).offset for f in fb]
    assert fb == ["n_sets", "n_groups", "group_offsets", "pk_offsets", "pk_indices", "raw_pks", "n_raw", "msgs", "sigs",
                  "sig_len", "scalars", "on_device"]


def _arrays(groups=(0, 2, 4), keys=(0, 1, 3, 4, 7)):
    n = len(keys) - 1
    return {"n_sets": n, "n_groups": len(groups) - 1, "group_offsets": np.array(groups, np.uint32),
            "pk_offsets": np.array(keys, np.uint32), "pk_indices": np.arange(max(keys[-1], 1), dtype=np.uint32),
            "msgs": np.zeros((len(groups) - 1, 32), np.uint8), "sigs": np.zeros((n, 192), np.uint8),
            "sig_len": np.full(n, 96, np.uint32), "scalars": np.arange(1, n + 1, dtype=np.uint64)}


def test_contract_violations_are_refused_without_a_device(lib):
    from lodestar_amd import native
    check = native.sma_check
    assert check(_arrays()) == (native.BGV_OK, "")
    assert check(_arrays(groups=(0, 4)))[0] == native.BGV_OK
    assert check(_arrays(keys=(0, 1, 2, 3, 4)))[0] == native.BGV_OK  # single-key sets are legal
    assert lib.bgv_sma_check(None) == native.BGV_E_INVALID_ARG
    for missing in ("group_offsets", "pk_offsets", "pk_indices", "msgs", "sigs", "sig_len"):  # a missing array
        a = _arrays()
        a[missing] = None
        st, msg = check(a)
        assert st == native.BGV_E_INVALID_ARG and "missing" in msg, missing
    a = _arrays()
    a["n_raw"] = 1  # raw rows announced, none given
    assert check(a)[0] == native.BGV_E_INVALID_ARG
    st, msg = check(_arrays(keys=(0, 3, 2, 4, 7)))  # pk_offsets run backwards
    assert st == native.BGV_E_INVALID_ARG and "pk_offsets not monotone" in msg
    st, msg = check(_arrays(keys=(1, 2, 3, 4, 7)))  # pk_offsets do not start at 0
    assert st == native.BGV_E_INVALID_ARG and "pk_offsets must span" in msg
    st, msg = check(_arrays(keys=(0, 1, 1, 4, 7)))  # a set without keys
    assert st == native.BGV_E_EMPTY_SET and "EMPTY_AGGREGATE_ARRAY (set 1)" in msg
    st, msg = check(_arrays(keys=(0, 1, 3, 4, 4)))  # the last set without keys
    assert st == native.BGV_E_EMPTY_SET and "set 3" in msg
    st, msg = check(_arrays(groups=(0, 3, 2, 4)))  # group offsets run backwards
    assert st == native.BGV_E_INVALID_ARG and "group_offsets not monotone" in msg
    st, msg = check(_arrays(groups=(0, 2, 2, 4)))  # an empty group
    assert st == native.BGV_E_INVALID_ARG and "empty" in msg
    st, msg = check(_arrays(groups=(0, 2, 3)))  # groups not ending at n_sets
    assert st == native.BGV_E_INVALID_ARG and "group_offsets must span" in msg
    st, msg = check(_arrays(groups=(1, 2, 4)))  # groups not starting at 0
    assert st == native.BGV_E_INVALID_ARG and "group_offsets must span" in msg
    assert check(_arrays(groups=(0, 1, 2, 3, 4, 4)))[0] == native.BGV_E_INVALID_ARG  # n_groups > n_sets
    a = _arrays()
    a["scalars"][2] = 0
    st, msg = check(a)
    assert st == native.BGV_E_INVALID_ARG and "scalars[2]" in msg
    a = _arrays()
    a["scalars"] = None  # drawn on the device
    assert check(a)[0] == native.BGV_OK


def test_on_device_batch_is_not_read(lib):
    """on_device: the arrays live in HBM, the host check must not touch them (the addresses here are not mapped)"""
    from lodestar_amd import native
    b = native.BgvSmaBatch()
    b.n_sets, b.n_groups, b.on_device = 4, 2, 1
    for f in ("group_offsets", "pk_offsets", "pk_indices", "msgs", "sigs", "sig_len", "scalars"):
        setattr(b, f, 0x10)
    assert lib.bgv_sma_check(ctypes.byref(b)) == native.BGV_OK
    b.pk_offsets = None  # the argument check still holds
    assert lib.bgv_sma_check(ctypes.byref(b)) == native.BGV_E_INVALID_ARG


def test_empty_batch_is_accepted(lib):
    from lodestar_amd import native
    b = native.BgvSmaBatch()
    assert lib.bgv_sma_check(ctypes.byref(b)) == native.BGV_OK


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_addon_exports_same_message_agg_entries():
    from tools import build as B
    addon = B.build_addon()
    if addon is None:
        pytest.skip("node_api.h not found")
    script = f"""
const a = require({addon!r});
for (const k of ["verifySameMessageAgg", "verifySameMessageAggSync"]) if (typeof a[k] !== "function") throw Error("missing " + k);
const v = require({os.path.join(ROOT, "lodestar_amd", "napi", "index.js")!r});
for (const c of [v.BlsGpuVerifier, v.BlsGpuSingleThreadVerifier])
  if (typeof c.prototype.verifyAggregateSetsSameMessage !== "function") throw Error("no verifyAggregateSetsSameMessage");
console.log("ok");
"""
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_encoder_and_merge_rule():
    """tests/js/same_message_agg_test.js --host: encodeSameMessageAgg, mergeSameMessage and the caller-side checks"""
    from tools import build as B
    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "same_message_agg_test.js"), "--host"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same message agg host checks OK" in r.stdout
