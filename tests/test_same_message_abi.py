"""C ABI of same-message batch verification (include/bgv.h bgv_sm_batch,
bgv_verify_same_message): exported symbols, struct layouts against the ctypes
mirrors, the host-side contract check, and the addon's entry points.  No
compute calls here (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_verify_same_message", "bgv_sm_check", "bgv_debug_same_message")


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
    fb = [f for f, _ in native.BgvSmBatch._fields_]
    fs = [f for f, _ in native.BgvSmStats._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu %zu\\n", sizeof(bgv_sm_batch), sizeof(bgv_sm_stats));']
    lines += [f'printf("%zu\\n", offsetof(bgv_sm_batch, {f}));' for f in fb]
    lines += [f'printf("%zu\\n", offsetof(bgv_sm_stats, {f}));' for f in fs]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == ctypes.sizeof(native.BgvSmBatch)
    assert vals[1] == ctypes.sizeof(native.BgvSmStats)
    assert vals[2:2 + len(fb)] == [getattr(native.BgvSmBatch, f).offset for f in fb]
    assert vals[2 + len(fb):] == [getattr(native.BgvSmStats, f).offset for f in fs]
    assert fb == ["n_sets", "n_groups", "group_offsets", "pk_indices", "raw_pks", "n_raw", "msgs", "sigs", "sig_len",
                  "scalars", "on_device"]
    assert fs == ["n_sets", "n_groups", "n_segments", "hashes", "pairs", "groups_retried", "sets_retried", "total_ms"]


def _arrays(offsets, n=4):
    return {"n_sets": n, "n_groups": len(offsets) - 1, "group_offsets": np.array(offsets, np.uint32),
            "pk_indices": np.arange(n, dtype=np.uint32), "msgs": np.zeros((len(offsets) - 1, 32), np.uint8),
            "sigs": np.zeros((n, 192), np.uint8), "sig_len": np.full(n, 96, np.uint32),
            "scalars": np.arange(1, n + 1, dtype=np.uint64)}


def _check(lib, arrays):
    from lodestar_amd import native
    b = native.Device.make_sm_batch(arrays)
    return lib.bgv_sm_check(ctypes.byref(b)), lib.bgv_last_error().decode()


def test_contract_violations_are_invalid_arg_without_a_device(lib):
    from lodestar_amd import native
    assert _check(lib, _arrays([0, 1, 4]))[0] == native.BGV_OK
    assert _check(lib, _arrays([0, 4]))[0] == native.BGV_OK
    assert lib.bgv_sm_check(None) == native.BGV_E_INVALID_ARG
    for missing in ("group_offsets", "pk_indices", "msgs", "sigs", "sig_len"):  # NULL arrays
        a = _arrays([0, 2, 4])
        a[missing] = None
        st, msg = _check(lib, a)
        assert st == native.BGV_E_INVALID_ARG and "missing" in msg, missing
    a = _arrays([0, 2, 4])
    a["n_raw"] = 1  # raw rows announced, none given
    assert _check(lib, a)[0] == native.BGV_E_INVALID_ARG
    st, msg = _check(lib, _arrays([0, 3, 2, 4]))  # backwards
    assert st == native.BGV_E_INVALID_ARG and "monotone" in msg
    st, msg = _check(lib, _arrays([0, 2, 2, 4]))  # an empty group
    assert st == native.BGV_E_INVALID_ARG and "empty" in msg
    st, msg = _check(lib, _arrays([0, 2, 3]))  # not ending at n_sets
    assert st == native.BGV_E_INVALID_ARG and "span" in msg
    st, msg = _check(lib, _arrays([1, 2, 4]))  # not starting at 0
    assert st == native.BGV_E_INVALID_ARG and "span" in msg
    assert _check(lib, _arrays([0, 1, 2, 3, 4, 4]))[0] == native.BGV_E_INVALID_ARG  # n_groups > n_sets
    a = _arrays([0, 2, 4])
    a["scalars"][2] = 0
    st, msg = _check(lib, a)
    assert st == native.BGV_E_INVALID_ARG and "scalars[2]" in msg
    a = _arrays([0, 2, 4])
    a["scalars"] = None  # drawn on the device
    assert _check(lib, a)[0] == native.BGV_OK


def test_empty_batch_is_accepted(lib):
    from lodestar_amd import native
    b = native.BgvSmBatch()
    assert lib.bgv_sm_check(ctypes.byref(b)) == native.BGV_OK


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_addon_exports_same_message_entries():
    from tools import build as B
    addon = B.build_addon()
    if addon is None:
        pytest.skip("node_api.h not found")
    script = f"""
const a = require({addon!r});
for (const k of ["verifySameMessage", "verifySameMessageSync"]) if (typeof a[k] !== "function") throw Error("missing " + k);
const v = require({os.path.join(ROOT, "lodestar_amd", "napi", "index.js")!r});
for (const c of [v.BlsGpuVerifier, v.BlsGpuSingleThreadVerifier])
  if (typeof c.prototype.verifySignatureSetsSameMessage !== "function") throw Error("no verifySignatureSetsSameMessage");
console.log("ok");
"""
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"
