"""C ABI of bgv_verify_same_message_aggregate (include/bgv.h bgv_sm_agg):
exported symbols, the struct layout against the ctypes mirror, and the
host-side contract check bgv_sm_agg_check: bgv_sm_check's refusals plus its own
two.  No compute calls here (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_verify_same_message_aggregate", "bgv_sm_agg_check", "bgv_sm_agg_ms")


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
    fa = [f for f, _ in native.BgvSmAgg._fields_]
    fb = [f for f, _ in native.BgvSmBatch._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu %zu\\n", sizeof(bgv_sm_agg), sizeof(bgv_sm_batch));']
    lines += [f'printf("%zu\\n", offsetof(bgv_sm_agg, {f}));' for f in fa]
    lines += [f'printf("%zu\\n", offsetof(bgv_sm_batch, {f}));' for f in fb]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == ctypes.sizeof(native.BgvSmAgg)
    assert vals[1] == ctypes.sizeof(native.BgvSmBatch)
    assert vals[2:2 + len(fa)] == [getattr(native.BgvSmAgg, f).offset for f in fa]
    assert vals[2 + len(fa):] == [getattr(native.BgvSmBatch, f).offset for f in fb]
    assert fa == ["take", "prev_sig96", "agg_sig96", "agg_count", "agg_code"]


def _arrays(offsets, n=4):
    return {"n_sets": n, "n_groups": len(offsets) - 1, "group_offsets": np.array(offsets, np.uint32),
            "pk_indices": np.arange(n, dtype=np.uint32), "msgs": np.zeros((len(offsets) - 1, 32), np.uint8),
            "sigs": np.zeros((n, 192), np.uint8), "sig_len": np.full(n, 96, np.uint32),
            "scalars": np.arange(1, n + 1, dtype=np.uint64)}


def test_own_refusals(lib):
    from lodestar_amd import native
    a = _arrays([0, 1, 4])
    assert native.sm_agg_check(a) == (native.BGV_OK, "")
    take, prev = np.ones(4, np.uint8), np.zeros((2, 96), np.uint8)
    assert native.sm_agg_check(a, take=take, prev=prev)[0] == native.BGV_OK
    st, msg = native.sm_agg_check(a, agg_sig=False)
    assert st == native.BGV_E_INVALID_ARG and "agg_sig96" in msg
    b = native.Device.make_sm_batch(a)
    assert lib.bgv_sm_agg_check(ctypes.byref(b), None) == native.BGV_E_INVALID_ARG
    assert "agg is NULL" in lib.bgv_last_error().decode()
    out = np.zeros((2, 96), np.uint8)
    agg = native.BgvSmAgg(agg_sig96=out.ctypes.data)
    assert lib.bgv_sm_agg_check(None, ctypes.byref(agg)) == native.BGV_E_INVALID_ARG
    # the verify entry refuses the same two before it touches its context
    for bad in (None, ctypes.byref(native.BgvSmAgg())):
        assert lib.bgv_verify_same_message_aggregate(None, ctypes.byref(b), bad, None, None, None) == native.BGV_E_INVALID_ARG


def test_every_refusal_of_bgv_sm_check(lib):
    from lodestar_amd import native

    def both(arrays):
        """the two checks agree on a refused batch: status and text"""
        b = native.Device.make_sm_batch(arrays)
        want = lib.bgv_sm_check(ctypes.byref(b)), lib.bgv_last_error().decode()
        got = native.sm_agg_check(arrays)
        assert want[0] == native.BGV_E_INVALID_ARG and got == want, (got, want)
        return got[1]

    for missing in ("group_offsets", "pk_indices", "msgs", "sigs", "sig_len"):  # NULL arrays
        a = _arrays([0, 2, 4])
        a[missing] = None
        assert "missing" in both(a), missing
    a = _arrays([0, 2, 4])
    a["n_raw"] = 1  # raw rows announced, none given
    both(a)
    assert "monotone" in both(_arrays([0, 3, 2, 4]))  # backwards
    assert "empty" in both(_arrays([0, 2, 2, 4]))  # an empty group
    assert "span" in both(_arrays([0, 2, 3]))  # not ending at n_sets
    assert "span" in both(_arrays([1, 2, 4]))  # not starting at 0
    both(_arrays([0, 1, 2, 3, 4, 4]))  # n_groups > n_sets
    a = _arrays([0, 2, 4])
    a["n_groups"] = 0  # sets without a group
    both(a)
    a = _arrays([0, 2, 4])
    a["scalars"][2] = 0
    assert "scalars[2]" in both(a)
    a = _arrays([0, 2, 4])
    a["scalars"] = None  # drawn on the device
    assert native.sm_agg_check(a)[0] == native.BGV_OK


def test_empty_batch_is_accepted(lib):
    from lodestar_amd import native
    out = np.zeros((1, 96), np.uint8)
    agg = native.BgvSmAgg(agg_sig96=out.ctypes.data)
    b = native.BgvSmBatch()
    assert lib.bgv_sm_agg_check(ctypes.byref(b), ctypes.byref(agg)) == native.BGV_OK
    assert lib.bgv_sm_agg_check(ctypes.byref(b), None) == native.BGV_E_INVALID_ARG  # agg is still required


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_addon_exports_the_aggregate_entries():
    from tools import build as B
    addon = B.build_addon()
    if addon is None:
        pytest.skip("node_api.h not found")
    script = f"""
const a = require({addon!r});
for (const k of ["verifySameMessageAggregate", "verifySameMessageAggregateSync"]) if (typeof a[k] !== "function") throw Error("missing " + k);
const v = require({os.path.join(ROOT, "lodestar_amd", "napi", "index.js")!r});
for (const c of [v.BlsGpuVerifier, v.BlsGpuSingleThreadVerifier])
  if (typeof c.prototype.verifyAndAggregateSameMessage !== "function") throw Error("no verifyAndAggregateSameMessage");
const calls = [{{sets: [1], message: Buffer.alloc(32)}}, {{sets: [2], message: Buffer.alloc(32), agg: {{}}}}, {{sets: [3], message: Buffer.alloc(32)}}];
const m = v.mergeSameMessage(calls);
if (JSON.stringify(m.groupOf) !== "[0,1,0]" || m.groups.length !== 2) throw Error("merge rule " + JSON.stringify(m.groupOf));
console.log("ok");
"""
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"
