"""C ABI of same-message batches over committee bitfields (include/bgv.h
bgv_smb_batch, bgv_verify_same_message_bits, bgv_smb_check): exported symbols,
struct layout against a compiled sizeof / offsetof, every refusal of the
host-side contract check with the set or group it names, and batches that sit
on the bounds.  No compute calls here (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_verify_same_message_bits", "bgv_smb_check", "bgv_debug_same_message_bits")
X = 0xFFFFFFFF  # BGV_SRC_EXPLICIT
LISTS = [0, 512, 0, 4400]  # lists 1 and 3 are set


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
    fb = [f for f, _ in native.BgvSmbBatch._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu\\n", sizeof(bgv_smb_batch));']
    lines += [f'printf("%zu\\n", offsetof(bgv_smb_batch, {f}));' for f in fb]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == ctypes.sizeof(native.BgvSmbBatch)
    assert vals[1:] == [getattr(native.BgvSmbBatch, f).offset for f in fb]
    assert fb == ["n_sets", "n_groups", "group_offsets", "src", "bits", "bits_len", "pk_indices", "n_indices", "raw_pks", "n_raw",
                  "msgs", "sigs", "sig_len", "scalars", "on_device"]


def _arrays(src, bits=b"\x01" * 64, groups=None, n_indices=40, scalars=None):
    from lodestar_amd import native
    n = len(src)
    raw = bytes(bits)
    groups = groups or [0, n]
    return {"n_sets": n, "n_groups": len(groups) - 1, "group_offsets": np.array(groups, np.uint32),
            "src": np.array([tuple(s) for s in src], native.SET_SRC_DTYPE) if n else np.zeros(1, native.SET_SRC_DTYPE),
            "bits": np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(1, np.uint8), "bits_len": len(raw),
            "pk_indices": np.arange(max(n_indices, 1), dtype=np.uint32), "n_indices": n_indices,
            "msgs": np.zeros((len(groups) - 1, 32), np.uint8), "sigs": np.zeros((max(n, 1), 192), np.uint8),
            "sig_len": np.full(max(n, 1), 96, np.uint32), "scalars": scalars}


OK_SRC = [(1, 0, 512, 0), (3, 4399, 1, 63), (X, 0, 40, 0), (3, 7, 9, 62)]


def _check(src, **kw):
    from lodestar_amd import native
    return native.smb_check(_arrays(src, **kw), LISTS)


def test_batches_on_the_bounds_are_accepted(lib):
    from lodestar_amd import native
    assert _check(OK_SRC) == (native.BGV_OK, "")
    assert _check(OK_SRC, groups=[0, 1, 2, 3, 4])[0] == native.BGV_OK  # n_groups == n_sets
    assert _check(OK_SRC, groups=[0, 3, 4], scalars=np.array([1, 2**64 - 1, 5, 7], np.uint64))[0] == native.BGV_OK
    # two sets sharing one bitfield, windows of two lists
    assert _check([(1, 0, 16, 3), (3, 4000, 16, 3)], bits=bytes(3) + b"\xff\x7f")[0] == native.BGV_OK
    # an odd bits_off
    assert _check([(3, 100, 9, 61)], bits=bytes(61) + b"\x55\x01")[0] == native.BGV_OK
    # a window that is the whole list
    assert _check([(3, 0, 4400, 0)], bits=b"\xff" * 550)[0] == native.BGV_OK
    assert _check([(1, 0, 512, 1)], bits=b"\x00" + b"\xff" * 64)[0] == native.BGV_OK
    assert _check([(X, 39, 1, 0xFFFFFFFF)], bits=b"")[0] == native.BGV_OK  # explicit: bits_off is ignored
    assert _check([], groups=[0])[0] == native.BGV_OK  # n_sets == 0 succeeds


VIOLATIONS = [
    # the group rules of bgv_sma_check
    ("groups_not_spanning", dict(src=OK_SRC, groups=[0, 3]), "INVALID", "group_offsets must span"),
    ("groups_not_from_zero", dict(src=OK_SRC, groups=[1, 4]), "INVALID", "group_offsets must span"),
    ("groups_backwards", dict(src=OK_SRC, groups=[0, 3, 2, 4]), "INVALID", "group_offsets not monotone"),
    ("empty_group", dict(src=OK_SRC, groups=[0, 2, 2, 4]), "INVALID", "group 1 is empty"),
    ("more_groups_than_sets", dict(src=OK_SRC[:2], groups=[0, 1, 2, 2]), "INVALID", "n_groups 3 > n_sets 2"),
    ("zero_scalar", dict(src=OK_SRC, scalars=np.array([1, 2, 0, 4], np.uint64)), "INVALID", "scalars[2]"),
    # the source rules of bgv_bits_check
    ("unset_list", dict(src=[(2, 0, 1, 0)]), "INVALID", "list 2"),
    ("list_id_past_the_lists", dict(src=OK_SRC[:1] + [(8, 0, 1, 0)]), "INVALID", "set 1"),
    ("off_len_wraps_32_bits", dict(src=[(1, 0xFFFFFFF0, 0x20, 0)]), "INVALID", "set 0"),
    ("off_len_past_list", dict(src=OK_SRC[:1] + [(1, 1, 512, 0)]), "INVALID", "set 1"),
    ("explicit_past_n_indices", dict(src=[(X, 1, 40, 0)]), "INVALID", "set 0"),
    ("explicit_wraps_32_bits", dict(src=[(X, 0xFFFFFFF0, 0x20, 0)]), "INVALID", "set 0"),
    ("bits_one_byte_past", dict(src=OK_SRC[:2] + [(3, 0, 9, 63)]), "INVALID", "set 2"),
    ("bits_off_wraps", dict(src=[(3, 0, 8, 0xFFFFFFFF)]), "INVALID", "set 0"),
    ("padding_bit", dict(src=[(1, 3, 5, 0)], bits=b"\x3f"), "INVALID", "padding"),
    ("padding_bit_second_set", dict(src=[(1, 0, 8, 0), (1, 0, 9, 1)], bits=b"\x01\x01\x80"), "INVALID", "set 1"),
    ("all_zero_bitfield", dict(src=OK_SRC[:1] + [(3, 0, 16, 0)], bits=bytes(64)), "EMPTY", "EMPTY_AGGREGATE_ARRAY (set 0)"),
    ("empty_second_set", dict(src=[(1, 0, 8, 0), (1, 0, 8, 1)], bits=b"\x01\x00"), "EMPTY", "EMPTY_AGGREGATE_ARRAY (set 1)"),
    ("explicit_len_zero", dict(src=OK_SRC[:1] + [(X, 0, 0, 0)], bits=b"\xff" * 64), "EMPTY", "EMPTY_AGGREGATE_ARRAY (set 1)"),
]


@pytest.mark.parametrize("name,kw,status,text", VIOLATIONS, ids=[v[0] for v in VIOLATIONS])
def test_contract_violations_are_refused_without_a_device(lib, name, kw, status, text):
    from lodestar_amd import native
    st, msg = _check(**kw)
    assert st == (native.BGV_E_INVALID_ARG if status == "INVALID" else native.BGV_E_EMPTY_SET), (name, st, msg)
    assert text in msg, (name, msg)


def test_key_total_must_fit_32_bits(lib):
    """three explicit sets over the same 2^31 announced indices: 3 * 2^31 keys (the check reads no index)"""
    from lodestar_amd import native
    a = _arrays([(X, 0, 1 << 31, 0)] * 3)
    a["n_indices"] = 1 << 31
    st, msg = native.smb_check(a, LISTS)
    assert st == native.BGV_E_INVALID_ARG and "32 bits" in msg, msg


def test_missing_arrays_and_null_arguments(lib):
    from lodestar_amd import native
    assert lib.bgv_smb_check(None, None) == native.BGV_E_INVALID_ARG
    b = native.make_smb_batch(_arrays(OK_SRC))
    assert lib.bgv_smb_check(ctypes.byref(b), None) == native.BGV_E_INVALID_ARG  # no list lengths
    for missing in ("group_offsets", "src", "msgs", "sigs", "sig_len", "bits", "pk_indices"):
        a = _arrays(OK_SRC)
        a[missing] = None
        st, msg = native.smb_check(a, LISTS)
        assert st == native.BGV_E_INVALID_ARG and ("missing" in msg or "NULL" in msg), (missing, msg)
    a = _arrays(OK_SRC)
    a["n_raw"] = 1  # raw rows announced, none given
    assert native.smb_check(a, LISTS)[0] == native.BGV_E_INVALID_ARG
    a = _arrays(OK_SRC)
    a["n_groups"] = 0
    st, msg = native.smb_check(a, LISTS)
    assert st == native.BGV_E_INVALID_ARG and "without a group" in msg


def test_on_device_batch_is_not_read(lib):
    """on_device: the arrays live in HBM, the host check must not touch them (the addresses here are not mapped)"""
    from lodestar_amd import native
    b = native.BgvSmbBatch()
    b.n_sets, b.n_groups, b.on_device, b.bits_len, b.n_indices = 4, 1, 1, 64, 40
    for f in ("group_offsets", "src", "bits", "pk_indices", "msgs", "sigs", "sig_len", "scalars"):
        setattr(b, f, 0x10)
    ll = np.array(LISTS + [0] * 4, np.uint32)
    assert lib.bgv_smb_check(ctypes.byref(b), ll.ctypes.data) == native.BGV_OK
    b.src = None  # the argument check still holds
    assert lib.bgv_smb_check(ctypes.byref(b), ll.ctypes.data) == native.BGV_E_INVALID_ARG
    assert native.smb_check(_arrays(OK_SRC, groups=[0, 3]), LISTS, on_device=True)[0] == native.BGV_OK
