"""C ABI of verification over committee bitfields (include/bgv.h
bgv_bits_batch, bgv_verify_bits, bgv_index_list_set): exported symbols, struct
sizes and layout against a compiled sizeof / offsetof, every refusal of the
host-side contract check, and a batch that sits exactly on each bound.  No
compute calls here (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_index_list_set", "bgv_index_list_len", "bgv_verify_bits", "bgv_bits_check", "bgv_debug_bits_expand")
X = 0xFFFFFFFF  # BGV_SRC_EXPLICIT


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


def test_struct_sizes_and_layout_match_ctypes(tmp_path):
    from lodestar_amd import native
    fb = [f for f, _ in native.BgvBitsBatch._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bgv.h"', "int main(void){",
             'printf("%zu %zu %d %u\\n", sizeof(bgv_set_src), sizeof(bgv_bits_batch), BGV_MAX_INDEX_LISTS, BGV_SRC_EXPLICIT);']
    lines += [f'printf("%zu\\n", offsetof(bgv_bits_batch, {f}));' for f in fb]
    lines += [f'printf("%zu\\n", offsetof(bgv_set_src, {f}));' for f in ("list", "off", "len", "bits_off")]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == 16 == native.SET_SRC_DTYPE.itemsize
    assert vals[1] == ctypes.sizeof(native.BgvBitsBatch)
    assert vals[2] == 8 == native.MAX_INDEX_LISTS
    assert vals[3] == X == native.SRC_EXPLICIT
    assert vals[4:4 + len(fb)] == [getattr(native.BgvBitsBatch, f).offset for f in fb]
    assert vals[4 + len(fb):] == [native.SET_SRC_DTYPE.fields[f][1] for f in ("list", "off", "len", "bits_off")]
    assert fb == ["n_sets", "n_jobs", "job_offsets", "src", "bits", "bits_len", "pk_indices", "n_indices", "raw_pks", "n_raw",
                  "msgs", "sigs", "sig_len", "scalars", "on_device"]


LISTS = [0, 512, 0, 4400]  # lists 1 and 3 are set


def _arrays(src, bits=b"\x01" * 64, jobs=None, n_indices=40):
    from lodestar_amd import native
    n = len(src)
    raw = bytes(bits)
    return {"n_sets": n, "n_jobs": len(jobs) - 1 if jobs else 1, "job_offsets": np.array(jobs or [0, n], np.uint32),
            "src": np.array([tuple(s) for s in src], native.SET_SRC_DTYPE),
            "bits": np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(1, np.uint8), "bits_len": len(raw),
            "pk_indices": np.arange(max(n_indices, 1), dtype=np.uint32), "n_indices": n_indices,
            "msgs": np.zeros((n, 32), np.uint8), "sigs": np.zeros((n, 192), np.uint8), "sig_len": np.full(n, 96, np.uint32),
            "scalars": None}


OK_SRC = [(1, 0, 512, 0), (3, 4399, 1, 63), (X, 0, 40, 0), (3, 7, 9, 62)]


def _check(src, **kw):
    from lodestar_amd import native
    return native.bits_check(_arrays(src, **kw), LISTS)


def test_a_batch_on_every_bound_is_accepted(lib):
    """off + len == the list's length, the last bitfield on the last byte of bits, every explicit index used"""
    from lodestar_amd import native
    assert _check(OK_SRC) == (native.BGV_OK, "")
    assert _check(OK_SRC, jobs=[0, 1, 1, 4])[0] == native.BGV_OK  # an empty job is legal, as for bgv_batch
    assert _check([(3, 0, 4400, 0)], bits=b"\x01" + bytes(549))[0] == native.BGV_OK  # the whole list, 550 bytes
    assert _check([(1, 3, 5, 0)], bits=b"\x1f")[0] == native.BGV_OK  # all five bits, clean padding
    assert _check([(X, 39, 1, 0xFFFFFFFF)], bits=b"")[0] == native.BGV_OK  # explicit: bits_off is ignored


VIOLATIONS = [
    ("off_len_wraps_32_bits", dict(src=[(1, 0xFFFFFFF0, 0x20, 0)]), "INVALID", "set 0"),
    ("off_len_past_list", dict(src=OK_SRC[:1] + [(1, 1, 512, 0)]), "INVALID", "set 1"),
    ("explicit_past_n_indices", dict(src=[(X, 1, 40, 0)]), "INVALID", "set 0"),
    ("explicit_wraps_32_bits", dict(src=[(X, 0xFFFFFFF0, 0x20, 0)]), "INVALID", "set 0"),
    ("bits_one_byte_past", dict(src=OK_SRC[:2] + [(3, 0, 9, 63)]), "INVALID", "set 2"),  # 63 + 2 == bits_len + 1
    ("bits_off_wraps", dict(src=[(3, 0, 8, 0xFFFFFFFF)]), "INVALID", "set 0"),
    ("padding_bit", dict(src=[(1, 3, 5, 0)], bits=b"\x3f"), "INVALID", "padding"),
    ("padding_bit_top", dict(src=[(1, 0, 9, 0)], bits=b"\x01\x80"), "INVALID", "set 0"),
    ("all_zero_bitfield", dict(src=OK_SRC[:1] + [(3, 0, 16, 0)], bits=bytes(64)), "EMPTY", "set 0"),
    ("empty_second_set", dict(src=[(1, 0, 8, 0), (1, 0, 8, 1)], bits=b"\x01\x00"), "EMPTY", "EMPTY_AGGREGATE_ARRAY (set 1)"),
    ("len_zero_list_set", dict(src=[(1, 0, 0, 0)]), "EMPTY", "set 0"),
    ("explicit_len_zero", dict(src=[(X, 0, 0, 0)]), "EMPTY", "set 0"),
    ("unset_list", dict(src=[(2, 0, 1, 0)]), "INVALID", "list 2"),
    ("list_id_past_the_lists", dict(src=[(8, 0, 1, 0)]), "INVALID", "set 0"),
    ("job_offsets_not_spanning", dict(src=OK_SRC, jobs=[0, 3]), "INVALID", "job_offsets must span"),
    ("job_offsets_not_from_zero", dict(src=OK_SRC, jobs=[1, 4]), "INVALID", "job_offsets must span"),
    ("job_offsets_backwards", dict(src=OK_SRC, jobs=[0, 3, 2, 4]), "INVALID", "job_offsets not monotone"),
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
    a = _arrays([(X, 0, 1 << 31, 0)] * 3, n_indices=40)
    a["n_indices"] = 1 << 31
    st, msg = native.bits_check(a, LISTS)
    assert st == native.BGV_E_INVALID_ARG and "32 bits" in msg, msg
    a = _arrays([(X, 0, 1 << 31, 0), (X, 0, (1 << 31) - 1, 0)], n_indices=40)  # 2^32 - 1 keys fit
    a["n_indices"] = 1 << 31
    assert native.bits_check(a, LISTS)[0] == native.BGV_OK


def test_missing_arrays_and_null_arguments(lib):
    from lodestar_amd import native
    assert lib.bgv_bits_check(None, None) == native.BGV_E_INVALID_ARG
    b = native.make_bits_batch(_arrays(OK_SRC))
    assert lib.bgv_bits_check(ctypes.byref(b), None) == native.BGV_E_INVALID_ARG  # no list lengths
    for missing in ("job_offsets", "src", "msgs", "sigs", "sig_len", "bits", "pk_indices"):
        a = _arrays(OK_SRC)
        a[missing] = None
        st, msg = native.bits_check(a, LISTS)
        assert st == native.BGV_E_INVALID_ARG and ("missing" in msg or "NULL" in msg), (missing, msg)
    a = _arrays(OK_SRC)
    a["n_raw"] = 1  # raw rows announced, none given
    assert native.bits_check(a, LISTS)[0] == native.BGV_E_INVALID_ARG


def test_on_device_batch_is_not_read(lib):
    """on_device: the arrays live in HBM, the host check must not touch them (the addresses here are not mapped)"""
    from lodestar_amd import native
    b = native.BgvBitsBatch()
    b.n_sets, b.n_jobs, b.on_device, b.bits_len, b.n_indices = 4, 1, 1, 64, 40
    for f in ("job_offsets", "src", "bits", "pk_indices", "msgs", "sigs", "sig_len", "scalars"):
        setattr(b, f, 0x10)
    ll = np.array(LISTS + [0] * 4, np.uint32)
    assert lib.bgv_bits_check(ctypes.byref(b), ll.ctypes.data) == native.BGV_OK
    b.src = None  # the argument check still holds
    assert lib.bgv_bits_check(ctypes.byref(b), ll.ctypes.data) == native.BGV_E_INVALID_ARG
