"""Resident key sums for bitfield sets, the part that needs no GPU
(include/bgv.h bgv_index_list_sums ... bgv_bits_plan): exported symbols, the
complement rule of bgv_bits_plan against a numpy restatement over the length /
participation grid, the gathered-key total of a mixed batch, every refusal of
bgv_bits_check refused by the plan too, and an on-device batch left unread."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_bits_abi import LISTS, VIOLATIONS, _arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgv_index_list_sums", "bgv_index_list_has_sums", "bgv_bits_path_stats", "bgv_bits_plan", "bgv_debug_bits_keys",
       "bgv_debug_index_list_sums", "bgv_index_list_sums_ms")
X = 0xFFFFFFFF
LENS = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 127, 128, 512, 2049]
LIST_LEN = [4400, 4400, 0, 512]  # lists 0, 1 and 3 are set
HAS_SUMS = [1, 0, 0, 1]          # list 1 has none


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


def rule(has_sums, length, pop):
    """the rule restated: window (two reads, one addition = two keys) + absent members < present members"""
    return bool(has_sums) and (length - pop) + 2 < pop


def pops_for(length):
    """pop on the boundary absent + 2 == pop and one either side, all ones, and all but one"""
    out = {length, length - 1}
    if (length + 2) % 2 == 0:
        b = (length + 2) // 2  # absent + 2 == pop
        out |= {b - 1, b, b + 1}
    else:
        out |= {(length + 2) // 2, (length + 2) // 2 + 1}  # either side of the (fractional) boundary
    return sorted(p for p in out if 1 <= p <= length)


class Mix:
    def __init__(self):
        self.src, self.bits, self.want_path, self.want_gather = [], bytearray(), [], 0

    def add(self, lst, off, b, bits_off=None):
        length, pop = len(b), int(np.count_nonzero(b))
        if bits_off is None:
            bits_off = len(self.bits)
            self.bits += np.packbits(b, bitorder="little").tobytes()
        self.src.append((lst, off, length, bits_off))
        cm = rule(HAS_SUMS[lst], length, pop)
        self.want_path.append(int(cm))
        self.want_gather += length - pop if cm else pop
        return bits_off

    def explicit(self, off, n):
        self.src.append((X, off, n, 0))
        self.want_path.append(0)
        self.want_gather += n


@pytest.fixture(scope="module")
def mix():
    rng = np.random.default_rng(5)
    m = Mix()
    for length in LENS:
        for pop in pops_for(length):
            b = np.zeros(length, bool)
            b[rng.permutation(length)[:pop]] = True
            for lst in (0, 1) if length > 512 else (0, 1, 3):
                m.add(lst, int(rng.integers(0, LIST_LEN[lst] - length + 1)), b)
        if length % 8 and length > 1:  # one bit clear in the last partial byte
            b = np.ones(length, bool)
            b[length - 1 - int(rng.integers(0, min(length % 8, length)))] = False
            m.add(0, 0, b)
    m.explicit(0, 40)
    m.explicit(39, 1)
    # two sets over one bitfield, windows of a list with sums and of one without
    b = np.ones(128, bool)
    b[[5, 77]] = False
    at = m.add(0, 100, b)
    m.add(1, 300, b, bits_off=at)
    m.add(3, 384, b, bits_off=at)
    return m


def test_boundary_cases_are_in_the_grid():
    for length in LENS:
        ps = pops_for(length)
        assert length in ps
        assert any(rule(1, length, p) for p in ps) == (length >= 3)
        assert any(not rule(1, length, p) for p in ps)
        if length % 2 == 0 and length >= 2:
            b = (length + 2) // 2
            assert (length - b) + 2 == b and not rule(1, length, b) and (b + 1 > length or rule(1, length, b + 1))


def test_plan_matches_the_rule_and_counts_the_gathered_keys(lib, mix):
    from lodestar_amd import native
    a = _arrays(mix.src, bits=bytes(mix.bits), jobs=[0, 7, len(mix.src)])
    st, msg, path, gathered = native.bits_plan(a, LIST_LEN, HAS_SUMS)
    assert st == native.BGV_OK, msg
    assert path.tolist() == mix.want_path
    assert gathered == mix.want_gather
    assert 0 < sum(mix.want_path) < len(mix.src)
    # the shared bitfield: complement over the lists with sums, direct over the one without
    assert mix.want_path[-3:] == [1, 0, 1]
    # no sums anywhere (or none announced): every set direct, every participating key gathered
    total = sum(int(np.count_nonzero(np.unpackbits(np.frombuffer(bytes(mix.bits), np.uint8), bitorder="little")[8 * bo:8 * bo + ln]))
                if lst != X else ln for lst, _, ln, bo in mix.src)
    for hs in ([0] * 8, None):
        st, _, path, gathered = native.bits_plan(a, LIST_LEN, hs)
        assert st == native.BGV_OK and not path.any() and gathered == total
    # path may be NULL, keys_gathered too
    b = native.make_bits_batch(a)
    ll = np.array(LIST_LEN + [0] * 4, np.uint32)
    hs = np.array(HAS_SUMS + [0] * 4, np.uint8)
    kg = ctypes.c_uint64()
    assert lib.bgv_bits_plan(ctypes.byref(b), ll.ctypes.data, hs.ctypes.data, None, ctypes.byref(kg)) == native.BGV_OK
    assert kg.value == mix.want_gather
    assert lib.bgv_bits_plan(ctypes.byref(b), ll.ctypes.data, hs.ctypes.data, None, None) == native.BGV_OK


def test_padding_bits_are_neither_present_nor_absent(lib):
    """len 5, all five bits: pop 5, absent 0 whatever sits above len in the byte (which the check refuses anyway)"""
    from lodestar_amd import native
    a = _arrays([(0, 3, 5, 0), (0, 3, 5, 1), (0, 3, 5, 2)], bits=b"\x1f\x0f\x07")
    st, _, path, gathered = native.bits_plan(a, LIST_LEN, HAS_SUMS)
    assert st == native.BGV_OK and path.tolist() == [1, 1, 0] and gathered == 0 + 1 + 3


@pytest.mark.parametrize("name,kw,status,text", VIOLATIONS, ids=[v[0] for v in VIOLATIONS])
def test_every_refusal_of_the_check_is_a_refusal_of_the_plan(lib, name, kw, status, text):
    from lodestar_amd import native
    a = _arrays(**kw)
    want = native.bits_check(a, LISTS)
    st, msg, _, gathered = native.bits_plan(a, LISTS, [0, 1, 0, 1])
    assert (st, msg) == want
    assert st == (native.BGV_E_INVALID_ARG if status == "INVALID" else native.BGV_E_EMPTY_SET) and text in msg
    assert gathered == 0


def test_on_device_batch_is_not_read(lib):
    """the addresses here are not mapped: touching them would fault"""
    from lodestar_amd import native
    b = native.BgvBitsBatch()
    b.n_sets, b.n_jobs, b.on_device, b.bits_len, b.n_indices = 4, 1, 1, 64, 40
    for f in ("job_offsets", "src", "bits", "pk_indices", "msgs", "sigs", "sig_len", "scalars"):
        setattr(b, f, 0x10)
    ll = np.array(LIST_LEN + [0] * 4, np.uint32)
    hs = np.array(HAS_SUMS + [0] * 4, np.uint8)
    path = np.full(4, 7, np.uint8)
    kg = ctypes.c_uint64(99)
    assert lib.bgv_bits_plan(ctypes.byref(b), ll.ctypes.data, hs.ctypes.data, path.ctypes.data, ctypes.byref(kg)) == native.BGV_OK
    assert kg.value == 0 and path.tolist() == [7] * 4
    b.src = None  # the argument check still holds
    assert lib.bgv_bits_plan(ctypes.byref(b), ll.ctypes.data, hs.ctypes.data, None, None) == native.BGV_E_INVALID_ARG
    assert lib.bgv_bits_plan(None, ll.ctypes.data, hs.ctypes.data, None, None) == native.BGV_E_INVALID_ARG


def test_host_check_and_kernels_share_the_rule():
    """one function decides the path: the host check and k_bits_count call it, no copy of the inequality elsewhere"""
    csrc = os.path.join(ROOT, "lodestar_amd", "csrc")
    hdr = open(os.path.join(csrc, "bits_expand.h")).read()
    kern = open(os.path.join(csrc, "bgv_bits.hip")).read()
    api = open(os.path.join(csrc, "bgv_api_bits.hip")).read()
    assert "BGV_HD bool bits_complement(" in hdr and "+ 2u < pop" in hdr
    for src in (kern, api):
        assert "bits_src_complement(" in src
        assert "2u < pop" not in src and "+ 2 <" not in src
    assert "bits_gather_word(" in kern
    # the tile sizes of the scan are named powers of two at the top of its unit
    sums = open(os.path.join(csrc, "bgv_sums.hip")).read()
    assert "constexpr uint32_t SUMS_TILE = 64;" in sums and "constexpr uint32_t SUMS_TILE2 = 64;" in sums
    from tools import build
    assert "bgv_sums.hip" in build.SOURCES


# ---- the helpers compiled for the host in a stand-alone program (never loaded into Python)
HOSTCHECK = os.path.join(ROOT, "tests", "native", "hostcheck_bits_sums.cpp")


def _run_hostcheck(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "hostcheck bits sums OK" in r.stdout, r.stdout
    return int(r.stdout.split()[-1])


def test_complement_helpers_against_the_bit_by_bit_loop(tmp_path):
    exe = tmp_path / "hostcheck_bits_sums"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), HOSTCHECK])
    assert _run_hostcheck(exe) >= 18 * 4 * 8


def test_complement_helpers_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hostcheck_bits_sums_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), HOSTCHECK])
    assert _run_hostcheck(exe) >= 18 * 4 * 8
