"""The bitfield-expansion helpers (lodestar_amd/csrc/bits_expand.h) compiled
for the host in a stand-alone program (tests/native/hostcheck_bits.cpp): the
expansion over the length / byte-offset / pattern grid against a bit-by-bit
loop, the span checks, and the same program again under AddressSanitizer and
UBSan (every bitfield ends on the last byte of its heap block, so a load past
the end is a finding).  The program is never loaded into Python."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "hostcheck_bits.cpp")
GRID_CASES = 17 * 4 * 3 * 7  # lengths x byte offsets x list offsets x patterns (clean padding)


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck bits OK (\d+)", r.stdout)
    assert m, r.stdout
    return int(m.group(1))


def test_helpers_against_the_bit_by_bit_loop(tmp_path):
    exe = tmp_path / "hostcheck_bits"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    assert _run(exe) >= GRID_CASES


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hostcheck_bits_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), SRC])
    assert _run(exe) >= GRID_CASES


def test_kernels_go_through_the_same_helpers():
    """the kernels and the host check call the header's functions, not copies of them"""
    csrc = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
    kern = open(os.path.join(csrc, "bgv_bits.hip")).read()
    api = open(os.path.join(csrc, "bgv_api_bits.hip")).read()
    for fn in ("bits_src_check", "bits_src_word", "bits_src_entry", "bits_words", "bits_popc"):
        assert fn + "(" in kern, fn
    for fn in ("bits_src_check", "bits_src_word", "bits_popc"):
        assert fn + "(" in api, fn
