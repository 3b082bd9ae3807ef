"""The per-step line products (lodestar_amd/csrc/pairing.h miller_step_lines,
miller_chain and the slicing helpers; kernels k_miller_steps and k_job_chain)
compiled for the host in a stand-alone program (tests/native/hostcheck_steps.cpp):
for the job sizes 1, 2, 3, G-1, G, G+1 and 2G+1 the step products followed by
the chain equal the product of the two-pair items, a rejected middle set is
left out and gives 1 at the job's first set, and the slices cover a ragged
batch with empty jobs.  The same program again under AddressSanitizer and
UBSan.  The program is never loaded into Python."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "hostcheck_steps.cpp")


def slice_sets():
    """the slice size the library is built with (bgv_api.hip BGV_STEPS_SLICE)"""
    api = open(os.path.join(ROOT, "lodestar_amd", "csrc", "bgv_api.hip")).read()
    return int(re.search(r"#define BGV_STEPS_SLICE (\d+)", api).group(1))


def _run(exe, gs):
    r = subprocess.run([str(exe)] + [str(g) for g in gs], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck steps OK (\d+)", r.stdout)
    assert m, r.stdout
    return int(m.group(1))


def test_steps_and_chain_against_the_item_loop(tmp_path):
    exe = tmp_path / "hostcheck_steps"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", str(exe), SRC])
    gs = [4, 5, slice_sets()]  # an even, an odd and the built slice size
    assert _run(exe, gs) >= len(gs) * 7 * 3


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hostcheck_steps_san"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), SRC])
    gs = [5]  # jobs of 1 .. 11 sets: line pairs, odd tails and up to three slices (a few seconds instrumented)
    assert _run(exe, gs) >= len(gs) * 7 * 3


def test_kernels_go_through_the_same_helpers():
    """the kernels and the host check call the header's functions, not copies of them"""
    csrc = os.path.join(ROOT, "lodestar_amd", "csrc")
    miller = open(os.path.join(csrc, "bgv_miller.hip")).read()
    kern = open(os.path.join(csrc, "bgv_kernels.hip")).read()
    for fn in ("miller_step_lines", "miller_item_sets", "miller_step_is_add"):
        assert fn + "(" in miller, fn
    assert "miller_item_count(" in kern
    assert "miller_job_rejected_pk(" in open(os.path.join(csrc, "bgv_tail.hip")).read()
