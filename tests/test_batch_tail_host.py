"""The batch-first tail compiled for the host in a
stand-alone program (tests/native/hostcheck_batch_tail.cpp) over the headers
the kernels are built from: the fold over all slices followed by one
recurrence equals the product of the per-job chains (1, 2, 8, 9 and 65 jobs,
a two-slice job, a rejected and an empty job), the window sums followed by one
Horner equal the sum of the per-job sums (a rejected job, S and -S), and the
one pair equals the product of the per-job pairs after the final
exponentiation.  The same program again under AddressSanitizer and UBSan.
The program is never loaded into Python."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "hostcheck_batch_tail.cpp")
CHECKS = 5 + 4 + 1  # chain identity per job count, S_batch cases, the pair


def slice_sets():
    """the slice size the library is built with (bgv_api.hip BGV_STEPS_SLICE)"""
    api = open(os.path.join(ROOT, "lodestar_amd", "csrc", "bgv_api.hip")).read()
    return int(re.search(r"#define BGV_STEPS_SLICE (\d+)", api).group(1))


def _run(exe, g):
    r = subprocess.run([str(exe), str(g)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck batch_tail OK (\d+)", r.stdout)
    assert m, r.stdout
    return int(m.group(1))


def test_batch_tail_against_the_per_job_tail(tmp_path):
    exe = tmp_path / "hostcheck_batch_tail"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", str(exe), SRC])
    for g in (3, slice_sets()):  # a small slice size (most jobs of one slice, some of two) and the built one
        assert _run(exe, g) == CHECKS


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hostcheck_batch_tail_san"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), SRC])
    assert _run(exe, 3) == CHECKS  # ~10 s instrumented


def test_launchers_and_host_check_share_the_shapes():
    """the launchers, the allocation and the host check size their trees through batch_tail.h, not copies of it"""
    csrc = os.path.join(ROOT, "lodestar_amd", "csrc")
    for name, fns in (("bgv_kernels.hip", ("tail_groups(", "tail_region1(")), ("bgv_tail.hip", ("tail_groups(", "tail_region1(")),
                      ("bgv_api.hip", ("tail_entries(",))):
        text = open(os.path.join(csrc, name)).read()
        for fn in fns:
            assert fn in text, (name, fn)
    host = open(SRC).read()
    assert "batch_tail.h" in host and "miller_chain(" in host
