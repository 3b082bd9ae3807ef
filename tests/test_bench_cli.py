"""bench.py's command line: a plain run does the timed steps and nothing
else, --full is where the other measurements live, and --dump-outputs writes
what the last timed step returned (the per-block verdicts) as float32 .npy.
The GPU case runs a 16-block segment (1,568 sets, four contexts in flight)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("one_in_flight", "c2_gossip_latency_ms", "c5_faulted_c4", "c4_host_resident", "c4_epoch_slice", "mixed_sizes",
             "strong_shard_projection", "reserved_device", "weak_scaling")


def test_options_are_offered():
    out = subprocess.check_output([sys.executable, BENCH, "--help"], cwd=ROOT).decode()
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out, opt


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_the_verdicts(tmp_path):
    blocks, steps = 16, 3
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--blocks", str(blocks),
                        "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j["metric"] == "BLS signature sets verified/sec (node)" and j["unit"] == "sets/s"
    assert j["higher_is_better"] is True and j["dtype"] == "u32"
    assert j["steps"] == steps and j["full"] is False and j["verified"] is True
    assert j["config"]["sets"] == blocks * 98
    # value and ms_per_step describe the same timed region (both rounded in the line)
    assert j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(blocks * 98 / (j["ms_per_step"] * 1e-3), rel=1e-2)
    for k in FULL_ONLY:
        assert k not in j, k
    assert j["roofline"] is None and j["cpu_baseline"] is None
    assert sorted(os.listdir(d)) == ["job_results.npy"]
    v = np.load(d / "job_results.npy")
    assert v.dtype == np.float32 and v.shape == (blocks,)
    assert (v == 1).all()
