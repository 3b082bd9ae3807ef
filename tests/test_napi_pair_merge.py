"""One Miller pair per distinct signing root of a job through the N-API addon,
driven from Node (tests/js/pair_merge_test.js): a 256-set, 4-job batch with 16
distinct roots on a context in the layout that merges reports the classes as
its pairs with pairMerge on and every set with it off, the same verdicts either
way, and the pool feeds its two counters."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "pair_merge_test.js")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_repeated_roots_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys, n, n_jobs = 600, 256, 4
    rng = np.random.default_rng(37)
    roots = [hashlib.sha256(b"napi pair merge %d" % k).digest() for k in range(16)]
    which = rng.permutation(np.repeat(np.arange(16), n // 16))  # 16 sets per root, across the jobs
    flat = [{"indices": [int(x) for x in rng.integers(0, n_keys, size=int(rng.integers(1, 5)))],
             "signingRoot": roots[int(which[i])].hex()} for i in range(n)]
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E50414D)
        table = d.pubkeys_get(0, n_keys)
        po = np.concatenate([[0], np.cumsum([len(s["indices"]) for s in flat])]).astype(np.uint32)
        arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po,
                  "pk_indices": np.array([x for s in flat for x in s["indices"]], np.uint32),
                  "msgs": np.stack([np.frombuffer(bytes.fromhex(s["signingRoot"]), np.uint8) for s in flat])}
        sigs = np.zeros((n, 192), np.uint8)
        d.gen_sign(arrays, sigs)
    finally:
        d.close()
    for i, s in enumerate(flat):
        s["signature"] = sigs[i, :96].tobytes().hex()
    per = n // n_jobs
    jobs = [flat[k * per:(k + 1) * per] for k in range(n_jobs)]
    pairs = sum(len({s["signingRoot"] for s in j}) for j in jobs)  # a root in two jobs is two classes
    assert 16 < pairs <= 64
    bad_job = 2
    jobs[bad_job][5] = {**jobs[bad_job][5], "signature": jobs[0][0]["signature"]}  # another set's signature
    expected = [j != bad_job for j in range(n_jobs)]
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "jobs.json").write_text(json.dumps({"jobs": jobs, "expected": expected, "pairs": pairs}))
    r = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pair merge test OK" in r.stdout
