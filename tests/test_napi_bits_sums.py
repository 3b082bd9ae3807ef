"""Committee sets over index lists with resident prefix sums through the N-API
addon, driven from Node (tests/js/bits_sums_test.js): one committee batch
through a verifier built with {sums: true} and through one without; the
verdicts agree and bitsPathStats shows the complement path on the first."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "bits_sums_test.js")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_addon_has_the_sums_entries():
    from tools import build as B
    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    r = subprocess.run([NODE, SCRIPT, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits sums host checks OK" in r.stdout


@pytest.mark.gpu
def test_committee_batch_with_and_without_sums_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys = 600
    rng = np.random.default_rng(29)
    lists = {1: rng.permutation(n_keys).astype(np.uint32), 4: rng.permutation(n_keys)[:512].astype(np.uint32)}
    jobs, flat = [], []
    n_complement = 0
    for j, size in enumerate([3, 1, 4, 2, 5, 3]):  # 18 sets in 6 jobs
        job = []
        for k in range(size):
            lid = 1 if (j + k) % 2 else 4
            length = int(rng.choice([9, 64, 128, 512]))
            off = int(rng.integers(0, lists[lid].size - length + 1))
            b = rng.random(length) < [1.0, 0.99, 0.5][(j + 2 * k) % 3]
            b[0] = True
            pop = int(b.sum())
            n_complement += int((length - pop) + 2 < pop)
            job.append({"committee": {"list": lid, "offset": off, "length": length},
                        "bits": np.packbits(b, bitorder="little").tobytes().hex(),
                        "indices": [int(x) for x in lists[lid][off:off + length][b]],  # what the set stands for (signing only)
                        "signingRoot": hashlib.sha256(b"napi sums %d %d" % (j, k)).digest().hex()})
            flat.append(job[-1])
        jobs.append(job)
    n = len(flat)
    assert n == 18 and 6 <= n_complement < n
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E53554D)
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
        del s["indices"]
    bad_job = 4
    jobs[bad_job][1]["signature"] = jobs[0][0]["signature"]  # another set's signature
    expected = [j != bad_job for j in range(len(jobs))]
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "jobs.json").write_text(json.dumps({"lists": {str(k): v.tolist() for k, v in lists.items()}, "jobs": jobs,
                                                    "expected": expected, "n_complement": n_complement}))
    r = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits sums test OK" in r.stdout
