"""Committee signature sets through the N-API addon, driven from Node
(tests/js/bits_test.js): the encoder and the routing rule on the host, and on
the GPU both Node classes on a 40-set mixed batch against the explicit-index
call on the same sets."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "bits_test.js")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_js_encoder_routing_and_addon_entries():
    """tests/js/bits_test.js --host: encodeJobsBits against intersectValues, the routing rule, the caller-side checks"""
    from tools import build as B
    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    r = subprocess.run([NODE, SCRIPT, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits host checks OK" in r.stdout


@pytest.mark.gpu
def test_committee_sets_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys = 600
    rng = np.random.default_rng(23)
    lists = {1: rng.permutation(n_keys).astype(np.uint32), 4: rng.permutation(n_keys)[:512].astype(np.uint32)}
    jobs, flat = [], []
    sizes = [3, 1, 5, 4, 2, 6, 3, 5, 4, 7]  # 40 sets in 10 jobs
    for j, size in enumerate(sizes):
        job = []
        for k in range(size):
            kind = (j + k) % 4
            root = hashlib.sha256(b"napi bits %d %d" % (j, k)).digest().hex()
            if kind == 0:
                s = {"type": "single", "indices": [int(rng.integers(n_keys))]}
            elif kind == 1:
                s = {"type": "aggregate", "indices": [int(x) for x in rng.integers(0, n_keys, size=int(rng.integers(2, 40)))]}
            else:
                lid = 1 if kind == 2 else 4
                length = int(rng.choice([9, 64, 128, 200, 512]))
                off = int(rng.integers(0, lists[lid].size - length + 1))
                b = rng.random(length) < 0.7
                b[0] = True
                s = {"type": "committee", "committee": {"list": lid, "offset": off, "length": length},
                     "bits": np.packbits(b, bitorder="little").tobytes().hex()}
                s["indices"] = [int(x) for x in lists[lid][off:off + length][b]]  # what the set stands for (signing only)
            s["signingRoot"] = root
            job.append(s)
            flat.append(s)
        jobs.append(job)
    n = len(flat)
    assert n == 40
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E424954)
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
        if s["type"] == "committee":
            del s["indices"]
    bad_job = 5
    victim = next(s for s in jobs[bad_job] if s["type"] == "committee")
    victim["signature"] = jobs[2][0]["signature"]  # another set's signature
    expected = [j != bad_job for j in range(len(jobs))]
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "jobs.json").write_text(json.dumps({"lists": {str(k): v.tolist() for k, v in lists.items()}, "jobs": jobs,
                                                    "expected": expected, "bad_job": bad_job}))
    r = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits test OK" in r.stdout
