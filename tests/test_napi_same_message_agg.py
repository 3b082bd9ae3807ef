"""verifyAggregateSetsSameMessage through the N-API addon, driven from Node
(tests/js/same_message_agg_test.js): three calls at once, two batchable and one
not, one bad signature; per-call, per-set results."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_aggregate_same_message_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys = 64
    m1, m2 = hashlib.sha256(b"napi same message agg 1").digest(), hashlib.sha256(b"napi same message agg 2").digest()
    rng = np.random.default_rng(11)
    shape = [(20, m1, True), (20, m1, True), (5, m2, False)]
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E415041)
        table = d.pubkeys_get(0, n_keys)
        calls = []
        for n, m, batchable in shape:
            keys = [[int(x) for x in rng.integers(0, n_keys, size=int(c))] for c in rng.choice([1, 2, 33, 40], size=n)]
            po = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32)
            arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po,
                      "pk_indices": np.array([x for k in keys for x in k], np.uint32),
                      "msgs": np.stack([np.frombuffer(m, np.uint8)] * n)}
            sigs = np.zeros((n, 192), np.uint8)
            d.gen_sign(arrays, sigs)
            calls.append({"message": m.hex(), "batchable": batchable, "expected": [True] * n,
                          "sets": [{"indices": k, "signature": sigs[j, :96].tobytes().hex()} for j, k in enumerate(keys)]})
    finally:
        d.close()
    assert sorted(calls[1]["sets"][7]["indices"]) != sorted(calls[1]["sets"][8]["indices"])
    calls[1]["sets"][7]["signature"] = calls[1]["sets"][8]["signature"]  # another aggregate's signature
    calls[1]["expected"][7] = False
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "calls.json").write_text(json.dumps(calls))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "same_message_agg_test.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same message agg test OK" in r.stdout
