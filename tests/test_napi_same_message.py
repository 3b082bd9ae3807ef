"""verifySignatureSetsSameMessage through the N-API addon, driven from Node
(tests/js/same_message_test.js): three calls at once, two batchable and one
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


def test_same_message_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys = 64
    m1, m2 = hashlib.sha256(b"napi same message 1").digest(), hashlib.sha256(b"napi same message 2").digest()
    shape = [(list(range(0, 20)), m1, True), (list(range(20, 40)), m1, True), (list(range(40, 45)), m2, False)]
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E415049)
        table = d.pubkeys_get(0, n_keys)
        calls = []
        for idxs, m, batchable in shape:
            n = len(idxs)
            arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32),
                      "pk_offsets": np.arange(n + 1, dtype=np.uint32), "pk_indices": np.array(idxs, np.uint32),
                      "msgs": np.stack([np.frombuffer(m, np.uint8)] * n)}
            sigs = np.zeros((n, 192), np.uint8)
            d.gen_sign(arrays, sigs)
            calls.append({"message": m.hex(), "batchable": batchable, "expected": [True] * n,
                          "sets": [{"index": i, "signature": sigs[k, :96].tobytes().hex()} for k, i in enumerate(idxs)]})
    finally:
        d.close()
    calls[1]["sets"][7]["signature"] = calls[1]["sets"][8]["signature"]  # another validator's signature
    calls[1]["expected"][7] = False
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "calls.json").write_text(json.dumps(calls))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "same_message_test.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same message test OK" in r.stdout
