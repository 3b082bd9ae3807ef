"""The split retry of the same-message entries through the N-API addon, driven
from Node (tests/js/sm_retry_test.js): one call of 64 sets with one bad
signature on a pool with and without the smRetry option, the context calls
smRetry / smRetryStats, and the single-thread verifier."""
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


def test_sm_retry_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n = 64
    m = hashlib.sha256(b"napi sm retry").digest()
    d = native.Device(0)
    try:
        d.gen_keys(0, n, 0x4E525452)
        table = d.pubkeys_get(0, n)
        arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32),
                  "pk_offsets": np.arange(n + 1, dtype=np.uint32), "pk_indices": np.arange(n, dtype=np.uint32),
                  "msgs": np.stack([np.frombuffer(m, np.uint8)] * n)}
        sigs = np.zeros((n, 192), np.uint8)
        d.gen_sign(arrays, sigs)
    finally:
        d.close()
    call = {"message": m.hex(), "expected": [True] * n,
            "sets": [{"index": i, "signature": sigs[i, :96].tobytes().hex()} for i in range(n)]}
    call["sets"][29]["signature"] = call["sets"][30]["signature"]  # another validator's signature
    call["expected"][29] = False
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "call.json").write_text(json.dumps(call))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "sm_retry_test.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sm retry test OK" in r.stdout
