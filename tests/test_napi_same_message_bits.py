"""Committee sets in verifyAggregateSetsSameMessage through the N-API addon,
driven from Node (tests/js/same_message_bits_test.js): a mixed call of
committee and explicit sets through both classes with the key metric taken
from the device, and a call without committee sets on the old path."""
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


def test_committee_sets_same_message_through_node(tmp_path):
    from lodestar_amd import native
    from tools import build as B

    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    n_keys, list_id = 600, 3
    rng = np.random.default_rng(43)
    lst = rng.permutation(n_keys).astype(np.uint32)
    m1, m2 = hashlib.sha256(b"napi same message bits 1").digest(), hashlib.sha256(b"napi same message bits 2").digest()
    # two batchable calls on one root (20 + 14 > 32 signatures: one merged device call), one explicit call on another
    shape = [(20, m1, True, True), (14, m1, True, False), (5, m2, False, False)]
    calls, keys, msgs = [], [], []
    for n, m, batchable, committees in shape:
        sets = []
        for j in range(n):
            if committees and j % 4 != 3:
                length = int(rng.choice([9, 64, 128]))
                off = int(rng.integers(0, n_keys - length + 1))
                b = rng.random(length) < [1.0, 0.98, 0.5][j % 3]
                b[0] = True
                idx = [int(x) for x in lst[off:off + length][b]]
                sets.append({"committee": {"list": list_id, "offset": off, "length": length},
                             "bits": np.packbits(b, bitorder="little").tobytes().hex()})
            else:
                idx = [int(x) for x in rng.integers(0, n_keys, size=int(rng.choice([1, 2, 33])))]
                sets.append({"indices": idx})
            keys.append(idx)
            msgs.append(m)
        calls.append({"message": m.hex(), "batchable": batchable, "expected": [True] * n, "sets": sets,
                      "keys": sum(len(k) for k in keys[-n:])})
    n = len(keys)
    d = native.Device(0)
    try:
        d.gen_keys(0, n_keys, 0x4E534D42)
        table = d.pubkeys_get(0, n_keys)
        po = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32)
        arrays = {"n_sets": n, "n_jobs": n, "job_offsets": np.arange(n + 1, dtype=np.uint32), "pk_offsets": po,
                  "pk_indices": np.array([x for k in keys for x in k], np.uint32),
                  "msgs": np.stack([np.frombuffer(m, np.uint8) for m in msgs])}
        sigs = np.zeros((n, 192), np.uint8)
        d.gen_sign(arrays, sigs)
    finally:
        d.close()
    flat = [s for c in calls for s in c["sets"]]
    for i, s in enumerate(flat):
        s["signature"] = sigs[i, :96].tobytes().hex()
    assert sorted(keys[5]) != sorted(keys[6]) and "committee" in calls[0]["sets"][5]
    calls[0]["sets"][5]["signature"] = calls[0]["sets"][6]["signature"]  # another set's signature
    calls[0]["expected"][5] = False
    (tmp_path / "table96.bin").write_bytes(table)
    (tmp_path / "list.json").write_text(json.dumps(lst.tolist()))
    (tmp_path / "calls.json").write_text(json.dumps({"listId": list_id, "calls": calls}))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "same_message_bits_test.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same message bits test OK" in r.stdout
