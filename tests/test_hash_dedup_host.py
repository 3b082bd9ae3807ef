"""The two hash_to_G2 counters of both pools (lodestar_amd/verifier.py,
lodestar_amd/napi/index.js) with a stand-in device: fed from a device batch's
`hashes`, summed over the shards of a sharded batch, and absent until a batch
reports them, so no existing metric changes.  No GPU needed."""
import json
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from lodestar_amd import native
from lodestar_amd import verifier as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"hash_to_g2_sets", "hash_to_g2_evaluated"}


class FakeDevice:
    """every batch repeats each root once: half as many evaluations as sets"""

    def __init__(self):
        self.last_stats = native.BgvStats()
        self.last_n = 0

    def verify(self, arrays, **kw):
        self.last_n = arrays["n_sets"]
        return np.ones(arrays["n_jobs"], np.int32), None

    def partial(self, arrays, **kw):
        self.last_n = arrays["n_sets"]
        return bytes(576), np.zeros(arrays["n_sets"], np.int32), np.ones(arrays["n_jobs"], np.int32), True

    def combine_final(self, parts):
        return True

    def hash_stats(self):
        return {"sets": self.last_n, "hashes": self.last_n // 2, "dedup": 1}


def _pool(n_dev):
    pool = object.__new__(V.BlsGpuVerifier)
    pool.devices = [FakeDevice() for _ in range(n_dev)]
    pool._ctx_dev, pool.n_devices, pool.prio_reserved = list(range(n_dev)), n_dev, False
    pool._dev_locks = [threading.Lock() for _ in range(n_dev)]
    pool.metrics, pool._rng = V._new_metrics(), None
    return pool


def _jobs(sizes):
    one = V.create_single_signature_set_from_components(V.PublicKey(index=3), bytes(32), b"\xaa" * 96)
    return [[one] * n for n in sizes]


def test_python_pool_feeds_the_two_counters():
    pool = _pool(1)
    before = dict(pool.metrics)
    assert not NEW & set(before)  # absent until a batch reports them
    assert pool._run_device_batch(_jobs([4, 6]), [0]) == [True, True]
    assert pool.metrics["hash_to_g2_sets"] == 10 and pool.metrics["hash_to_g2_evaluated"] == 5
    assert pool._run_device_batch(_jobs([2]), [0]) == [True]
    assert pool.metrics["hash_to_g2_sets"] == 12 and pool.metrics["hash_to_g2_evaluated"] == 6
    # no existing key left or changed its type; the batch counters moved as before
    assert set(pool.metrics) == set(before) | NEW
    assert all(type(pool.metrics[k]) is type(v) for k, v in before.items())
    assert pool.metrics["sets_started"] == 12 and pool.metrics["jobs_started"] == 3


def test_python_pool_adds_up_the_shards():
    pool = _pool(2)
    assert pool._run_device_batch(_jobs([8, 8, 4, 4]), [0, 1]) == [True] * 4
    per_dev = [d.last_n for d in pool.devices]
    assert all(per_dev) and sum(per_dev) == 24
    assert pool.metrics["hash_to_g2_sets"] == 24
    assert pool.metrics["hash_to_g2_evaluated"] == sum(n // 2 for n in per_dev)


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_hash_stats_and_node_pool_feeds_the_counters():
    from tools import build as B
    addon = B.build_addon()
    if addon is None:
        pytest.skip("node_api.h not found")
    script = f"""
const a = require({addon!r});
if (typeof a.hashStats !== "function") throw Error("missing hashStats");
const v = require({os.path.join(ROOT, "lodestar_amd", "napi", "index.js")!r});
const pool = Object.create(v.BlsGpuVerifier.prototype);
const hist = () => ({{count: 0, sum: 0}});
pool.metrics = {{
  lodestar_bls_thread_pool_time_seconds_sum: 0, lodestar_bls_worker_thread_time_per_sigset_seconds: hist(),
  lodestar_bls_thread_pool_success_jobs_signature_sets_count: 0, lodestar_bls_thread_pool_error_jobs_signature_sets_count: 0,
  lodestar_bls_thread_pool_batch_retries_total: 0, lodestar_bls_thread_pool_batch_sigs_success_total: 0,
}};
const keys = Object.keys(pool.metrics);
const jobs = [{{sets: new Array(6)}}, {{sets: new Array(4)}}];
const res = {{results: Int32Array.from([1, -1]), workerStartMs: 1, workerEndMs: 3, batchRetries: 0, batchSigsSuccess: 6}};
pool.recordWork(jobs, res);  // a result without `hashes` (partialFinish) feeds nothing
const without = Object.keys(pool.metrics);
pool.recordWork(jobs, {{...res, hashes: 7}});
pool.recordWork(jobs, {{...res, hashes: 10}});
console.log(JSON.stringify({{keys, without, after: pool.metrics}}));
"""
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert out["without"] == out["keys"]
    assert set(out["after"]) == set(out["keys"]) | {"hashToG2Sets", "hashToG2Evaluated"}
    assert out["after"]["hashToG2Sets"] == 20 and out["after"]["hashToG2Evaluated"] == 17
    assert out["after"]["lodestar_bls_thread_pool_success_jobs_signature_sets_count"] == 18
    assert out["after"]["lodestar_bls_thread_pool_error_jobs_signature_sets_count"] == 12
