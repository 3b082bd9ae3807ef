"""The Miller stage as per-step line products (bgv_cfg.miller_steps: kernels
k_miller_steps and k_job_chain) against the item loop
it stands in for and against the golden vectors.  Values are exact field
elements: every comparison is byte equality, after the final exponentiation
where the Miller value itself is not canonical.  Run on an MI355X (-m gpu)."""
import os
import re

import numpy as np
import pytest

from oracle import bls12_381 as B
from tests import gpu_util as G
from tests.hostcheck import b_tower

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_KEYS = 4400
SEED = 0x53544550
LAYOUT = dict(split=0, miller=1, msm=2, lines=1)  # the bulk one-lane layout over lines, forced at any size
BAD_ENCODING, NOT_IN_GROUP, INDEX_RANGE = 1, 3, 9


def slice_sets():
    api = open(os.path.join(ROOT, "lodestar_amd", "csrc", "bgv_api.hip")).read()
    return int(re.search(r"#define BGV_STEPS_SLICE (\d+)", api).group(1))


def _flat(gt_bytes: bytes):
    return B.tower_to_f12(b_tower(gt_bytes))


def _golden_gt(hexstr: str):
    return tuple(int(hexstr[96 * k: 96 * k + 96], 16) for k in range(12))


def open_dev(**cfg):
    from lodestar_amd import native
    d = native.Device(0, **cfg)
    d.gen_keys(0, N_KEYS, SEED)
    return d


@pytest.fixture(scope="module")
def steps():
    d = open_dev(miller_steps=1, **LAYOUT)
    yield d
    d.close()


@pytest.fixture(scope="module")
def items():
    d = open_dev(miller_steps=0, **LAYOUT)
    yield d
    d.close()


# ------------------------------------------------------------ (a) golden batch
def test_golden_batch_stage_values():
    from lodestar_amd import native
    v = G.batch_vectors()
    sets = [s for j in v["jobs"] for s in j["sets"]]
    d = native.Device(0, miller_steps=1, **LAYOUT)
    try:
        G.load_golden_table(d)
        arrays, expected, codes = G.golden_arrays()
        out = d.debug_stages(arrays)
        path = d.miller_path()
    finally:
        d.close()
    n, J = arrays["n_sets"], arrays["n_jobs"]
    jo = arrays["job_offsets"]
    assert path["steps"] == 1 and path["slice_sets"] == slice_sets()
    assert path["items"] == sum(-(-int(jo[j + 1] - jo[j]) // slice_sets()) for j in range(J))
    assert out["job_result"].tolist() == expected
    assert out["set_code"].tolist() == codes
    for i, s in enumerate(sets):
        for key in ("sig_aff", "h_aff", "pk_agg", "rpk_aff"):
            assert out[key][i].tobytes().hex() == s[key], (key, i)
    for j, job in enumerate(v["jobs"]):
        assert out["s_aff"][j].tobytes().hex() == job["s_aff"], ("s_aff", j)
        assert B.f12_eq(_flat(out["job_fe"][j].tobytes()), _golden_gt(job["job_gt"])), ("job_gt", j)
        assert B.f12_eq(_flat(out["pair_fe"][n + j].tobytes()), _golden_gt(job["job_pair_gt"])), ("job_pair", j)
    assert B.f12_eq(_flat(out["batch_fe"].tobytes()), _golden_gt(v["batch_gt"]))
    # the job is the item: its set product at its first set (1 when a pubkey of
    # the job was rejected), 1 at its other sets
    for j in range(J):
        beg, end = int(jo[j]), int(jo[j + 1])
        if beg == end:
            continue
        want = B.F12_ONE
        if all(sets[k]["pk_agg"] != "00" * 96 for k in range(beg, end)):
            for k in range(beg, end):
                want = B.f12_mul(want, _golden_gt(sets[k]["pair_gt"]))
        assert B.f12_eq(_flat(out["pair_fe"][beg].tobytes()), want), ("job set product", j)
        for k in range(beg + 1, end):
            assert B.f12_eq(_flat(out["pair_fe"][k].tobytes()), B.F12_ONE), ("other set", k)


# ------------------------------------------------- (b), (c) ragged synthetic batch
def ragged_sizes():
    g = slice_sets()
    rng = np.random.default_rng(SEED)
    edge = sorted({1, 2, max(g - 1, 1), g, g + 1, 2 * g + 1, 98})
    sizes = edge + [int(x) for x in rng.integers(20, 99, size=40 - len(edge))]
    rng.shuffle(sizes)
    return sizes


def wrong_point_sig():
    """an on-curve point outside G2 from the golden vectors (BLST_POINT_NOT_IN_GROUP)"""
    for j in G.batch_vectors()["jobs"]:
        for s in j["sets"]:
            if s.get("code") == NOT_IN_GROUP and len(s["sig"]) == 192:
                return np.frombuffer(bytes.fromhex(s["sig"]), np.uint8)
    raise AssertionError("no not-in-G2 vector in the golden file")


def ragged_batch(dev, faults: bool):
    """~40 jobs of 1 .. 2G+1 sets, ~2,500 sets of 1-4 table keys; with faults: 2% of the sets, a quarter each of
    wrong-message signature (False), swapped key (False), cleared compression flag (rejected) and a signature
    outside G2 (rejected), plus one key index past the table (a rejected pubkey) in a job of several slices"""
    sizes = ragged_sizes()
    n = sum(sizes)
    rng = np.random.default_rng(SEED + 1)
    counts = rng.integers(1, 5, size=n)
    jo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    po = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    a = {"n_sets": n, "n_jobs": len(sizes), "job_offsets": jo, "pk_offsets": po,
         "pk_indices": rng.integers(0, N_KEYS - 1, size=int(counts.sum())).astype(np.uint32),
         "msgs": rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
         "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)}
    sign_msgs = a["msgs"].copy()
    code = np.zeros(n, np.int32)
    false_set = np.zeros(n, bool)
    pick = np.sort(rng.choice(n, size=int(n * 0.02), replace=False)) if faults else np.zeros(0, np.int64)
    kind = rng.permutation(np.arange(len(pick)) % 4)
    sign_msgs[pick[kind == 0], 0] ^= 1
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign(dict({k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "pk_offsets", "pk_indices")}, msgs=sign_msgs), sigs)
    for i in pick[kind == 1]:
        a["pk_indices"][po[i]] += 1  # another key of the table
    sigs[pick[kind == 2], 0] &= 0x7F
    sigs[pick[kind == 3], :96] = wrong_point_sig()
    code[pick[kind == 2]] = BAD_ENCODING
    code[pick[kind == 3]] = NOT_IN_GROUP
    false_set[pick[(kind == 0) | (kind == 1)]] = True
    pk_code = np.zeros(n, np.int32)
    a["range_job"] = -1
    if faults:
        j = sizes.index(2 * slice_sets() + 1)
        i = int(jo[j]) + sizes[j] // 2  # the middle set of the three-slice job (the next one not faulted already)
        while i in pick:
            i += 1
        assert i < jo[j + 1]
        a["pk_indices"][po[i]] = N_KEYS
        pk_code[i] = INDEX_RANGE
        a["range_job"] = j
    a["sigs"], a["sig_len"] = sigs, np.full(n, 96, np.uint32)
    want = []
    for j in range(len(sizes)):  # a job reports its first signature code, else its first key code
        verdict = 0 if false_set[jo[j]:jo[j + 1]].any() else 1
        for c in (pk_code[jo[j]:jo[j + 1]], code[jo[j]:jo[j + 1]]):
            nz = np.nonzero(c)[0]
            if len(nz):
                verdict = -int(c[nz[0]])
        want.append(verdict)
    return a, want, (code + pk_code).tolist()


@pytest.fixture(scope="module")
def faulted(steps):
    return ragged_batch(steps, True)


@pytest.fixture(scope="module")
def clean(steps):
    return ragged_batch(steps, False)


def test_ragged_batch_against_the_item_loop(steps, items, faulted, clean):
    for a, want, code in (faulted, clean):
        s = steps.debug_stages(a)
        assert steps.miller_path()["steps"] == 1
        t = items.debug_stages(a)
        assert items.miller_path() == {"steps": 0, "slice_sets": 1, "items": a["n_sets"]}
        assert s["job_result"].tolist() == t["job_result"].tolist() == want
        assert s["set_code"].tolist() == t["set_code"].tolist() == code
        assert s["job_fe"].tobytes() == t["job_fe"].tobytes()
        assert s["batch_fe"].tobytes() == t["batch_fe"].tobytes()
        for key in ("h_aff", "rpk_aff", "s_aff"):
            assert s[key].tobytes() == t[key].tobytes(), key
        n = a["n_sets"]
        assert s["pair_fe"][n:].tobytes() == t["pair_fe"][n:].tobytes()  # the (-G1, S_job) pairs
        for j, w in enumerate(want):  # by construction: a valid job's product is 1, a false one's is not
            one = B.f12_eq(_flat(s["job_fe"][j].tobytes()), B.F12_ONE)
            assert one == (w != 0), j
        # the job's set product at its first set is the product of the item loop's per-set values
        jo = a["job_offsets"]
        for j in sorted({0, len(want) // 2, len(want) - 1, max(a["range_job"], 0)}):
            beg, end = int(jo[j]), int(jo[j + 1])
            prod = B.F12_ONE
            for k in range(beg, end):
                prod = B.f12_mul(prod, _flat(t["pair_fe"][k].tobytes()))
            if any(c == INDEX_RANGE for c in code[beg:end]):
                prod = B.F12_ONE
            assert B.f12_eq(_flat(s["pair_fe"][beg].tobytes()), prod), j


def test_verify_and_partial(steps, faulted, clean):
    for (a, want, code), retries in ((faulted, 1), (clean, 0)):
        jr, sc = steps.verify(a)
        assert steps.miller_path()["steps"] == 1
        assert jr.tolist() == want
        assert sc.tolist() == code
        assert steps.last_stats.batch_retries == retries
        layout = steps.last_stats.layout()  # the configured pairs keep being reported
        assert layout["pairs_per_item"] == 1 and layout["lines"] == 1 and layout["split"] == 0
        m, sc2, jr2, ok = steps.partial(a)
        assert steps.miller_path()["steps"] == 1
        assert sc2.tolist() == sc.tolist()
        assert ok == all(w >= 0 for w in want)
        assert steps.combine_final([m]) == (retries == 0)
        assert steps.partial_finish().tolist() == want


# ------------------------------------------------------------------ (d) auto rule
def test_auto_rule_on_a_700_block_batch():
    """default cfg on 700 blocks of 98 sets: the layout chooses two pairs per item over lines by itself, and the
    steps path with it; an explicit pairs keeps the item loop"""
    from lodestar_amd import native
    n, k, per_job = 700 * 98, 2, 98
    rng = np.random.default_rng(SEED + 2)
    a = {"n_sets": n, "n_jobs": 700, "job_offsets": (np.arange(701) * per_job).astype(np.uint32),
         "pk_offsets": (np.arange(n + 1) * k).astype(np.uint32),
         "pk_indices": rng.integers(0, N_KEYS, size=n * k).astype(np.uint32),
         "msgs": rng.integers(0, 256, size=(n, 32), dtype=np.uint8)}
    bad = np.zeros(n, bool)
    bad[rng.choice(n, size=9, replace=False)] = True
    sign_msgs = a["msgs"].copy()
    sign_msgs[bad, 3] ^= 0x10
    want = [0 if bad[j * per_job:(j + 1) * per_job].any() else 1 for j in range(700)]
    da, dp = open_dev(), open_dev(pairs=2)
    try:
        sigs = np.zeros((n, 192), np.uint8)
        da.gen_sign(dict(a, msgs=sign_msgs), sigs)
        a.update(sigs=sigs, sig_len=np.full(n, 96, np.uint32), scalars=rng.integers(1, 2**63, size=n, dtype=np.uint64))
        jr, sc = da.verify(a)
        g = slice_sets()
        assert da.miller_path() == {"steps": 1, "slice_sets": g, "items": 700 * -(-98 // g)}
        assert da.last_stats.layout()["pairs_per_item"] == 2 and da.last_stats.layout()["lines"] == 1
        assert jr.tolist() == want and not sc.any() and da.last_stats.batch_retries == 1
        jr2, sc2 = dp.verify(a)
        assert dp.miller_path() == {"steps": 0, "slice_sets": 2, "items": 700 * 49}
        assert dp.last_stats.layout()["pairs_per_item"] == 2
        assert dp.last_stats.layout() == da.last_stats.layout()
        assert jr2.tolist() == want and not sc2.any()
        # below the size where the layout takes two pairs per item, auto stays off
        small = dict(a, n_sets=980, n_jobs=10, job_offsets=a["job_offsets"][:11].copy(), pk_offsets=a["pk_offsets"][:981].copy(),
                     pk_indices=a["pk_indices"][:980 * k].copy(), msgs=a["msgs"][:980].copy(), sigs=a["sigs"][:980].copy(),
                     sig_len=a["sig_len"][:980].copy(), scalars=a["scalars"][:980].copy())
        jr3, _ = da.verify(small)
        assert da.miller_path()["steps"] == 0 and jr3.tolist() == want[:10]
    finally:
        da.close()
        dp.close()
