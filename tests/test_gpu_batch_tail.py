"""The batch-first tail of the steps path (bgv_batch_tail, DESIGN.md section 3j:
k_win_fold, k_msm_job over one virtual job, one k_miller_coop pair,
k_step_fold, k_batch_chain, and the guarded per-job kernels behind
k_batch_final) against the context set to batch_tail(0), which runs the per-job
tail, and against the verdicts the batches have by construction.

One context is open at a time: the module's context is switched between the
modes from call to call (the mode holds from the next call on), and the
default-layout case, which needs a context of its own, runs first and closes
it.  Every hardware queue of a process keeps scratch for its largest frame, and
the suite's CU-masked contexts (tests/test_gpu_shards.py) need eight queues of
their own later in the same process ("Queue resources").
Run on an MI355X (-m gpu)."""
import numpy as np
import pytest

from tests.test_gpu_miller_steps import N_KEYS, SEED, open_dev, slice_sets, wrong_point_sig

pytestmark = pytest.mark.gpu

# the forced layout of tests/test_gpu_miller_steps.py, every subgroup check deferred
LAYOUT = dict(split=0, miller=1, msm=2, lines=1, miller_steps=1, defer_pct=100)
BAD_ENCODING, NOT_IN_GROUP, INDEX_RANGE, EMPTY_JOB = 1, 3, 9, 10
FIRST = {"batch_first": 1, "retried": 0}
RETRIED = {"batch_first": 1, "retried": 1}


# first in the file: before the module's context exists
def test_default_context_auto_rule():
    """default cfg on 700 blocks of 98 sets of 2 keys (the auto-rule shape of the steps test): the steps path and
    the batch-first tail with it; nine faulted sets take the retry; 980 sets stay off both"""
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
    d = open_dev()
    try:
        sigs = np.zeros((n, 192), np.uint8)
        d.gen_sign(dict(a, msgs=sign_msgs), sigs)
        a.update(sigs=sigs, sig_len=np.full(n, 96, np.uint32), scalars=rng.integers(1, 2**63, size=n, dtype=np.uint64))
        jr, sc = d.verify(a)
        assert d.miller_path()["steps"] == 1 and d.tail_path() == RETRIED
        assert jr.tolist() == want and not sc.any() and d.last_stats.batch_retries == 1
        small = dict(a, n_sets=980, n_jobs=10, job_offsets=a["job_offsets"][:11].copy(), pk_offsets=a["pk_offsets"][:981].copy(),
                     pk_indices=a["pk_indices"][:980 * k].copy(), msgs=a["msgs"][:980].copy(), sigs=a["sigs"][:980].copy(),
                     sig_len=a["sig_len"][:980].copy(), scalars=a["scalars"][:980].copy())
        jr3, _ = d.verify(small)
        assert d.miller_path()["steps"] == 0 and d.tail_path()["batch_first"] == 0 and jr3.tolist() == want[:10]
    finally:
        d.close()


@pytest.fixture(scope="module")
def dev():
    d = open_dev(**LAYOUT)  # auto: on wherever the steps path is
    yield d
    d.close()


def job_sizes(n_jobs):
    """sizes from {1, 2, G-1, G, G+1, 98} in turn, the last but one job empty"""
    g = slice_sets()
    pool = [g + 1, 1, 98, 2, g, g - 1]
    sizes = [pool[j % len(pool)] for j in range(n_jobs)]
    if n_jobs > 1:
        sizes[n_jobs - 2] = 0
    return sizes


def build(dev, sizes, faults=(), seed=0):
    """a ragged batch of 1-2 table keys per set; faults: (job, kind) with kind "msg" (a signature over another
    message: the job is False), "enc" (cleared compression flag), "grp" (a point outside G2), "range" (a key index
    past the table), at the job's middle set.  Returns (arrays, verdicts by construction, set codes)."""
    n, J = sum(sizes), len(sizes)
    rng = np.random.default_rng(SEED + 77 + seed)
    counts = rng.integers(1, 3, size=n)
    jo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    po = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    a = {"n_sets": n, "n_jobs": J, "job_offsets": jo, "pk_offsets": po,
         "pk_indices": rng.integers(0, N_KEYS, size=max(int(counts.sum()), 1)).astype(np.uint32),
         "msgs": rng.integers(0, 256, size=(max(n, 1), 32), dtype=np.uint8),
         "scalars": rng.integers(1, 2**64 - 1, size=max(n, 1), dtype=np.uint64, endpoint=True)}
    sign_msgs = a["msgs"].copy()
    at = {j: int(jo[j]) + sizes[j] // 2 for j, _ in faults}
    for j, kind in faults:
        if kind == "msg":
            sign_msgs[at[j], 5] ^= 0x04
    sigs = np.zeros((max(n, 1), 192), np.uint8)
    if n:
        dev.gen_sign(dict({k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "pk_offsets", "pk_indices")}, msgs=sign_msgs), sigs)
    code = np.zeros(n, np.int32)
    want = [1 if s else -EMPTY_JOB for s in sizes]
    for j, kind in faults:
        i = at[j]
        if kind == "msg":
            want[j] = 0
        elif kind == "enc":
            sigs[i, 0] &= 0x7F
            code[i], want[j] = BAD_ENCODING, -BAD_ENCODING
        elif kind == "grp":
            sigs[i, :96] = wrong_point_sig()
            code[i], want[j] = NOT_IN_GROUP, -NOT_IN_GROUP
        elif kind == "range":
            a["pk_indices"][po[i]] = N_KEYS
            code[i], want[j] = INDEX_RANGE, -INDEX_RANGE
    a["sigs"], a["sig_len"] = sigs, np.full(max(n, 1), 96, np.uint32)
    return a, want, code.tolist()


def stats_of(dev):
    s = dev.last_stats
    return (s.n_sets, s.n_jobs, s.pubkeys_aggregated, s.batch_retries, s.batch_sigs_success, dev.last_stats.layout())


def both(dev, a, want, code, path, verify="verify"):
    """the batch through the batch-first tail (auto), then through the per-job tail (the context set to mode 0)"""
    try:
        jr, sc = getattr(dev, verify)(a)
        assert dev.miller_path()["steps"] == 1
        assert dev.tail_path() == path
        s_on = stats_of(dev)
        assert dev.last_stats.batch_retries == path["retried"]
        dev.batch_tail(0)
        jr0, sc0 = getattr(dev, verify)(a)
        assert dev.tail_path() == {"batch_first": 0, "retried": 0}
        assert jr.tolist() == jr0.tolist() == want
        assert sc.tolist() == sc0.tolist() == code
        assert s_on == stats_of(dev)
    finally:
        dev.batch_tail(-1)


@pytest.mark.parametrize("n_jobs", [1, 8, 9, 64, 65])
def test_clean_ragged_batches(dev, n_jobs):
    a, want, code = build(dev, job_sizes(n_jobs), seed=n_jobs)
    both(dev, a, want, code, FIRST)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_wrong_message_signature(dev, where):
    sizes = job_sizes(65)
    j = {"first": 0, "middle": 32, "last": 64}[where]
    a, want, code = build(dev, sizes, [(j, "msg")], seed=100 + j)
    assert want.count(0) == 1
    both(dev, a, want, code, RETRIED)


@pytest.mark.parametrize("kind", ["enc", "grp", "range"])
def test_rejected_job_is_left_out(dev, kind):
    """the rejected job is out of S_batch and out of the fold: the others verify at the batch check"""
    a, want, code = build(dev, job_sizes(9), [(4, kind)], seed=200)
    assert want[4] < 0 and all(w == 1 for k, w in enumerate(want) if k not in (4, 7))
    both(dev, a, want, code, FIRST)
    # ... and beside a False job the retry reports all three kinds of verdict
    a, want, code = build(dev, job_sizes(9), [(4, kind), (2, "msg")], seed=201)
    both(dev, a, want, code, RETRIED)


def test_all_jobs_rejected_and_no_jobs(dev):
    sizes = [3, 0, slice_sets() + 1]
    a, want, code = build(dev, sizes, [(0, "enc"), (2, "grp")], seed=300)
    assert all(w < 0 for w in want)
    both(dev, a, want, code, FIRST)
    a, want, code = build(dev, [], seed=301)
    jr, sc = dev.verify(a)
    assert len(jr) == 0 and dev.tail_path()["retried"] == 0
    retries = dev.last_stats.batch_retries
    dev.batch_tail(0)
    try:
        jr0, _ = dev.verify(a)
        assert len(jr0) == 0 and dev.last_stats.batch_retries == retries
    finally:
        dev.batch_tail(-1)


@pytest.mark.parametrize("fault", [None, "msg"])
def test_partial_combine_finish_on_two_shards(dev, fault):
    sizes = job_sizes(18)
    a, want, code = build(dev, sizes, [(12, fault), (3, "enc")] if fault else [], seed=400)
    jo, po = a["job_offsets"], a["pk_offsets"]

    def shard(j0, j1):
        s0, s1 = int(jo[j0]), int(jo[j1])
        return {"n_sets": s1 - s0, "n_jobs": j1 - j0, "job_offsets": (jo[j0:j1 + 1] - jo[j0]).astype(np.uint32),
                "pk_offsets": (po[s0:s1 + 1] - po[s0]).astype(np.uint32), "pk_indices": a["pk_indices"][po[s0]:po[s1]].copy(),
                "msgs": a["msgs"][s0:s1].copy(), "sigs": a["sigs"][s0:s1].copy(), "sig_len": a["sig_len"][s0:s1].copy(),
                "scalars": a["scalars"][s0:s1].copy()}

    shards = [shard(0, 9), shard(9, 18)]
    try:
        dev.batch_tail(0)
        jr, sc = dev.verify(a)  # the per-job tail's verdicts of the whole batch
        assert jr.tolist() == want and sc.tolist() == code
        dev.batch_tail(1)
        parts = [dev.partial(s) for s in shards]
        assert dev.tail_path() == FIRST
        assert parts[0][1].tolist() + parts[1][1].tolist() == code
        assert (parts[0][3] and parts[1][3]) == all(w >= 0 for w in want)
        m0, m1 = parts[0][0], parts[1][0]
        assert dev.combine_final([m0, m1]) == (fault is None)
        assert dev.combine_final([m0]) and dev.combine_final([m1]) == (fault is None)
        got = []
        for k, s in enumerate(shards):  # the pending partial is per context: this shard's once more, then its verdicts
            dev.partial(s)
            got += dev.partial_finish().tolist()
            assert dev.tail_path() == (RETRIED if fault and k == 1 else FIRST)
        assert got == want
    finally:
        dev.batch_tail(-1)


@pytest.mark.parametrize("fault", [None, "msg"])
def test_verify_bits(dev, fault):
    from lodestar_amd import native
    a, want, code = build(dev, job_sizes(9), [(5, fault)] if fault else [], seed=500)
    po = a["pk_offsets"]
    n = a["n_sets"]
    src = np.zeros(n, native.SET_SRC_DTYPE)
    src["list"], src["off"], src["len"], src["bits_off"] = native.SRC_EXPLICIT, po[:-1], np.diff(po), 0xFFFFFFF0
    b = {k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "pk_indices", "msgs", "sigs", "sig_len", "scalars")}
    b.update(src=src, bits=np.zeros(4, np.uint8), bits_len=4, n_indices=int(po[-1]))
    both(dev, b, want, code, RETRIED if fault else FIRST, verify="verify_bits")
