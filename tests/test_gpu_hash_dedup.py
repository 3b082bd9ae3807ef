"""hash_to_G2 once per distinct signing root in the bulk layout (bgv_cfg.hash_dedup,
bgv_hash_stats): a context that groups its sets by root (hash_dedup = 1) against
one that hashes every set (hash_dedup = 0), on the same batches with injected
scalars.  Auto means off (measured), so the grouping
contexts opt in.
Everything observable must be equal: job results, set codes, counters and the
bytes of every set's H(m); only the number of evaluations differs.  Run on an
MI355X (-m gpu)."""
import hashlib
import threading

import numpy as np
import pytest

from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu

SEED = 0x48444450
N_KEYS = 4400
INDEX_RANGE = 9   # BGV_SET_INDEX_RANGE
BAD_ENCODING = 1  # BLST_BAD_ENCODING
CLASS_CYCLE = [1, 2, 3, 64, 65, 128]
N4 = 4229  # 66 waves + 5 lanes


def open_dev(**cfg):
    from lodestar_amd import native
    d = native.Device(0, **cfg)
    d.gen_keys(0, N_KEYS, SEED)
    return d


@pytest.fixture(scope="module")
def autos():
    """three contexts in the bulk layout that group their sets by root"""
    ds = [open_dev(split=0, hash_dedup=1) for _ in range(3)]
    yield ds
    for d in ds:
        d.close()


@pytest.fixture(scope="module")
def A(autos):
    return autos[0]


@pytest.fixture(scope="module")
def B():
    d = open_dev(split=0, hash_dedup=0)
    yield d
    d.close()


def root(tag, k):
    return np.frombuffer(hashlib.sha256(b"hash dedup %s %d" % (tag, k)).digest(), np.uint8).copy()


def make_batch(dev, rng, set_root, job_sizes):
    """a signed batch: set i carries roots[set_root[i]] (see callers) and 1-4 table keys"""
    n = len(set_root)
    assert sum(job_sizes) == n
    counts = rng.integers(1, 5, size=n)
    a = {"n_sets": n, "n_jobs": len(job_sizes),
         "job_offsets": np.concatenate([[0], np.cumsum(job_sizes)]).astype(np.uint32),
         "pk_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32),
         "pk_indices": rng.integers(0, N_KEYS, size=int(counts.sum())).astype(np.uint32),
         "msgs": np.ascontiguousarray(set_root, np.uint8),
         "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)}
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "pk_offsets", "pk_indices", "msgs")}, sigs)
    a["sigs"] = sigs
    a["sig_len"] = np.full(n, 96, np.uint32)
    return a


def distinct(a):
    return len({m.tobytes() for m in a["msgs"]})


def shape4(dev, seed):
    """4,229 sets; classes of 1, 2, 3, 64, 65 and 128 sets shuffled over the whole batch, so they cross waves and
    jobs; jobs of 1 to 128 sets; four roots that differ in byte 0 only, byte 31 only, bytes 12-19 only"""
    rng = np.random.default_rng(seed)
    sizes = CLASS_CYCLE * 16 + [3, 3, 3, 3, 3, 3, 2, 1]
    assert sum(sizes) == N4
    roots = [root(b"class %d" % seed, k) for k in range(len(sizes))]
    base = roots[-8]
    for k, (lo, hi) in zip((-7, -6, -5), ((0, 1), (31, 32), (12, 20))):
        roots[k] = base.copy()
        roots[k][lo:hi] ^= 0x5A
    assert roots[-5][:8].tobytes() == base[:8].tobytes() and roots[-5][24:].tobytes() == base[24:].tobytes()
    cls = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    jobs = [1, 128]
    while sum(jobs) < N4:
        jobs.append(min(int(rng.integers(1, 129)), N4 - sum(jobs)))
    rng.shuffle(jobs)
    a = make_batch(dev, rng, np.stack(roots)[cls], jobs)
    assert distinct(a) == len(sizes) == 104
    a["cls"], a["class_sizes"] = cls, sizes
    return a


@pytest.fixture(scope="module")
def s4(A):
    return shape4(A, 4)


@pytest.fixture(scope="module")
def s3(A):
    """197 sets (3 waves + 5 lanes) of one root in 5 jobs: every lane of every wave races for one slot"""
    return make_batch(A, np.random.default_rng(3), np.stack([root(b"one", 0)] * 197), [40, 40, 40, 40, 37])


@pytest.fixture(scope="module")
def s2(A):
    return make_batch(A, np.random.default_rng(2), np.stack([root(b"all", k) for k in range(197)]), [50, 50, 50, 47])


COUNTERS = ("batch_retries", "batch_sigs_success", "pubkeys_aggregated", "n_sets", "n_jobs")


def run(dev, a, **kw):
    jr, sc = dev.verify(a, **kw)
    st = {k: int(getattr(dev.last_stats, k)) for k in COUNTERS}
    hs = dev.hash_stats()
    dbg = dev.debug_stages(a, **kw)
    assert dev.hash_stats() == hs  # bgv_debug_stages reports the same path
    assert dbg["job_result"].tolist() == jr.tolist() and dbg["set_code"].tolist() == sc.tolist()
    return {"jr": jr.tolist(), "sc": sc.tolist(), "stats": st, "hash_stats": hs, "h_aff": dbg["h_aff"].copy()}


_REF = {}


def reference(B, name, a):
    """the hash_dedup = 0 context's outputs, computed once per batch"""
    if name not in _REF:
        r = run(B, a)
        n = a["n_sets"]
        assert r["hash_stats"] == {"sets": n, "hashes": n, "dedup": 0}
        _REF[name] = r
    return _REF[name]


def parity(dev, B, name, a, want_jr, **kw):
    ref = reference(B, name, a)
    got = run(dev, a, **kw)
    n = a["n_sets"]
    assert got["hash_stats"] == {"sets": n, "hashes": distinct(a), "dedup": 1}
    assert got["jr"] == ref["jr"] == want_jr
    assert got["sc"] == ref["sc"]
    assert got["stats"] == ref["stats"]
    assert got["h_aff"].tobytes() == ref["h_aff"].tobytes()
    return got


def g2_bytes(pt):
    return b"".join((v % O.P).to_bytes(48, "big") for v in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]))


def test_one_set(A, B):
    a = make_batch(A, np.random.default_rng(1), np.stack([root(b"single", 0)]), [1])
    got = parity(A, B, "one", a, [1])
    assert got["hash_stats"]["hashes"] == 1


def test_all_roots_distinct(A, B, s2):
    got = parity(A, B, "s2", s2, [1] * 4)
    assert got["hash_stats"]["hashes"] == 197


def test_one_root_for_every_set(A, B, s3):
    got = parity(A, B, "s3", s3, [1] * 5)
    assert got["hash_stats"]["hashes"] == 1 and not any(got["sc"])


def test_classes_across_waves_and_jobs(A, B, s4):
    got = parity(A, B, "s4", s4, [1] * s4["n_jobs"])
    assert got["stats"]["batch_retries"] == 0 and got["stats"]["batch_sigs_success"] == N4
    # H(m) of 8 sets against the from-spec oracle: the near-equal roots, a single, members of large classes
    cls, sizes = s4["cls"], s4["class_sizes"]
    picks = [int(np.flatnonzero(cls == len(sizes) + k)[-1]) for k in (-8, -7, -6, -5)]
    picks += [int(np.flatnonzero(cls == k)[-1]) for k in (0, 3, 4, 5)]  # sizes 1, 64, 65, 128: their last members
    for i in picks:
        assert got["h_aff"][i].tobytes() == g2_bytes(O.hash_to_g2(s4["msgs"][i].tobytes())), i


def faulty(dev, s4):
    """shape 4 with three faults, each inside a class of several sets and each in a job of its own"""
    a = dict(s4)
    cls = s4["cls"]
    jo, po = s4["job_offsets"], s4["pk_offsets"]
    job_of = lambda i: int(np.searchsorted(jo, i, side="right")) - 1
    wrong = int(np.flatnonzero(cls == 3)[5])    # class of 64
    undec = next(int(m) for m in np.flatnonzero(cls == 4) if job_of(m) != job_of(wrong))   # class of 65
    ranged = next(int(m) for m in np.flatnonzero(cls == 5) if job_of(m) not in (job_of(wrong), job_of(undec)))  # of 128
    a["sigs"] = s4["sigs"].copy()
    a["sigs"][wrong] = wrong_root_signature(dev, s4, wrong, undec)
    a["sigs"][undec, 0] &= 0x7F  # compression flag cleared
    a["pk_indices"] = s4["pk_indices"].copy()
    a["pk_indices"][po[ranged]] = N_KEYS  # one past the table
    want = [1] * a["n_jobs"]
    want[job_of(wrong)], want[job_of(undec)], want[job_of(ranged)] = 0, -BAD_ENCODING, -INDEX_RANGE
    return a, want, (wrong, undec, ranged)


def test_faults_inside_classes(A, B, s4):
    a, want, (wrong, undec, ranged) = faulty(A, s4)
    got = parity(A, B, "s5", a, want)
    assert got["stats"]["batch_retries"] == 1
    assert got["sc"][undec] == BAD_ENCODING and got["sc"][ranged] == INDEX_RANGE


def test_state_between_calls(A, B, s2, s3, s4):
    """one root -> all distinct -> shape 4 -> one root again: a table or a counter left from the call before shows"""
    for name, a in (("s3", s3), ("s2", s2), ("s4", s4), ("s3", s3)):
        parity(A, B, name, a, [1] * a["n_jobs"])


def to_device(a):
    import torch
    out = dict(a)
    for k, v in a.items():
        if isinstance(v, np.ndarray) and k not in ("cls",):
            flat = np.ascontiguousarray(v)
            view = flat.view(np.uint8) if flat.dtype.itemsize == 1 else flat.view(np.int64) if k == "scalars" else flat.view(np.int32)
            out[k] = torch.from_numpy(view.copy()).to("cuda:0")
    return out


def test_on_device_inputs(A, B, s4):
    ref = reference(B, "s4", s4)
    got = run(A, to_device(s4), on_device=True)
    assert got["hash_stats"] == {"sets": N4, "hashes": 104, "dedup": 1}
    assert got["jr"] == ref["jr"] and got["sc"] == ref["sc"] and got["stats"] == ref["stats"]
    assert got["h_aff"].tobytes() == ref["h_aff"].tobytes()


# ---------------------------------------------------------------- other entries
def bits_batch(dev, lst):
    """48 committee sets over windows of one resident list, roots shared in runs of 4, in 6 jobs; participation
    near 99% (the complement path of a context with sums) and near 50%"""
    from lodestar_amd import native
    rng = np.random.default_rng(8)
    n = 48
    src, bits, idx, po = [], bytearray(), [], [0]
    for i in range(n):
        length = int(rng.choice([64, 128, 128, 200]))
        off = int(rng.integers(0, N_KEYS - length + 1))
        b = rng.random(length) < (0.99 if i % 3 else 0.5)
        b[0] = True
        src.append((0, off, length, len(bits)))
        bits += np.packbits(b, bitorder="little").tobytes()
        idx.append(lst[off:off + length][b])
        po.append(po[-1] + int(b.sum()))
    msgs = np.stack([root(b"bits", i // 4) for i in range(n)])
    jobs = np.arange(0, n + 1, 8, dtype=np.uint32)
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({"n_sets": n, "n_jobs": 6, "job_offsets": jobs, "pk_offsets": np.array(po, np.uint32),
                  "pk_indices": np.concatenate(idx).astype(np.uint32), "msgs": msgs}, sigs)
    return {"n_sets": n, "n_jobs": 6, "job_offsets": jobs, "src": np.array(src, native.SET_SRC_DTYPE),
            "bits": np.frombuffer(bytes(bits), np.uint8).copy(), "bits_len": len(bits),
            "pk_indices": np.zeros(1, np.uint32), "n_indices": 0, "msgs": msgs, "sigs": sigs,
            "sig_len": np.full(n, 96, np.uint32),
            "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)}, po[-1]


def test_verify_bits_with_and_without_sums(A, B):
    lst = np.random.default_rng(9).permutation(N_KEYS).astype(np.uint32)
    for d in (A, B):
        d.index_list_set(0, lst)
    try:
        a, keys = bits_batch(A, lst)
        for sums in (False, True):
            out = []
            for d in (A, B):
                d.index_list_sums(0, sums)
                jr, sc = d.verify_bits(a)
                out.append((jr.tolist(), sc.tolist(), {k: int(getattr(d.last_stats, k)) for k in COUNTERS}, d.bits_path_stats()))
                assert d.hash_stats() == ({"sets": 48, "hashes": 12, "dedup": 1} if d is A else {"sets": 48, "hashes": 48, "dedup": 0})
            assert out[0] == out[1]
            assert out[0][0] == [1] * 6 and not any(out[0][1]) and out[0][2]["pubkeys_aggregated"] == keys
            assert (out[0][3]["sets_complement"] > 0) == sums
    finally:
        for d in (A, B):
            d.index_list_set(0, np.zeros(0, np.uint32))


def job_slice(a, j0, j1):
    jo, po = a["job_offsets"], a["pk_offsets"]
    s0, s1 = int(jo[j0]), int(jo[j1])
    out = {"n_sets": s1 - s0, "n_jobs": j1 - j0, "job_offsets": (jo[j0:j1 + 1] - jo[j0]).astype(np.uint32),
           "pk_offsets": (po[s0:s1 + 1] - po[s0]).astype(np.uint32), "pk_indices": a["pk_indices"][po[s0]:po[s1]].copy()}
    for k in ("msgs", "sigs", "sig_len", "scalars"):
        out[k] = a[k][s0:s1].copy()
    return out


def wrong_root_signature(dev, s4, i, other):
    """set i's own keys over the root of set `other`: decodes, lies in the group, verifies nothing here"""
    po = s4["pk_offsets"]
    one = {"n_sets": 1, "n_jobs": 1, "job_offsets": np.array([0, 1], np.uint32),
           "pk_offsets": np.array([0, po[i + 1] - po[i]], np.uint32),
           "pk_indices": s4["pk_indices"][po[i]:po[i + 1]].copy(), "msgs": s4["msgs"][other:other + 1].copy()}
    sig = np.zeros((1, 192), np.uint8)
    dev.gen_sign(one, sig)
    return sig[0]


@pytest.mark.parametrize("fault", [False, True], ids=["clean", "fault_in_second_half"])
def test_partial_on_two_contexts(autos, B, s4, fault):
    a = s4
    want = [1] * s4["n_jobs"]
    mid = s4["n_jobs"] // 2
    if fault:  # every job decodes, the combined check fails, partial_finish finds the job
        jo = s4["job_offsets"]
        i = int([m for m in np.flatnonzero(s4["cls"] == 3) if m >= jo[mid]][0])  # a member of a class of 64
        other = int(np.flatnonzero(s4["cls"] == 4)[0])
        a = dict(s4)
        a["sigs"] = s4["sigs"].copy()
        a["sigs"][i] = wrong_root_signature(autos[0], s4, i, other)
        want[int(np.searchsorted(jo, i, side="right")) - 1] = 0
    halves = [job_slice(a, 0, mid), job_slice(a, mid, s4["n_jobs"])]
    parts, ref_parts = [], []
    for d, h in zip(autos[:2], halves):
        m, sc, jr, ok = d.partial(h)
        assert d.hash_stats() == {"sets": h["n_sets"], "hashes": distinct(h), "dedup": 1}
        parts.append((m, sc.tolist(), jr.tolist(), ok))
    for h in halves:
        m, sc, jr, ok = B.partial(h)
        assert B.hash_stats() == {"sets": h["n_sets"], "hashes": h["n_sets"], "dedup": 0}
        ref_parts.append((m, sc.tolist(), jr.tolist(), ok))
    assert parts == ref_parts  # the Miller products byte for byte
    ok = autos[2].combine_final([p[0] for p in parts])
    assert ok == B.combine_final([p[0] for p in ref_parts]) == (not fault)
    if fault:
        jr = autos[1].partial_finish().tolist()
        assert jr == B.partial_finish().tolist() == want[mid:]


LAYOUTS = [dict(split=0, hash_dedup=1, pairs=2, lines=1, defer_pct=75), dict(split=0, hash_dedup=1, pairs=1, lines=0),
           dict(split=0, hash_dedup=1, timing=1)]


@pytest.mark.parametrize("cfg", LAYOUTS, ids=["pairs2_lines_defer75", "pairs1_nolines", "timed"])
def test_bulk_layouts(B, s4, cfg):
    d = open_dev(**cfg)
    try:
        parity(d, B, "s4", s4, [1] * s4["n_jobs"])
        if cfg.get("timing"):
            d.verify(s4)
            assert d.last_stats.stage_ms[1] > 0  # hash_to_g2: both kernels sit inside the stage's events
    finally:
        d.close()


def test_auto_is_off(B, s4):
    """the measured decision: a context that does not ask for the grouping launches the kernels it always launched"""
    d = open_dev(split=0)
    try:
        ref = reference(B, "s4", s4)
        jr, sc = d.verify(s4)
        assert d.hash_stats() == {"sets": N4, "hashes": N4, "dedup": 0}
        assert jr.tolist() == ref["jr"] and sc.tolist() == ref["sc"]
    finally:
        d.close()


def test_latency_mode_hashes_every_set(B, s4):
    d = open_dev(split=1, hash_dedup=1)
    try:
        ref = reference(B, "s4", s4)
        got = run(d, s4)
        assert got["hash_stats"] == {"sets": N4, "hashes": N4, "dedup": 0}
        assert got["jr"] == ref["jr"] and got["sc"] == ref["sc"]
        assert got["h_aff"].tobytes() == ref["h_aff"].tobytes()
    finally:
        d.close()


def test_three_batches_in_flight(autos, B):
    """per-context tables and a per-call key: three grouping contexts verify differently seeded batches at once"""
    batches = [shape4(autos[0], 100 + k) for k in range(3)]
    refs = [run(B, a) for a in batches]
    out, errs = [None] * 3, []

    def work(k):
        try:
            out[k] = run(autos[k], batches[k])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(3):
        assert out[k]["hash_stats"] == {"sets": N4, "hashes": 104, "dedup": 1}
        assert out[k]["jr"] == refs[k]["jr"] == [1] * batches[k]["n_jobs"] and out[k]["sc"] == refs[k]["sc"]
        assert out[k]["stats"] == refs[k]["stats"]
        assert out[k]["h_aff"].tobytes() == refs[k]["h_aff"].tobytes()


def test_same_message_entry_reports_zeros(A, s3):
    n = s3["n_sets"]
    A.verify(s3)
    assert A.hash_stats()["sets"] == n
    po = s3["pk_offsets"]
    sm = {"n_sets": 1, "n_groups": 1, "group_offsets": np.array([0, 1], np.uint32),
          "pk_indices": s3["pk_indices"][:1].copy(), "msgs": s3["msgs"][:1].copy(), "sigs": s3["sigs"][:1].copy(),
          "sig_len": s3["sig_len"][:1].copy(), "scalars": s3["scalars"][:1].copy()}
    assert po[0] == 0
    A.verify_same_message(sm)
    assert A.hash_stats() == {"sets": 0, "hashes": 0, "dedup": 0}
