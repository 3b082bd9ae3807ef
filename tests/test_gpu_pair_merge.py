"""One Miller pair per distinct signing root of a job (bgv_pair_merge, bgv_pair_stats,
bgv_debug_pair_classes): contexts that merge against one that pairs every set, on
the same batches with injected scalars, in the bulk layout with the one-lane loop
(split=0, miller=1).  The unmerged path is pinned to the golden values by the stage
tests; here everything observable must be equal (job results, set codes, counters,
the final exponentiations of every job product and of the batch product), the
classes must partition every job exactly by root, and every class key must be the
oracle's sum of the reference context's scaled keys.  Run on an MI355X (-m gpu)."""
import hashlib
import threading

import numpy as np
import pytest

from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu

SEED = 0x50414952
N_KEYS = 512
INDEX_RANGE = 9   # BGV_SET_INDEX_RANGE
BAD_ENCODING = 1  # BLST_BAD_ENCODING
BULK = dict(split=0, miller=1)  # the layout that merges
COUNTERS = ("batch_retries", "batch_sigs_success", "pubkeys_aggregated", "n_sets", "n_jobs")
JOBS_A = [130, 65, 64, 3, 2, 1]


def open_dev(**cfg):
    from lodestar_amd import native
    d = native.Device(0, **cfg)
    d.gen_keys(0, N_KEYS, SEED)
    return d


@pytest.fixture(scope="module")
def merged():
    """three contexts that merge"""
    ds = [open_dev(pair_merge=True, **BULK) for _ in range(3)]
    yield ds
    for d in ds:
        d.close()


@pytest.fixture(scope="module")
def A(merged):
    return merged[0]


@pytest.fixture(scope="module")
def B():
    """the reference: the same layout, one pair per set"""
    d = open_dev(**BULK)
    yield d
    d.close()


def root(tag, k):
    return np.frombuffer(hashlib.sha256(b"pair merge %s %d" % (tag, k)).digest(), np.uint8).copy()


def make_batch(dev, rng, set_root, job_sizes, counts=None, indices=None):
    """a signed batch of table keys (1 to 4 per set unless given) with injected scalars"""
    n = len(set_root)
    assert sum(job_sizes) == n
    counts = rng.integers(1, 5, size=n) if counts is None else np.asarray(counts)
    a = {"n_sets": n, "n_jobs": len(job_sizes),
         "job_offsets": np.concatenate([[0], np.cumsum(job_sizes)]).astype(np.uint32),
         "pk_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32),
         "pk_indices": (rng.integers(0, N_KEYS, size=int(counts.sum())) if indices is None else np.asarray(indices)).astype(np.uint32),
         "msgs": np.ascontiguousarray(set_root, np.uint8),
         "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)}
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "pk_offsets", "pk_indices", "msgs")}, sigs)
    a["sigs"] = sigs
    a["sig_len"] = np.full(n, 96, np.uint32)
    return a


def job_of(a, i):
    return int(np.searchsorted(a["job_offsets"], i, side="right")) - 1


def class_keys(a):
    """(job, root) of every set"""
    return [(job_of(a, i), a["msgs"][i].tobytes()) for i in range(a["n_sets"])]


def n_pairs(a):
    return len(set(class_keys(a)))


@pytest.fixture(scope="module")
def sA(A):
    """shape A, 265 sets: 130 sets over three interleaved roots (classes of 44, 43 and 43 that cross waves and items),
    65 of one root, 64 distinct, (a, b, a), 2 of one root, 1; root a is also one of the three of the first job"""
    rng = np.random.default_rng(1)
    ra, rb = root(b"a", 0), root(b"b", 0)
    three = [ra, root(b"three", 1), root(b"three", 2)]
    roots = [three[i % 3] for i in range(130)] + [root(b"one", 0)] * 65 + [root(b"distinct", k) for k in range(64)]
    roots += [ra, rb, ra] + [root(b"two", 0)] * 2 + [root(b"last", 0)]
    a = make_batch(A, rng, np.stack(roots), JOBS_A)
    assert a["n_sets"] == 265 and n_pairs(a) == 3 + 1 + 64 + 2 + 1 + 1
    return a


@pytest.fixture(scope="module")
def sB(A):
    """shape B: one job of 300 sets over 7 roots (span above 256: the tree fold) and a 5-set job"""
    rng = np.random.default_rng(2)
    roots = [root(b"tree", int(k)) for k in rng.integers(0, 7, size=300)] + [root(b"tree", 0), root(b"tail", 1)] * 2 + [root(b"tail", 2)]
    a = make_batch(A, rng, np.stack(roots), [300, 5])
    assert n_pairs(a) == 7 + 3
    return a


_REF = {}


def stats_of(dev):
    return {k: int(getattr(dev.last_stats, k)) for k in COUNTERS}


def reference(B, name, a):
    """the unmerged context's outputs, computed once per batch and left unchanged"""
    if name not in _REF:
        jr, sc = B.verify(a)
        st = stats_of(B)
        assert B.pair_stats() == {"sets": a["n_sets"], "pairs": a["n_sets"], "merged": 0, "fallback": 0}
        dbg = B.debug_stages(a)
        assert B.pair_stats() == {"sets": 0, "pairs": 0, "merged": 0, "fallback": 0}  # the per-set plan reports nothing
        assert dbg["job_result"].tolist() == jr.tolist() and dbg["set_code"].tolist() == sc.tolist()
        _REF[name] = {"jr": jr.tolist(), "sc": sc.tolist(), "stats": st, "rpk": dbg["rpk_aff"].copy(),
                      "job_fe": dbg["job_fe"].copy(), "batch_fe": dbg["batch_fe"].copy()}
    return _REF[name]


def g1_of(row):
    b = row.tobytes()
    return None if b == bytes(96) else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def g1_bytes(pt):
    return bytes(96) if pt is None else (pt[0] % O.P).to_bytes(48, "big") + (pt[1] % O.P).to_bytes(48, "big")


def check_classes(a, out, rpk):
    """cls partitions every job exactly by root inside class_off; p_class is the oracle's sum of the members' keys"""
    cls, off = out["cls"].tolist(), out["class_off"].tolist()
    keys = class_keys(a)
    by_key, by_cls = {}, {}
    for i, (k, c) in enumerate(zip(keys, cls)):
        assert off[k[0]] <= c < off[k[0] + 1], i
        assert by_key.setdefault(k, c) == c and by_cls.setdefault(c, k) == k, i
    assert off[0] == 0 and off[-1] == len(by_key) == len(out["p_class"])
    for j in range(a["n_jobs"]):
        assert off[j + 1] - off[j] == len({k for k in by_key if k[0] == j})
    sums = {}
    for i, c in enumerate(cls):
        sums[c] = O.E1.add(sums.get(c), g1_of(rpk[i])) if c in sums else g1_of(rpk[i])
    for c, pt in sums.items():
        assert out["p_class"][c].tobytes() == g1_bytes(pt), c


def parity(dev, B, name, a, want_jr, fallback=0, classes=True):
    """a merged context against the reference on one batch; returns the merged context's debug outputs"""
    ref = reference(B, name, a)
    jr, sc = dev.verify(a)
    ps, st = dev.pair_stats(), stats_of(dev)
    print(name, "pair_stats", ps, "stats", st)
    n = a["n_sets"]
    assert ps == ({"sets": n, "pairs": n, "merged": 0, "fallback": 1} if fallback else
                  {"sets": n, "pairs": n_pairs(a), "merged": 1, "fallback": 0})
    assert jr.tolist() == ref["jr"] == want_jr
    assert sc.tolist() == ref["sc"]
    assert st == ref["stats"]
    out = dev.debug_pair_classes(a)
    assert dev.pair_stats() == ps
    assert out["job_result"].tolist() == ref["jr"] and out["set_code"].tolist() == ref["sc"]
    assert out["job_fe"].tobytes() == ref["job_fe"].tobytes()
    assert out["batch_fe"].tobytes() == ref["batch_fe"].tobytes()
    if classes:
        check_classes(a, out, ref["rpk"])
    return out


def cref_job(dev, a, j, expect):
    """job j re-verified by the C restatement of the reference"""
    from oracle import cref
    jo, po, idx = a["job_offsets"], a["pk_offsets"], a["pk_indices"]
    table = np.frombuffer(dev.pubkeys_get(0, dev.pubkeys_count()), np.uint8).reshape(-1, 96)
    pks, msgs, sigs = [], [], []
    for i in range(int(jo[j]), int(jo[j + 1])):
        pks.append(cref.aggregate([table[int(r)].tobytes() for r in idx[po[i]:po[i + 1]]]))
        msgs.append(a["msgs"][i].tobytes())
        sigs.append(a["sigs"][i, : int(a["sig_len"][i])].tobytes())
    assert cref.verify_job(pks, msgs, sigs) == expect, j


# ------------------------------------------------------------------- shapes
def test_shape_a(A, B, sA):
    parity(A, B, "sA", sA, [1] * 6)
    assert A.hash_stats() == {"sets": 265, "hashes": len({m.tobytes() for m in sA["msgs"]}), "dedup": 1}
    cref_job(A, sA, 3, 1)  # (a, b, a): one clean merged job


LAYOUTS = [dict(pairs=1, lines=0), dict(pairs=2, lines=1, miller_steps=0, defer_pct=75), dict(pairs=4, lines=1, miller_steps=0),
           dict(pairs=2, lines=1, miller_steps=1), dict(prefold=1), dict(timing=1)]


@pytest.mark.parametrize("cfg", LAYOUTS, ids=["pairs1_nolines", "pairs2_lines_defer75", "pairs4_lines", "steps", "prefold", "timed"])
def test_shape_a_layouts(B, sA, cfg):
    d = open_dev(pair_merge=True, **BULK, **cfg)
    try:
        parity(d, B, "sA", sA, [1] * 6)
        if "miller_steps" in cfg:
            assert d.miller_path()["steps"] == cfg["miller_steps"]
        if "pairs" in cfg:
            assert d.last_stats.pairs_per_item == cfg["pairs"] and d.last_stats.lines == cfg["lines"]
    finally:
        d.close()


def test_shape_b_tree_fold(A, B, sB):
    parity(A, B, "sB", sB, [1, 1])


# ------------------------------------------------------------------- faults
def wrong_root_signature(dev, a, i, other):
    """set i's own keys over the root of set `other`: decodes, lies in the group, verifies nothing here"""
    po = a["pk_offsets"]
    one = {"n_sets": 1, "n_jobs": 1, "job_offsets": np.array([0, 1], np.uint32),
           "pk_offsets": np.array([0, po[i + 1] - po[i]], np.uint32),
           "pk_indices": a["pk_indices"][po[i]:po[i + 1]].copy(), "msgs": a["msgs"][other:other + 1].copy()}
    sig = np.zeros((1, 192), np.uint8)
    dev.gen_sign(one, sig)
    return sig[0]


def test_wrong_signature_in_a_class_of_44(A, B, sA):
    """a member of the 44-member class of root a in job 0; job 3 carries root a too and stays valid"""
    a = dict(sA, sigs=sA["sigs"].copy())
    a["sigs"][63] = wrong_root_signature(A, sA, 63, 130)  # set 63: i % 3 == 0, root a
    parity(A, B, "wrong", a, [0, 1, 1, 1, 1, 1])
    assert A.last_stats.batch_retries == 1
    cref_job(A, a, 0, 0)
    cref_job(A, a, 3, 1)


def test_cleared_compression_flag(A, B, sA):
    a = dict(sA, sigs=sA["sigs"].copy())
    a["sigs"][150, 0] &= 0x7F  # a member of the 65-member class
    out = parity(A, B, "undec", a, [1, -BAD_ENCODING, 1, 1, 1, 1])
    assert out["set_code"][150] == BAD_ENCODING


def test_index_past_the_table(A, B, sA):
    a = dict(sA, pk_indices=sA["pk_indices"].copy())
    a["pk_indices"][sA["pk_offsets"][259]] = N_KEYS  # the first a of (a, b, a)
    out = parity(A, B, "ranged", a, [1, 1, 1, -INDEX_RANGE, 1, 1], classes=False)
    assert out["set_code"][259] == INDEX_RANGE
    assert out["p_class"][int(out["cls"][259])].tobytes() == bytes(96)  # a rejected member: the class is inert


# ------------------------------------------------------------ equal scalars
def test_equal_key_root_and_scalar_doubles(A, B):
    rng = np.random.default_rng(5)
    r = root(b"double", 0)
    a = make_batch(A, rng, np.stack([r, r, root(b"double", 1)]), [3], counts=[1, 1, 1], indices=[17, 17, 40])
    a["scalars"][1] = a["scalars"][0]
    out = parity(A, B, "double", a, [1])
    rpk = g1_of(reference(B, "double", a)["rpk"][0])
    assert out["p_class"][int(out["cls"][0])].tobytes() == g1_bytes(O.E1.add(rpk, rpk))


def test_key_beside_its_negation_falls_back(A, B):
    """raw PK and raw -PK with one root and equal scalars, signatures sigma and -sigma: both sets are valid, the class
    sums to the identity, the call runs again unmerged"""
    rng = np.random.default_rng(6)
    r = root(b"neg", 0)
    a = make_batch(A, rng, np.stack([r, r, root(b"neg", 1)]), [3], counts=[1, 1, 2], indices=[23, 23, 5, 6])
    pk = A.pubkeys_get(23, 1)
    y = int.from_bytes(pk[48:], "big")
    a["raw_pks"] = np.frombuffer(pk + pk[:48] + (O.P - y).to_bytes(48, "big"), np.uint8).copy()
    a["n_raw"] = 2
    a["pk_indices"] = np.array([0x80000000, 0x80000001, 5, 6], np.uint32)
    a["sigs"][1] = a["sigs"][0]
    a["sigs"][1, 0] ^= 0x20  # the sign flag: -sigma
    a["scalars"][1] = a["scalars"][0]
    out = parity(A, B, "neg", a, [1], fallback=1, classes=False)
    c = int(out["cls"][0])
    assert out["cls"][1] == c != out["cls"][2] and out["p_class"][c].tobytes() == bytes(96)
    # unequal scalars: no identity, no fallback
    a2 = dict(a, scalars=a["scalars"].copy())
    a2["scalars"][1] += 1
    parity(A, B, "neg2", a2, [1])


# ------------------------------------------------ where it must not engage
@pytest.mark.parametrize("cfg", [dict(split=1), dict(split=0, miller=2)], ids=["latency_mode", "two_lane_loop"])
def test_other_layouts_run_unmerged(B, sA, cfg):
    ref = reference(B, "sA", sA)
    d = open_dev(pair_merge=True, **cfg)
    try:
        jr, sc = d.verify(sA)
        assert d.pair_stats() == {"sets": 265, "pairs": 265, "merged": 0, "fallback": 0}
        assert jr.tolist() == ref["jr"] and sc.tolist() == ref["sc"] and stats_of(d) == ref["stats"]
    finally:
        d.close()


def test_same_message_entry_reports_zeros(A, sA):
    A.verify(sA)
    assert A.pair_stats()["merged"] == 1
    sm = {"n_sets": 1, "n_groups": 1, "group_offsets": np.array([0, 1], np.uint32),
          "pk_indices": sA["pk_indices"][:1].copy(), "msgs": sA["msgs"][:1].copy(), "sigs": sA["sigs"][:1].copy(),
          "sig_len": sA["sig_len"][:1].copy(), "scalars": sA["scalars"][:1].copy()}
    if sA["pk_offsets"][1] == 1:
        assert A.verify_same_message(sm)[0].tolist() == [True]
    else:
        A.verify_same_message(sm)
    assert A.pair_stats() == {"sets": 0, "pairs": 0, "merged": 0, "fallback": 0}


def test_switch_values(A, sA):
    from lodestar_amd import native
    with pytest.raises(native.BgvNativeError):
        A.pair_merge(2)
    A.pair_merge(0)
    try:
        A.verify(sA)
        assert A.pair_stats() == {"sets": 265, "pairs": 265, "merged": 0, "fallback": 0}
    finally:
        A.pair_merge(1)
    A.verify(sA)
    assert A.pair_stats()["merged"] == 1


# -------------------------------------------------------------- other paths
def to_device(a):
    import torch
    out = dict(a)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            flat = np.ascontiguousarray(v)
            view = flat.view(np.uint8) if flat.dtype.itemsize == 1 else flat.view(np.int64) if k == "scalars" else flat.view(np.int32)
            out[k] = torch.from_numpy(view.copy()).to("cuda:0")
    return out


def test_on_device_inputs(A, B, sA):
    ref = reference(B, "sA", sA)
    jr, sc = A.verify(to_device(sA), on_device=True)
    assert A.pair_stats() == {"sets": 265, "pairs": n_pairs(sA), "merged": 1, "fallback": 0}
    assert jr.tolist() == ref["jr"] and sc.tolist() == ref["sc"] and stats_of(A) == ref["stats"]


def test_library_drawn_scalars(A, sA):
    a = {k: v for k, v in sA.items() if k != "scalars"}
    for _ in range(2):  # two draws, the verdicts by construction
        jr, sc = A.verify(a)
        assert jr.tolist() == [1] * 6 and not sc.any() and A.pair_stats()["merged"] == 1
    bad = dict(a, sigs=sA["sigs"].copy())
    bad["sigs"][200] = wrong_root_signature(A, sA, 200, 0)
    jr, _ = A.verify(bad)
    assert jr.tolist() == [1, 1, 0, 1, 1, 1]


def bits_batch(dev, lst):
    """48 committee sets over windows of one resident list, roots shared in runs of 4, in 6 jobs of 8"""
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
            "scalars": rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)}


def test_verify_bits(A, B):
    lst = np.random.default_rng(9).permutation(N_KEYS).astype(np.uint32)
    for d in (A, B):
        d.index_list_set(0, lst)
    try:
        a = bits_batch(A, lst)
        out = []
        for d in (A, B):
            jr, sc = d.verify_bits(a)
            out.append((jr.tolist(), sc.tolist(), stats_of(d)))
            assert d.pair_stats() == {"sets": 48, "pairs": 12 if d is A else 48, "merged": int(d is A), "fallback": 0}
        assert out[0] == out[1] and out[0][0] == [1] * 6 and not any(out[0][1])
        bad = dict(a, sigs=a["sigs"].copy())
        bad["sigs"][9] = a["sigs"][10]  # another set's signature: same root, other keys
        assert A.verify_bits(bad)[0].tolist() == B.verify_bits(bad)[0].tolist() == [1, 0, 1, 1, 1, 1]
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


@pytest.mark.parametrize("fault", [False, True], ids=["clean", "fault_in_the_merged_shard"])
def test_partial_merged_with_unmerged_shard(A, B, sA, fault):
    """jobs 0-1 through a merged context, jobs 2-5 through the unmerged one: the 576 bytes may differ from the
    unmerged shard's, the combined verdict may not"""
    a = sA
    if fault:
        a = dict(sA, sigs=sA["sigs"].copy())
        a["sigs"][63] = wrong_root_signature(A, sA, 63, 130)
    h0, h1 = job_slice(a, 0, 2), job_slice(a, 2, 6)
    m0, sc0, jr0, ok0 = A.partial(h0)
    assert A.pair_stats() == {"sets": 195, "pairs": 4, "merged": 1, "fallback": 0}
    m1, sc1, jr1, ok1 = B.partial(h1)
    assert B.pair_stats() == {"sets": 70, "pairs": 70, "merged": 0, "fallback": 0}
    assert ok0 and ok1 and not sc0.any() and not sc1.any()
    assert B.combine_final([m0, m1]) == (not fault)
    assert A.partial_finish().tolist() == ([0, 1] if fault else [1, 1])
    assert B.partial_finish().tolist() == [1, 1, 1, 1]


def test_three_merged_contexts_at_once(merged, B, sA):
    ref = reference(B, "sA", sA)
    out, errs = [None] * 3, []

    def work(k):
        try:
            jr, sc = merged[k].verify(sA)
            out[k] = (jr.tolist(), sc.tolist(), stats_of(merged[k]), merged[k].pair_stats())
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(3):
        assert out[k] == (ref["jr"], ref["sc"], ref["stats"], {"sets": 265, "pairs": n_pairs(sA), "merged": 1, "fallback": 0})


def test_python_pool_with_pair_merge(B, sA):
    """the pool's bulk context merges (its layout pinned to the one that does): the reference verdicts, fewer pairs
    than sets in the counters"""
    import asyncio
    from lodestar_amd import verifier as V
    from tests import gpu_util as G
    a = dict(sA, sigs=sA["sigs"].copy())
    a["sigs"][63] = wrong_root_signature(B, sA, 63, 130)
    want = [bool(r) for r in reference(B, "wrong", a)["jr"]]
    assert want == [False, True, True, True, True, True]
    jobs = G.sets_from_arrays({k: v for k, v in a.items() if k != "scalars"})
    pool = V.BlsGpuVerifier(devices=(0,), contexts_per_device=1, pair_merge=True, device_cfg=BULK)
    try:
        for c in pool._contexts():
            c.gen_keys(0, N_KEYS, SEED)
        assert pool._run_device_batch(jobs, [0]) == want
        m = pool.metrics
        assert m["miller_pairs_sets"] == 265 and m["miller_pairs_evaluated"] == n_pairs(sA) < m["miller_pairs_sets"]
        assert m["hash_to_g2_sets"] == 265 and m["hash_to_g2_evaluated"] == len({r.tobytes() for r in sA["msgs"]})
    finally:
        asyncio.run(pool.close())
