"""Sets given as committee bitfields over resident index lists on the GPU
(bgv_verify_bits, bgv_index_list_set): the expansion kernels against a numpy
expansion over the length / alignment / pattern grid, host and on-device; a
verdict differential against the untouched bgv_verify on the expanded arrays,
clean and with three faults; the clamps of an on-device batch that breaks the
contract; the life cycle of a list.  Run on an MI355X (-m gpu)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x42495453
N_KEYS = 4400
L_BIG, L_SYNC, L_LIFE = 0, 5, 6  # list ids: 4,400 entries, 512 entries, the life-cycle test's own
X = 0xFFFFFFFF
RAW0 = 0x80000000
LENS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 512, 2047, 2048, 2049, 4100]
PATTERNS = ["first", "last", "all", "alt", "r1", "r50", "r99"]
INDEX_RANGE = 9  # BGV_SET_INDEX_RANGE


@pytest.fixture(scope="module")
def lists():
    """both lists are permutations, so a wrong offset shows"""
    return {L_BIG: np.random.default_rng(1).permutation(N_KEYS).astype(np.uint32),
            L_SYNC: np.random.default_rng(2).permutation(N_KEYS)[:512].astype(np.uint32)}


@pytest.fixture(scope="module")
def dev(lists):
    from lodestar_amd import native
    d = native.Device(0)
    d.gen_keys(0, N_KEYS, SEED)
    for k, v in lists.items():
        d.index_list_set(k, v)
    yield d
    d.close()


def pattern_bits(pat, length, rng):
    b = np.zeros(length, bool)
    if pat == "first":
        b[0] = True
    elif pat == "last":
        b[-1] = True
    elif pat == "all":
        b[:] = True
    elif pat == "alt":
        b[::2] = True
    else:
        b = rng.random(length) < {"r1": 0.01, "r50": 0.5, "r99": 0.99}[pat]
        if not b.any():
            b[int(rng.integers(length))] = True
    return b


def pack(b):
    return np.packbits(b, bitorder="little")  # SSZ bit order: bit j is bit j % 8 of byte j / 8


class Builder:
    """a bits batch under construction: sources, the packed bitfields, explicit indices"""

    def __init__(self):
        self.src, self.bits, self.idx = [], bytearray(), []

    def committee(self, list_id, off, b, align=None):
        if align is not None:  # the bitfield starts at a byte offset of this residue mod 4
            while len(self.bits) % 4 != align:
                self.bits.append(0xFF)  # filler that belongs to no set: all ones, so reading it shows
        self.src.append((list_id, off, len(b), len(self.bits)))
        self.bits += pack(b).tobytes()

    def shared(self, list_id, off, length, k):
        """a set over the bitfield of set k"""
        assert length == self.src[k][2]
        self.src.append((list_id, off, length, self.src[k][3]))

    def explicit(self, keys):
        self.src.append((X, len(self.idx), len(keys), 0xFFFFFFF0))  # bits_off is ignored
        self.idx += [int(x) for x in keys]

    def arrays(self, jobs=None):
        from lodestar_amd import native
        n = len(self.src)
        return {"n_sets": n, "n_jobs": len(jobs) - 1 if jobs else 1, "job_offsets": np.array(jobs or [0, n], np.uint32),
                "src": np.array(self.src, native.SET_SRC_DTYPE), "bits": np.frombuffer(bytes(self.bits), np.uint8).copy(),
                "bits_len": len(self.bits), "pk_indices": np.array(self.idx or [0], np.uint32), "n_indices": len(self.idx)}


def np_expand(a, lists):
    """the numpy expansion: (pk_offsets, pk_indices)"""
    out, off = [], [0]
    bits = np.unpackbits(a["bits"], bitorder="little")
    for lst, o, ln, bo in a["src"].tolist():
        if lst == X:
            out.append(a["pk_indices"][o:o + ln])
        else:
            out.append(lists[lst][o:o + ln][bits[8 * bo:8 * bo + ln].astype(bool)])
        off.append(off[-1] + len(out[-1]))
    return np.array(off, np.uint32), np.concatenate(out).astype(np.uint32)


def to_device(a):
    """the arrays of a batch as tensors on the GPU"""
    import torch
    out = dict(a)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            flat = np.ascontiguousarray(v)
            view = flat.view(np.uint8) if flat.dtype.itemsize == 1 else flat.view(np.int32) if k != "scalars" else flat.view(np.int64)
            out[k] = torch.from_numpy(view.copy()).to("cuda:0")
    return out


@pytest.fixture(scope="module")
def grid(lists):
    """~300 sets: every length x every pattern, byte offsets 0..3 mod 4, offsets zero and odd, both lists; explicit
    singles, 33-key sets and a raw key between them; two sets over one bitfield; the last bitfield ends bits"""
    rng = np.random.default_rng(7)
    b = Builder()
    k = 0
    for length in LENS:
        for pat in PATTERNS:
            use_sync = length <= 512 and k % 3 == 0
            room = (512 if use_sync else N_KEYS) - length
            off = 0 if k % 2 == 0 or room == 0 else min(room, 1 + 2 * int(rng.integers(0, 150)))
            if off and off % 2 == 0:
                off -= 1
            b.committee(L_SYNC if use_sync else L_BIG, off, pattern_bits(pat, length, rng), align=k % 4)
            if k % 2 == 1:
                b.explicit([[int(rng.integers(N_KEYS))], rng.integers(0, N_KEYS, size=33), [RAW0]][(k // 2) % 3])
            k += 1
    for _ in range(120):  # random sets up to a sync committee's size
        length = int(rng.integers(1, 513))
        bits = rng.random(length) < rng.random()
        bits[int(rng.integers(length))] = True  # a host batch refuses a set without keys
        b.committee(L_BIG, int(rng.integers(0, N_KEYS - length + 1)), bits, align=None)
    first_128 = next(i for i, s in enumerate(b.src) if s[0] != X and s[2] == 128)
    b.shared(L_SYNC, 301, 128, first_128)  # the same 16 bytes, another window of another list
    b.committee(L_BIG, 1, pattern_bits("r50", 77, rng), align=3)  # ends on the last byte of bits
    assert b.src[-1][3] + 10 == len(b.bits)
    a = b.arrays()
    assert 280 <= a["n_sets"] <= 330
    assert {s[3] % 4 for s in b.src if s[0] != X} == {0, 1, 2, 3}
    return a


def test_expansion_grid_host(dev, lists, grid):
    want_off, want_idx = np_expand(grid, lists)
    off, idx = dev.debug_bits_expand(grid, cap=want_idx.size)
    assert np.array_equal(off, want_off)
    assert np.array_equal(idx, want_idx)
    # a buffer that is too small is refused, with the size it needs
    from lodestar_amd import native
    with pytest.raises(native.BgvNativeError) as e:
        dev.debug_bits_expand(grid, cap=want_idx.size - 1)
    assert e.value.status == native.BGV_E_INVALID_ARG and str(want_idx.size) in str(e.value)


def test_expansion_grid_on_device(dev, lists, grid):
    want_off, want_idx = np_expand(grid, lists)
    off, idx = dev.debug_bits_expand(to_device(grid), on_device=True, cap=want_idx.size)
    assert np.array_equal(off, want_off)
    assert np.array_equal(idx, want_idx)


# ------------------------------------------------------------ verdict differential
FAULT_SET_OFF, FAULT_SET_LEN = 4200, 100  # a window of the big list that only the index-range fault's set reads


@pytest.fixture(scope="module")
def signed(dev, lists):
    """~200 sets in 24 jobs over table rows, signed on the device over the expanded batch; left unchanged"""
    rng = np.random.default_rng(11)
    b = Builder()
    jobs = [0]
    for j in range(24):
        for _ in range(int(rng.integers(6, 13))):
            kind = rng.random()
            if kind < 0.25:
                b.explicit([int(rng.integers(N_KEYS))])
            elif kind < 0.35:
                b.explicit(rng.integers(0, N_KEYS, size=int(rng.integers(2, 40))))
            else:
                length = int(rng.choice([1, 9, 33, 64, 128, 128, 128, 257, 512, 2049]))
                use_sync = length <= 512 and rng.random() < 0.3
                room = (512 if use_sync else FAULT_SET_OFF) - length
                p = [0.02, 0.5, 0.99][int(rng.integers(3))]
                bits = rng.random(length) < p
                bits[int(rng.integers(length))] = True
                b.committee(L_SYNC if use_sync else L_BIG, int(rng.integers(0, room + 1)), bits)
        if j == 20:
            b.committee(L_BIG, FAULT_SET_OFF, np.ones(FAULT_SET_LEN, bool))
        jobs.append(len(b.src))
    a = b.arrays(jobs)
    n = a["n_sets"]
    assert 180 <= n <= 260, n
    a["msgs"] = np.stack([np.frombuffer(hashlib.sha256(b"bits set %d" % i).digest(), np.uint8) for i in range(n)])
    a["scalars"] = rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    po, idx = np_expand(a, lists)
    sigs = np.zeros((n, 192), np.uint8)
    dev.gen_sign({"n_sets": n, "n_jobs": a["n_jobs"], "job_offsets": a["job_offsets"], "pk_offsets": po, "pk_indices": idx,
                  "msgs": a["msgs"]}, sigs)
    a["sigs"] = sigs
    a["sig_len"] = np.full(n, 96, np.uint32)
    return a


def expanded(a, lists):
    po, idx = np_expand(a, lists)
    e = {k: a[k] for k in ("n_sets", "n_jobs", "job_offsets", "msgs", "sigs", "sig_len", "scalars")}
    e["pk_offsets"], e["pk_indices"] = po, idx
    return e


def both_ways(dev, a, lists):
    """bgv_verify_bits on a host batch and on a device batch, and bgv_verify on the expanded arrays"""
    jr_h, sc_h = dev.verify_bits(a)
    agg_h = int(dev.last_stats.pubkeys_aggregated)
    jr_d, sc_d = dev.verify_bits(to_device(a), on_device=True)
    agg_d = int(dev.last_stats.pubkeys_aggregated)
    jr_e, sc_e = dev.verify(expanded(a, lists))
    agg_e = int(dev.last_stats.pubkeys_aggregated)
    assert jr_h.tolist() == jr_e.tolist() and sc_h.tolist() == sc_e.tolist() and agg_h == agg_e
    assert jr_d.tolist() == jr_e.tolist() and sc_d.tolist() == sc_e.tolist() and agg_d == agg_e
    return jr_e, sc_e


def test_verdicts_equal_bgv_verify_on_the_expansion(dev, lists, signed):
    jr, sc = both_ways(dev, signed, lists)
    assert jr.tolist() == [1] * signed["n_jobs"] and not sc.any()
    assert int(dev.last_stats.pubkeys_aggregated) == np_expand(signed, lists)[1].size


def test_three_faults_change_only_their_jobs(dev, lists, signed):
    a = dict(signed)
    jo = a["job_offsets"].tolist()
    src = a["src"].tolist()
    # job 3: a signature that belongs to another set
    a["sigs"] = signed["sigs"].copy()
    a["sigs"][jo[3]] = signed["sigs"][jo[4]]
    # job 9: one participation bit flipped in a committee set that keeps other bits
    a["bits"] = signed["bits"].copy()
    po, _ = np_expand(signed, lists)
    k = next(i for i in range(jo[9], jo[10]) if src[i][0] != X and src[i][2] >= 9 and po[i + 1] - po[i] >= 2)
    a["bits"][src[k][3] + 1] ^= 0x01  # bit 8 of the set
    # job 20: a list entry equal to the table count, read by the set that owns that window alone
    fault_set = next(i for i in range(jo[20], jo[21]) if src[i][:3] == (L_BIG, FAULT_SET_OFF, FAULT_SET_LEN))
    bad = {**lists, L_BIG: lists[L_BIG].copy()}
    bad[L_BIG][FAULT_SET_OFF + 50] = N_KEYS
    dev.index_list_set(L_BIG, bad[L_BIG])
    try:
        jr, sc = both_ways(dev, a, bad)
    finally:
        dev.index_list_set(L_BIG, lists[L_BIG])
    want = [1] * a["n_jobs"]
    want[3], want[9], want[20] = 0, 0, -INDEX_RANGE
    assert jr.tolist() == want
    assert sc[fault_set] == INDEX_RANGE


# ------------------------------------------------------------ device robustness
def test_on_device_source_past_its_list_rejects_only_its_job(dev, lists, signed):
    """the clamp in front of the gather: the broken source expands to one index past any table"""
    a = dict(signed)
    jo = a["job_offsets"].tolist()
    src = signed["src"].copy()
    k = next(i for i in range(a["n_sets"]) if src[i]["list"] == L_SYNC)
    job = int(np.searchsorted(jo, k, side="right")) - 1
    src[k]["off"] = 512 - src[k]["len"] + 1  # off + len is one past the list
    a["src"] = src
    jr, sc = dev.verify_bits(to_device(a), on_device=True)
    want = [1] * a["n_jobs"]
    want[job] = -INDEX_RANGE
    assert jr.tolist() == want
    assert sc[k] == INDEX_RANGE
    po, idx = np_expand(signed, lists)
    assert int(dev.last_stats.pubkeys_aggregated) == idx.size - int(po[k + 1] - po[k]) + 1  # the broken set counts one key
    # the 32-bit wrap: off + len == 2^32 + 16 must not pass as 16
    src[k]["off"], src[k]["len"] = 0xFFFFFFF0, 0x20
    jr, sc = dev.verify_bits(to_device(a), on_device=True)
    assert jr.tolist() == want and sc[k] == INDEX_RANGE
    # the host path refuses the same batch outright
    from lodestar_amd import native
    with pytest.raises(native.BgvNativeError) as e:
        dev.verify_bits(a)
    assert e.value.status == native.BGV_E_INVALID_ARG and f"set {k}" in str(e.value)


def test_on_device_padding_bits_are_masked(dev, lists, signed):
    a = dict(signed)
    src = signed["src"].tolist()
    bits = signed["bits"].copy()
    dirty = [i for i, s in enumerate(src) if s[0] != X and s[2] % 8]
    assert len(dirty) >= 10
    for i in dirty:
        _, _, ln, bo = src[i]
        bits[bo + (ln + 7) // 8 - 1] |= (0xFF << (ln % 8)) & 0xFF
    a["bits"] = bits
    want_off, want_idx = np_expand(signed, lists)
    off, idx = dev.debug_bits_expand(to_device(a), on_device=True, cap=want_idx.size)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    jr, sc = dev.verify_bits(to_device(a), on_device=True)
    assert jr.tolist() == [1] * a["n_jobs"] and not sc.any()
    from lodestar_amd import native
    with pytest.raises(native.BgvNativeError) as e:  # a host batch with such bits is refused
        dev.verify_bits(a)
    assert e.value.status == native.BGV_E_INVALID_ARG and "padding" in str(e.value)


# ------------------------------------------------------------ list life cycle
def test_list_life_cycle(dev):
    from lodestar_amd import native
    rng = np.random.default_rng(3)
    first = rng.permutation(N_KEYS)[:300].astype(np.uint32)
    second = rng.permutation(N_KEYS)[:200].astype(np.uint32)
    b = Builder()
    bits = rng.random(150) < 0.5
    b.committee(L_LIFE, 37, bits)
    a = b.arrays()
    assert dev.index_list_len(L_LIFE) == 0
    with pytest.raises(native.BgvNativeError) as e:  # not set yet
        dev.debug_bits_expand(a, cap=256)
    assert e.value.status == native.BGV_E_INVALID_ARG and f"list {L_LIFE}" in str(e.value)
    dev.index_list_set(L_LIFE, first)
    assert dev.index_list_len(L_LIFE) == 300
    assert np.array_equal(dev.debug_bits_expand(a, cap=256)[1], first[37:187][bits])
    dev.index_list_set(L_LIFE, second)  # replaced between two calls
    assert dev.index_list_len(L_LIFE) == 200
    assert np.array_equal(dev.debug_bits_expand(a, cap=256)[1], second[37:187][bits])
    refused = second.copy()
    refused[77] |= 0x80000000  # lists hold table rows only
    with pytest.raises(native.BgvNativeError) as e:
        dev.index_list_set(L_LIFE, refused)
    assert e.value.status == native.BGV_E_INVALID_ARG and "entry 77" in str(e.value)
    assert dev.index_list_len(L_LIFE) == 200  # unchanged
    assert np.array_equal(dev.debug_bits_expand(a, cap=256)[1], second[37:187][bits])
    beyond = second.copy()
    beyond[0] = N_KEYS + 5  # past the table's current count: allowed, the table may grow
    dev.index_list_set(L_LIFE, beyond)
    assert dev.index_list_len(L_LIFE) == 200
    with pytest.raises(native.BgvNativeError):  # no such list id
        dev.index_list_set(native.MAX_INDEX_LISTS, second)
    dev.index_list_set(L_LIFE, np.zeros(0, np.uint32))  # dropped
    assert dev.index_list_len(L_LIFE) == 0
    with pytest.raises(native.BgvNativeError) as e:
        dev.debug_bits_expand(a, cap=256)
    assert e.value.status == native.BGV_E_INVALID_ARG
    st, _ = native.bits_check({**a, "msgs": np.zeros((1, 32), np.uint8), "sigs": np.zeros((1, 192), np.uint8),
                               "sig_len": np.full(1, 96, np.uint32)}, [0] * 8)
    assert st == native.BGV_E_INVALID_ARG
