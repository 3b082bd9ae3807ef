"""Host side of the committee set kind (lodestar_amd/verifier.py):
encode_jobs_bits against a pure-Python intersectValues, the routing rule of
both verifiers (no committee set: the old encoder's arrays, byte for byte, on
the old device call) and the caller-side checks.  No GPU."""
import asyncio

import numpy as np
import pytest

from lodestar_amd import native
from lodestar_amd import verifier as V

X = native.SRC_EXPLICIT


def intersect_values(bits: bytes, length: int, values: list) -> list:
    """BitArray.intersectValues: the values whose bit is set; throws on a length mismatch"""
    if len(values) != length or len(bits) != (length + 7) // 8:
        raise ValueError("length mismatch")
    return [values[j] for j in range(length) if (bits[j >> 3] >> (j & 7)) & 1]


def expand(arrays: dict, lists: dict) -> tuple[list, list]:
    """(pk_offsets, pk_indices) a bits batch stands for"""
    off, idx = [0], []
    bits = arrays["bits"].tobytes()
    for s in arrays["src"][: arrays["n_sets"]]:
        lst, o, ln, bo = (int(s[k]) for k in ("list", "off", "len", "bits_off"))
        if lst == X:
            idx += arrays["pk_indices"][o : o + ln].tolist()
        else:
            idx += intersect_values(bits[bo : bo + (ln + 7) // 8], ln, lists[lst][o : o + ln])
        off.append(len(idx))
    return off, idx


def _bits(length, rng, p=0.5):
    b = bytearray((length + 7) // 8)
    for j in range(length):
        if rng.random() < p:
            b[j >> 3] |= 1 << (j & 7)
    if not any(b):
        b[0] |= 1
    return bytes(b)


def _jobs():
    rng = np.random.default_rng(5)
    root = lambda k: bytes([k]) * 32  # noqa: E731
    raw = bytes(range(96))
    jobs = [
        [V.create_single_signature_set_from_components(V.PublicKey(index=11), root(1), b"\xa1" * 96),
         V.create_committee_signature_set_from_components(V.CommitteeRef(0, 64, 128), _bits(128, rng), root(2), b"\xa2" * 96),
         V.create_aggregate_signature_set_from_components([V.PublicKey(index=i) for i in (5, 4, 3)], root(3), b"\xa3" * 192)],
        [V.create_committee_signature_set_from_components(V.CommitteeRef(1, 0, 512), _bits(512, rng, 0.99), root(4), b"\xa4" * 96)],
        [V.create_single_signature_set_from_components(V.PublicKey(raw=raw), root(5), b"\xa5" * 96),
         V.create_committee_signature_set_from_components(V.CommitteeRef(0, 1, 13), _bits(13, rng), root(6), b"\xa6" * 7),
         V.create_aggregate_signature_set_from_components([V.PublicKey(raw=raw), V.PublicKey(index=9)], root(7), b"\xa7" * 96)],
    ]
    return jobs


LISTS = {0: [int(x) for x in np.random.default_rng(1).permutation(4400)], 1: [int(x) for x in np.random.default_rng(2).permutation(512)]}


def test_encode_jobs_bits_against_intersect_values():
    jobs = _jobs()
    sc = np.arange(1, 8, dtype=np.uint64)
    a = V.encode_jobs_bits(jobs, sc)
    assert a["n_sets"] == 7 and a["n_jobs"] == 3 and a["job_offsets"].tolist() == [0, 3, 4, 7]
    assert a["src"].dtype == native.SET_SRC_DTYPE and a["src"].flags["C_CONTIGUOUS"]
    assert [int(x) for x in a["src"]["list"]] == [X, 0, X, 1, X, 0, X]
    assert a["src"]["len"].tolist() == [1, 128, 3, 512, 1, 13, 2]
    assert a["src"]["off"].tolist() == [0, 64, 1, 0, 4, 1, 5]
    assert a["src"]["bits_off"].tolist() == [0, 0, 0, 16, 0, 80, 0]  # byte-packed, any alignment
    assert a["bits_len"] == 16 + 64 + 2 == a["bits"].size and a["bits"].dtype == np.uint8
    assert a["n_indices"] == 7 and a["pk_indices"].tolist() == [11, 5, 4, 3, 0x80000000, 0x80000000, 9]
    assert a["n_raw"] == 1 and a["raw_pks"].tobytes() == bytes(range(96))
    assert a["scalars"] is sc
    # the expansion is what the explicit encoder gives for the same sets after intersectValues
    flat = []
    for job in jobs:
        out = []
        for s in job:
            if s.type == V.SignatureSetType.committee:
                c = s.committee
                rows = intersect_values(s.bits, c.length, LISTS[c.list_id][c.offset : c.offset + c.length])
                out.append(V.create_aggregate_signature_set_from_components([V.PublicKey(index=i) for i in rows],
                                                                            s.signingRoot, s.signature))
            else:
                out.append(s)
        flat.append(out)
    e = V.encode_jobs(flat, sc)
    off, idx = expand(a, LISTS)
    assert off == e["pk_offsets"].tolist() and idx == e["pk_indices"].tolist()
    for k in ("msgs", "sigs", "sig_len", "job_offsets"):
        assert np.array_equal(a[k], e[k]), k
    assert a["sig_len"].tolist() == [96, 96, 192, 96, 96, 7, 96] and not a["sigs"][5].any()
    assert V.get_aggregated_pubkeys_count([s for j in jobs for s in j]) == e["pk_offsets"][-1] - 2  # the two singles


def test_routing_rule_without_committee_sets_is_the_old_path():
    jobs = [[s for s in job if s.type != V.SignatureSetType.committee] for job in _jobs()]
    jobs = [j for j in jobs if j]
    sc = np.arange(1, 5, dtype=np.uint64)
    use_bits, a = V.encode_device_batch(jobs, sc)
    e = V.encode_jobs(jobs, sc)
    assert use_bits is False and set(a) == set(e)
    for k, v in e.items():
        if isinstance(v, np.ndarray):
            assert a[k].dtype == v.dtype and a[k].tobytes() == v.tobytes(), k
        else:
            assert a[k] == v, k
    use_bits, a = V.encode_device_batch(_jobs(), None)
    assert use_bits is True and "src" in a and "pk_offsets" not in a


class FakeDevice:
    def __init__(self):
        self.calls = []
        self.last_stats = native.BgvStats()

    def verify(self, arrays, **kw):
        self.calls.append(("verify", arrays))
        return np.ones(arrays["n_jobs"], np.int32), None

    def verify_bits(self, arrays, **kw):
        self.calls.append(("verify_bits", arrays))
        return np.ones(arrays["n_jobs"], np.int32), None


def test_both_verifiers_route_by_set_kind():
    plain = [[s for s in _jobs()[0] if s.type != V.SignatureSetType.committee]]
    # single-thread verifier
    st = object.__new__(V.BlsGpuSingleThreadVerifier)
    st.device, st._closed = FakeDevice(), False
    st.metrics = {"aggregated_pubkeys_total": 0, "main_thread_time_s": 0.0, "main_thread_calls": 0}
    assert asyncio.run(st.verify_signature_sets(plain[0])) is True
    assert asyncio.run(st.verify_signature_sets(_jobs()[0])) is True
    assert [c[0] for c in st.device.calls] == ["verify", "verify_bits"]
    assert "pk_offsets" in st.device.calls[0][1] and st.device.calls[1][1]["src"]["len"].tolist() == [1, 128, 3]
    # the pool's device batch: several devices offered, a batch with a committee set goes whole to one context
    import threading
    pool = object.__new__(V.BlsGpuVerifier)
    pool.devices = [FakeDevice(), FakeDevice()]
    pool._ctx_dev, pool.n_devices, pool.prio_reserved = [0, 1], 2, False
    pool._dev_locks = [threading.Lock(), threading.Lock()]
    pool.metrics, pool._rng = V._new_metrics(), None
    assert pool._run_device_batch(_jobs(), [0, 1]) == [True, True, True]
    assert [c[0] for c in pool.devices[0].calls] == ["verify_bits"] and pool.devices[1].calls == []
    assert pool.devices[0].calls[0][1]["n_jobs"] == 3
    assert pool._run_device_batch(plain, [0]) == [True]
    assert pool.devices[0].calls[1][0] == "verify"


def test_caller_side_checks_of_committee_sets():
    ok = V.create_committee_signature_set_from_components(V.CommitteeRef(0, 0, 9), b"\x01\x01", bytes(32), b"\xaa" * 96)
    V.check_sets([ok])
    bad = [
        V.create_committee_signature_set_from_components(V.CommitteeRef(0, 0, 9), b"\x01", bytes(32), b""),       # one byte short
        V.create_committee_signature_set_from_components(V.CommitteeRef(0, 0, 8), b"\x01\x00", bytes(32), b""),   # one byte long
        V.create_committee_signature_set_from_components(V.CommitteeRef(8, 0, 8), b"\x01", bytes(32), b""),       # no such list
        V.create_committee_signature_set_from_components(V.CommitteeRef(0, 0, 16), b"\x00\x00", bytes(32), b""),  # nobody signed
        V.create_committee_signature_set_from_components(V.CommitteeRef(0, 0, 8), b"\x01", bytes(31), b""),       # short root
    ]
    for s in bad:
        with pytest.raises(V.BlsError):
            V.check_sets([s])
    with pytest.raises(V.BlsError):
        V.encode_jobs_bits([[bad[0]]])
