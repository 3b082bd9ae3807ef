"""Host side of committee sets in the same-message entry
(lodestar_amd/verifier.py, lodestar_amd/napi/index.js): the two encoders
against hand-built arrays, the routing rule with a fake device (no committee
set: the old encoder's arrays, byte for byte, on the old device call), the
caller-side checks and the addon's exports.  No GPU."""
import asyncio
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from lodestar_amd import native
from lodestar_amd import verifier as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = native.SRC_EXPLICIT
RAW = bytes(range(96))
M1, M2 = bytes([1]) * 32, bytes([2]) * 32
BITS_13 = bytes([0b10110101, 0b00010010])  # 13 members, 7 of them


def _groups():
    """two groups: committee sets, explicit sets as PublicKeys and as indices, a raw key, a malformed signature"""
    return [
        (M1, [(V.CommitteeKeys(V.CommitteeRef(0, 64, 128), b"\xff" * 15 + b"\x7f"), b"\xa1" * 96),
              ([V.PublicKey(index=5), V.PublicKey(raw=RAW), V.PublicKey(index=3)], b"\xa2" * 192),
              (V.CommitteeKeys(V.CommitteeRef(1, 1, 13), BITS_13), b"\xa3" * 7)]),
        (M2, [([9, 8], b"\xa4" * 96),
              (V.CommitteeKeys(V.CommitteeRef(1, 0, 512), b"\xff" * 64), b"\xa5" * 96),
              ([V.PublicKey(raw=RAW)], b"\xa6" * 96)]),
    ]


def test_encode_same_message_bits_against_hand_built_arrays():
    sc = np.arange(1, 7, dtype=np.uint64)
    a = V.encode_same_message_bits(_groups(), sc)
    assert a["n_sets"] == 6 and a["n_groups"] == 2 and a["group_offsets"].tolist() == [0, 3, 6]
    assert a["group_offsets"].dtype == np.uint32
    assert a["src"].dtype == native.SET_SRC_DTYPE and a["src"].flags["C_CONTIGUOUS"]
    assert [tuple(int(v) for v in s) for s in a["src"]] == [(0, 64, 128, 0), (X, 0, 3, 0), (1, 1, 13, 16), (X, 3, 2, 0),
                                                            (1, 0, 512, 18), (X, 5, 1, 0)]
    assert a["bits_len"] == 16 + 2 + 64 == a["bits"].size and a["bits"].dtype == np.uint8
    assert a["bits"].tobytes() == b"\xff" * 15 + b"\x7f" + BITS_13 + b"\xff" * 64
    assert a["n_indices"] == 6 and a["pk_indices"].tolist() == [5, 0x80000000, 3, 9, 8, 0x80000000]  # one raw row, used twice
    assert a["n_raw"] == 1 and a["raw_pks"].tobytes() == RAW
    assert a["msgs"].shape == (2, 32) and a["msgs"].tobytes() == M1 + M2  # one root per GROUP
    assert a["sig_len"].tolist() == [96, 192, 7, 96, 96, 96] and not a["sigs"][2].any()
    assert a["sigs"][1].tobytes() == b"\xa2" * 192 and a["sigs"][0, :96].tobytes() == b"\xa1" * 96
    assert a["scalars"] is sc
    # what the C check makes of it
    from tools import build
    build.build()
    assert native.smb_check(a, [4400, 513]) == (native.BGV_OK, "")
    st, msg = native.smb_check(a, [4400, 511])
    assert st == native.BGV_E_INVALID_ARG and "set 4" in msg
    # all explicit: the sources run over the same pk_indices encode_same_message_agg gives
    plain = [(m, [s for s in sets if not isinstance(s[0], V.CommitteeKeys)]) for m, sets in _groups()]
    b, e = V.encode_same_message_bits(plain), V.encode_same_message_agg(plain)
    assert b["pk_indices"].tolist() == e["pk_indices"].tolist() and b["bits_len"] == 0
    assert b["src"]["off"].tolist() == e["pk_offsets"][:-1].tolist()
    assert b["src"]["len"].tolist() == np.diff(e["pk_offsets"]).tolist()
    for k in ("group_offsets", "msgs", "sigs", "sig_len"):
        assert np.array_equal(b[k], e[k]), k


def test_encoder_refusals():
    with pytest.raises(V.BlsError):
        V.encode_same_message_bits([(M1, [])])
    with pytest.raises(V.BlsError):
        V.encode_same_message_bits([(M1[:31], [([1], b"")])])
    with pytest.raises(V.BlsError):
        V.encode_same_message_bits([(M1, [([], b"")])])
    with pytest.raises(V.BlsError):
        V.encode_same_message_bits([(M1, [(V.CommitteeKeys(V.CommitteeRef(0, 0, 9), b"\x01"), b"")])])  # one byte short


class FakeDevice:
    def __init__(self):
        self.calls = []
        self.last_sm_stats = native.BgvSmStats()
        self.last_sm_stats.groups_retried = 1

    def verify_same_message_agg(self, arrays, **kw):
        self.calls.append(("verify_same_message_agg", arrays))
        return np.ones(arrays["n_sets"], bool), np.zeros(arrays["n_sets"], np.int32)

    def verify_same_message_bits(self, arrays, **kw):
        self.calls.append(("verify_same_message_bits", arrays))
        ok = np.ones(arrays["n_sets"], bool)
        ok[0] = False
        return ok, np.zeros(arrays["n_sets"], np.int32)

    def bits_path_stats(self):
        self.calls.append(("bits_path_stats", None))
        return {"sets_complement": 2, "keys_expanded": 777, "keys_gathered": 3}


def _calls(with_committee):
    (m1, s1), (m2, s2) = _groups()
    if not with_committee:
        s1 = [s for s in s1 if not isinstance(s[0], V.CommitteeKeys)]
        s2 = [s for s in s2 if not isinstance(s[0], V.CommitteeKeys)]
    return [(s1, m1), (s2, m2), (s2[:1], m1)]  # the third call shares the first one's root


def test_routing_rule_without_committee_sets_is_the_old_path():
    calls = _calls(False)
    dev, metrics = FakeDevice(), {}
    sc = np.arange(1, 5, dtype=np.uint64)
    out = V.run_same_message_agg_calls(dev, calls, lambda n: sc[:n], metrics)
    assert out == [[True], [True, True], [True]]
    assert [c[0] for c in dev.calls] == ["verify_same_message_agg"]  # and the path counters are not asked
    a = dev.calls[0][1]
    groups, _ = V.merge_same_message(calls)
    e = V.encode_same_message_agg(groups, sc[:4])
    assert set(a) == set(e)
    for k, v in e.items():
        if isinstance(v, np.ndarray):
            assert a[k].dtype == v.dtype and a[k].tobytes() == v.tobytes(), k
        else:
            assert a[k] == v, k
    assert metrics == {"same_message_agg_sets_started": 4, "same_message_agg_retries": 1, "aggregated_pubkeys_total": 8}


def test_routing_rule_with_a_committee_set_is_the_new_entry():
    calls = _calls(True)
    dev, metrics = FakeDevice(), {"aggregated_pubkeys_total": 1000}
    out = V.run_same_message_agg_calls(dev, calls, None, metrics)
    assert [c[0] for c in dev.calls] == ["verify_same_message_bits", "bits_path_stats"]
    a = dev.calls[0][1]
    # merged: the third call joins the first group
    assert a["n_sets"] == 7 and a["n_groups"] == 2 and a["group_offsets"].tolist() == [0, 4, 7]
    assert [int(x) for x in a["src"]["list"]] == [0, X, 1, X, X, 1, X]
    assert a["scalars"] is None and "pk_offsets" not in a
    assert out == [[False, True, True], [True, True, True], [True]]
    # the key count comes from the device
    assert metrics == {"aggregated_pubkeys_total": 1777, "same_message_agg_sets_started": 7, "same_message_agg_retries": 1}
    # one committee set among explicit ones is enough
    one = [([([1, 2], b"\xaa" * 96), (V.CommitteeKeys(V.CommitteeRef(0, 0, 8), b"\x0f"), b"\xab" * 96)], M1)]
    dev = FakeDevice()
    V.run_same_message_agg_calls(dev, one, None, None)
    assert [c[0] for c in dev.calls] == ["verify_same_message_bits"]


def test_both_verifiers_route_by_set_kind():
    st = object.__new__(V.BlsGpuSingleThreadVerifier)
    st.device, st._closed, st.metrics = FakeDevice(), False, {}
    (m1, s1), _ = _groups()
    explicit = [s for s in s1 if not isinstance(s[0], V.CommitteeKeys)]
    assert asyncio.run(st.verify_aggregate_sets_same_message(explicit, m1)) == [True]
    assert asyncio.run(st.verify_aggregate_sets_same_message(s1, m1)) == [False, True, True]
    assert [c[0] for c in st.device.calls] == ["verify_same_message_agg", "verify_same_message_bits", "bits_path_stats"]
    assert st.metrics["aggregated_pubkeys_total"] == 3 + 777

    import threading
    pool = object.__new__(V.BlsGpuVerifier)
    pool.devices = [FakeDevice()]
    pool._ctx_dev, pool.n_devices, pool.prio_reserved = [0], 1, False
    pool._dev_locks, pool._idle = [threading.Lock()], [True]
    pool.metrics, pool._rng = V._new_metrics(), None
    assert pool._run_same_message_agg([(s1, m1)]) == [[False, True, True]]
    assert pool._run_same_message_agg([(explicit, m1)]) == [[True]]
    assert [c[0] for c in pool.devices[0].calls] == ["verify_same_message_bits", "bits_path_stats", "verify_same_message_agg"]


def test_caller_side_checks_of_committee_keys():
    ok = (V.CommitteeKeys(V.CommitteeRef(0, 0, 9), b"\x01\x01"), b"\xaa" * 96)
    V.check_aggregate_same_message([ok, ([1, 2], b"")], M1)
    bad = [
        V.CommitteeKeys(V.CommitteeRef(0, 0, 9), b"\x01"),        # one byte short
        V.CommitteeKeys(V.CommitteeRef(0, 0, 8), b"\x01\x00"),    # one byte long
        V.CommitteeKeys(V.CommitteeRef(8, 0, 8), b"\x01"),        # no such list
        V.CommitteeKeys(V.CommitteeRef(-1, 0, 8), b"\x01"),
        V.CommitteeKeys(V.CommitteeRef(0, 0, 16), b"\x00\x00"),   # nobody signed
        V.CommitteeKeys(V.CommitteeRef(0, 0xFFFFFFFF, 8), b"\x01"),
        V.CommitteeKeys(None, b"\x01"),
    ]
    for k in bad:
        with pytest.raises(V.BlsError):
            V.check_aggregate_same_message([ok, (k, b"")], M1)
    with pytest.raises(V.BlsError) as e:
        V.check_aggregate_same_message([(bad[4], b"")], M1)
    assert "EMPTY_AGGREGATE_ARRAY" in str(e.value)
    with pytest.raises(V.BlsError):
        V.check_aggregate_same_message([ok], M1[:31])  # the root is 32 bytes


# ------------------------------------------------------------ Node
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_same_message_bits_entries():
    from tools import build as B
    addon = B.build_addon()
    if addon is None:
        pytest.skip("node_api.h not found")
    script = f"""
const a = require({addon!r});
for (const k of ["verifySameMessageBits", "verifySameMessageBitsSync"]) if (typeof a[k] !== "function") throw Error("missing " + k);
const v = require({os.path.join(ROOT, "lodestar_amd", "napi", "index.js")!r});
for (const k of ["encodeSameMessageBits", "hasCommitteeKeys"]) if (typeof v[k] !== "function") throw Error("missing " + k);
console.log("ok");
"""
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_encoder_equals_the_python_encoder(tmp_path):
    """encodeSameMessageBits on the groups of this file against encode_same_message_bits, array by array, and the
    caller-side checks of checkAggregateSameMessage"""
    from tools import build as B
    if B.build_addon() is None:
        pytest.skip("node_api.h not found")
    a = V.encode_same_message_bits(_groups())
    want = {"groupOffsets": a["group_offsets"].tolist(), "src": a["src"].view(np.uint32).tolist(), "bits": a["bits"].tolist(),
            "pkIndices": a["pk_indices"].tolist(), "msgs": a["msgs"].reshape(-1).tolist(), "sigs": a["sigs"].reshape(-1).tolist(),
            "sigLen": a["sig_len"].tolist(), "rawPks": a["raw_pks"].tolist()}
    (tmp_path / "want.json").write_text(json.dumps(want))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "same_message_bits_test.js"), "--host", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same message bits host checks OK" in r.stdout
