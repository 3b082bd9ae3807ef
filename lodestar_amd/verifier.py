"""Host-side mirror of Lodestar's BLS verifier interface, backed by the gfx950
HIP library through the C ABI (lodestar_amd/native.py -> include/bgv.h).

Reference interface (maschad/lodestar, packages/beacon-node/src/chain/bls/):

* ``IBlsVerifier`` (interface.ts:20-51): ``verifySignatureSets(sets, opts)``
  -> Promise<boolean>, ``close()``, ``canAcceptWork()``.  Here:
  ``BlsGpuVerifier.verify_signature_sets`` (a coroutine), ``close``,
  ``can_accept_work``.
* ``VerifySignatureOpts`` {batchable, verifyOnMainThread} (interface.ts:3-18).
* ``ISignatureSet`` single / aggregate (state-transition/src/util/
  signatureSets.ts:5-22).  Pubkeys are references into the HBM-resident
  ``index2pubkey`` table (``PubkeyTable``), so a set carries index lists
  instead of serialized points (BASELINE north_star); raw pubkeys outside
  the table are still accepted (``PublicKey.from_bytes``).
* Pool semantics of ``BlsMultiThreadWorkerPool`` (multithread/index.ts:
  151-431): sets chunked into jobs of <= 128 (``chunkify_maximize_chunk_size``,
  multithread/utils.ts:4-19), batchable jobs buffered up to 100 ms or until
  more than 32 sigs are waiting, job verdict = AND of its sets, the call's
  verdict = AND of its jobs, a job whose signature does not parse rejects
  with ``BLST_ERROR: BLST_<CODE>``, an empty aggregate rejects with
  ``EMPTY_AGGREGATE_ARRAY``, a job of zero sets rejects with
  ``Empty signature set`` (maybeBatch.ts:29-31), ``close()`` rejects pending
  jobs with ``QueueError(QUEUE_ABORTED)`` (multithread/index.ts:193-214).

What differs on purpose: the worker pool packs <= 128 sigs per worker
message (prepareWork, index.ts:405-420) because a CPU worker verifies one
batch at a time; a GPU wants one large batch, so every queued job is packed
into one device batch (bounded by ``max_sets_per_device_batch``).  Verdicts
are unaffected: the device checks the whole batch once and falls back to
per-job checks exactly where the worker retries (worker.ts:64-85).
"""
from __future__ import annotations

import asyncio
import enum
import math
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from . import native
from .dist import RESERVED_CAP, job_work, shard_jobs

MAX_SIGNATURE_SETS_PER_JOB = 128  # multithread/index.ts:39
MAX_BUFFERED_SIGS = 32            # multithread/index.ts:48
MAX_BUFFER_WAIT_MS = 100          # multithread/index.ts:57
MAX_JOBS_CAN_ACCEPT_WORK = 512    # multithread/index.ts:62
PRIORITY_CUS = 32  # CUs of the first device kept for verifyOnMainThread (bgv_cfg.cu_split; one per SE)
# device batches in flight per GPU, one context each (napi/index.js
# CONTEXTS_PER_DEVICE): the next batches' phase 1 fills the SIMDs a batch's
# Miller phase leaves idle (profiles/r06b_overlap_sizes.txt)
CONTEXTS_PER_DEVICE = 3
# the priority context's sizing job (BlsGpuVerifier._warm_priority)
G1_GENERATOR_96 = bytes.fromhex(
    "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
    "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
IDENTITY_SIG_96 = bytes([0xC0]) + bytes(95)
MAX_SETS_PER_DEVICE_BATCH = 1 << 17
# a device batch of at least this many sets (and >= 2 jobs) is split by job
# over the idle devices: each returns a partial Miller product and ONE final
# exponentiation checks their product.  Below it the batch runs
# whole on one device and other devices take the next batch: one GPU verifies
# 2,000-4,000 sets in 7-10 ms, within ~2 ms of the split, which pays a host
# round trip and the combined final exponentiation
SHARD_MIN_SETS = 4096


class BlsError(Exception):
    """Rejection raised by verify_signature_sets; ``message`` follows the
    strings the reference's tests match (multithread.test.ts:97,
    test/spec/general/bls.ts:37)."""

    def __init__(self, message: str, code: int | None = None):
        super().__init__(message)
        self.message = message
        self.code = code


class QueueErrorCode(str, enum.Enum):
    QUEUE_ABORTED = "QUEUE_ERROR_QUEUE_ABORTED"  # util/queue/errors.ts


class QueueError(Exception):
    def __init__(self, code: QueueErrorCode = QueueErrorCode.QUEUE_ABORTED):
        super().__init__(code.value)
        self.code = code


def error_for_code(code: int) -> BlsError:
    if code == 10:
        return BlsError("Empty signature set", code)
    return BlsError(f"BLST_ERROR: {native.SET_CODE_NAMES.get(code, 'BLST_UNKNOWN')}", code)


# --------------------------------------------------------------- data types
class SignatureSetType(str, enum.Enum):
    single = "single"
    aggregate = "aggregate"
    committee = "committee"


@dataclass(frozen=True)
class PublicKey:
    """A trusted pubkey: either a row of the device index2pubkey table
    (``index``) or raw bytes (96 B uncompressed x||y, or 48 B compressed)."""

    index: int | None = None
    raw: bytes | None = None

    @staticmethod
    def from_bytes(b: bytes) -> "PublicKey":
        if len(b) not in (48, 96):
            raise BlsError("BLST_ERROR: BLST_INVALID_SIZE", 8)
        return PublicKey(raw=bytes(b))


@dataclass(frozen=True)
class CommitteeRef:
    """A window of a resident index list (bgv_index_list_set): entries
    [offset, offset + length) of list ``list_id``, e.g. one committee's slice of
    an epoch shuffling, or the whole sync committee."""

    list_id: int
    offset: int
    length: int


@dataclass(frozen=True)
class CommitteeKeys:
    """The keys of one set of verify_aggregate_sets_same_message given as a
    committee and its participation bits, in place of a pubkey list: the members
    of ``committee`` whose bit is set (ceil(length / 8) bytes, SSZ bit order)."""

    committee: CommitteeRef
    bits: bytes


@dataclass
class VerifySignatureOpts:
    batchable: bool = False
    verifyOnMainThread: bool = False


@dataclass
class ISignatureSet:
    type: SignatureSetType
    signingRoot: bytes
    signature: bytes
    pubkey: PublicKey | None = None
    pubkeys: list[PublicKey] = field(default_factory=list)
    committee: CommitteeRef | None = None  # type committee: the keys are the committee members whose bit is set
    bits: bytes | None = None              # ceil(length / 8) bytes, SSZ bit order


def create_single_signature_set_from_components(pubkey: PublicKey, signing_root: bytes, signature: bytes) -> ISignatureSet:
    """util/signatureSets.ts:40-51"""
    return ISignatureSet(SignatureSetType.single, bytes(signing_root), bytes(signature), pubkey=pubkey)


def create_aggregate_signature_set_from_components(pubkeys, signing_root: bytes, signature: bytes) -> ISignatureSet:
    """util/signatureSets.ts:53-64"""
    return ISignatureSet(SignatureSetType.aggregate, bytes(signing_root), bytes(signature), pubkeys=list(pubkeys))


def create_committee_signature_set_from_components(committee: CommitteeRef, bits: bytes, signing_root: bytes,
                                                   signature: bytes) -> ISignatureSet:
    """An aggregate set whose keys are given as (committee, participation bits)
    instead of indices: what the reference holds before
    aggregationBits.intersectValues(committeeIndices) (cache/epochContext.ts:620-623,
    block/processSyncCommittee.ts:89).  The device expands it (bgv_verify_bits)."""
    return ISignatureSet(SignatureSetType.committee, bytes(signing_root), bytes(signature), committee=committee,
                         bits=bytes(bits))


def _popcount(b: bytes) -> int:
    return bin(int.from_bytes(b, "little")).count("1") if b else 0


def get_aggregated_pubkeys_count(sets) -> int:
    """chain/bls/utils.ts:18-26; a committee set counts its set bits"""
    return sum(len(s.pubkeys) if s.type == SignatureSetType.aggregate else _popcount(s.bits)
               for s in sets if s.type != SignatureSetType.single)


def chunkify_maximize_chunk_size(arr: list, min_per_chunk: int) -> list[list]:
    """multithread/utils.ts:4-19: split maximizing the smallest chunk."""
    chunk_count = len(arr) // min_per_chunk
    if chunk_count <= 1:
        return [arr]
    per_chunk = math.ceil(len(arr) / chunk_count)
    return [arr[i : i + per_chunk] for i in range(0, len(arr), per_chunk)]


# ------------------------------------------------------------ pubkey table
class PubkeyTable:
    """``index2pubkey`` resident in HBM (state-transition/src/cache/
    pubkeyCache.ts:6,56-77 syncPubkeys; cache/epochContext.ts:701-704
    addPubkey).  One replica per device."""

    def __init__(self, devices: list[native.Device]):
        self.devices = devices
        self.pubkey2index: dict[bytes, int] = {}

    def __len__(self):
        return self.devices[0].pubkeys_count()

    def sync_pubkeys(self, pubkeys48: list[bytes]):
        """Append every validator pubkey not yet in the table (compressed).
        A key that does not deserialize throws like PublicKey.fromBytes and
        leaves the table unchanged."""
        if len(self.pubkey2index) != len(self):  # pubkeyCache.ts:61-63
            raise BlsError(f"Pubkey indices have fallen out of sync: {len(self.pubkey2index)} != {len(self)}")
        start = len(self)
        new = pubkeys48[start:]
        if not new:
            return
        blob = b"".join(new)
        self._set(start, blob)
        for i, pk in enumerate(new):
            self.pubkey2index[bytes(pk)] = start + i

    def add_pubkey(self, index: int, pubkey48: bytes):
        """epochContext.ts:701-704.  The device table is append-only: index
        may rewrite a row or append the next one, not leave a gap."""
        self._set(index, pubkey48)
        self.pubkey2index[bytes(pubkey48)] = index

    def _set(self, first: int, blob: bytes):
        for d in self.devices:
            try:
                d.pubkeys_set(first, blob, native.PK_COMPRESSED_48)
            except native.BgvNativeError as e:
                if e.status == native.BGV_E_BAD_PUBKEY:
                    raise BlsError(str(e).split(": ", 1)[-1]) from e
                raise

    def __getitem__(self, index: int) -> PublicKey:
        return PublicKey(index=index)


# ------------------------------------------------------- batch marshalling
class _SetArrays:
    """What the five encoders share: the per-set arrays of a batch (include/bgv.h), filled one set at a time by
    keys() or committee(), then signature().  Keys land in pk_indices (table rows, or bit 31 and a row of raw_pks,
    every distinct raw key stored once); a set's keys are delimited by pk_offsets, or with `sources` by a bgv_set_src
    record (an explicit run of pk_indices, or a committee over the packed bitfields)."""

    def __init__(self, n_sets: int, offsets: bool = False, sources: bool = False):
        self.n = 0  # sets finished: the row signature() fills next
        self.idx: list[int] = []
        self.raw: list[bytes] = []
        self.raw_pos: dict[bytes, int] = {}
        self.pk_off = [0] if offsets else None
        self.src = np.zeros(max(n_sets, 1), dtype=native.SET_SRC_DTYPE) if sources else None
        self.bits = bytearray()
        self.sigs = np.zeros((max(n_sets, 1), 192), dtype=np.uint8)
        self.sig_len = np.zeros(max(n_sets, 1), dtype=np.uint32)

    def keys(self, pks) -> None:
        """these keys (PublicKeys) for the current set; none raises like PublicKey.aggregate"""
        if len(pks) == 0:
            raise BlsError("EMPTY_AGGREGATE_ARRAY")
        if self.src is not None:
            self.src[self.n] = (native.SRC_EXPLICIT, len(self.idx), len(pks), 0)
        for pk in pks:
            if pk.index is not None:
                self.idx.append(pk.index)
            else:
                r = pk.raw if len(pk.raw) == 96 else _decompress_raw48(pk.raw)
                if r not in self.raw_pos:
                    self.raw_pos[r] = len(self.raw)
                    self.raw.append(r)
                self.idx.append(0x80000000 | self.raw_pos[r])
        if self.pk_off is not None:
            self.pk_off.append(len(self.idx))

    def committee(self, c: CommitteeRef, bits: bytes) -> None:
        """this committee and bitfield for the current set"""
        if len(bits) != (c.length + 7) // 8:
            raise _bitfield_error(c, bits)
        self.src[self.n] = (c.list_id, c.offset, c.length, len(self.bits))
        self.bits += bits

    def signature(self, sig: bytes) -> None:
        """this signature, which ends the current set; a length other than 96 or 192 leaves the row zero"""
        sl = len(sig)
        self.sig_len[self.n] = sl
        if sl in (96, 192):
            self.sigs[self.n, :sl] = np.frombuffer(bytes(sig), dtype=np.uint8)
        self.n += 1

    def finish(self, msgs: np.ndarray, scalars) -> dict:
        """the entries every encoder's result ends with, after its own head (counts and job or group offsets)"""
        out = {}
        if self.pk_off is not None:
            out["pk_offsets"] = np.array(self.pk_off, dtype=np.uint32)
        if self.src is not None:
            out["src"] = self.src
            out["bits"] = np.frombuffer(bytes(self.bits), dtype=np.uint8).copy() if self.bits else np.zeros(1, np.uint8)
            out["bits_len"] = len(self.bits)
        out["pk_indices"] = np.array(self.idx if self.idx else [0], dtype=np.uint32)
        if self.src is not None:
            out["n_indices"] = len(self.idx)
        out["raw_pks"] = np.frombuffer(b"".join(self.raw), dtype=np.uint8).copy() if self.raw else None
        out.update(n_raw=len(self.raw), msgs=msgs, sigs=self.sigs, sig_len=self.sig_len, scalars=scalars)
        return out


def _put_root(msgs: np.ndarray, row: int, root: bytes) -> None:
    if len(root) != 32:
        raise BlsError("signingRoot must be 32 bytes")
    msgs[row] = np.frombuffer(bytes(root), dtype=np.uint8)


def _set_keys(s: ISignatureSet) -> list:
    return [s.pubkey] if s.type == SignatureSetType.single else s.pubkeys


def encode_jobs(jobs: list[list[ISignatureSet]], scalars: np.ndarray | None = None) -> dict:
    """Flatten jobs of sets into the SoA arrays of bgv_batch (include/bgv.h).
    Raises BlsError("EMPTY_AGGREGATE_ARRAY") like PublicKey.aggregate."""
    n = sum(len(j) for j in jobs)
    acc = _SetArrays(n, offsets=True)
    msgs = np.zeros((max(n, 1), 32), dtype=np.uint8)
    job_off = [0]
    for job in jobs:
        for s in job:
            acc.keys(_set_keys(s))
            _put_root(msgs, acc.n, s.signingRoot)
            acc.signature(s.signature)
        job_off.append(acc.n)
    return {"n_sets": n, "n_jobs": len(jobs), "job_offsets": np.array(job_off, dtype=np.uint32), **acc.finish(msgs, scalars)}


def has_committee_sets(jobs) -> bool:
    return any(s.type == SignatureSetType.committee for job in jobs for s in job)


def encode_jobs_bits(jobs: list[list[ISignatureSet]], scalars: np.ndarray | None = None) -> dict:
    """Flatten jobs of sets into the arrays of bgv_bits_batch (include/bgv.h):
    single and aggregate sets become explicit sources over pk_indices, committee
    sets list sources over the packed bitfields.  Raises BlsError like encode_jobs."""
    n = sum(len(j) for j in jobs)
    acc = _SetArrays(n, sources=True)
    msgs = np.zeros((max(n, 1), 32), dtype=np.uint8)
    job_off = [0]
    for job in jobs:
        for s in job:
            if s.type == SignatureSetType.committee:
                acc.committee(s.committee, s.bits)
            else:
                acc.keys(_set_keys(s))
            _put_root(msgs, acc.n, s.signingRoot)
            acc.signature(s.signature)
        job_off.append(acc.n)
    return {"n_sets": n, "n_jobs": len(jobs), "job_offsets": np.array(job_off, dtype=np.uint32), **acc.finish(msgs, scalars)}


def encode_device_batch(jobs: list[list[ISignatureSet]], scalars: np.ndarray | None = None) -> tuple[bool, dict]:
    """The routing rule of both verifiers: a device batch that holds a committee
    set goes through bgv_verify_bits (True, encode_jobs_bits arrays); any other
    batch takes exactly the path it took before (False, encode_jobs arrays)."""
    if has_committee_sets(jobs):
        return True, encode_jobs_bits(jobs, scalars)
    return False, encode_jobs(jobs, scalars)


def verify_device_batch(device, jobs: list[list[ISignatureSet]], scalars: np.ndarray | None = None):
    """encode_device_batch + the matching device call: job results as Device.verify returns them"""
    use_bits, arrays = encode_device_batch(jobs, scalars)
    call = device.verify_bits if use_bits else device.verify
    return call(arrays, want_set_codes=False)[0]


def _decompress_raw48(b: bytes) -> bytes:
    raise BlsError("raw compressed pubkeys must be added to the table (PubkeyTable.add_pubkey)")


def _check_key(pk) -> None:
    """the caller-side checks of one key: it exists, a raw key is a 96-byte uncompressed point (compressed keys
    live in the table), an index fits the 31 bits pk_indices leaves it"""
    if pk is None:
        raise BlsError("EMPTY_AGGREGATE_ARRAY")
    if pk.index is None and len(pk.raw) != 96:
        _decompress_raw48(pk.raw)
    if pk.index is not None and not (0 <= pk.index < 0x80000000):
        raise BlsError(f"pubkey index {pk.index} out of range")


def _bitfield_error(c: CommitteeRef, bits: bytes) -> BlsError:
    return BlsError(f"committee set: {len(bits)} bitfield bytes for {c.length} members")


def _check_committee(c: CommitteeRef | None, bits: bytes | None) -> None:
    """the caller-side checks of a committee and its participation bits"""
    if c is None or bits is None or not (0 <= c.list_id < native.MAX_INDEX_LISTS):
        raise BlsError("committee set without a committee, bits or a valid list id")
    if c.offset < 0 or c.length < 0 or c.offset + c.length > 0xFFFFFFFF or len(bits) != (c.length + 7) // 8:
        raise _bitfield_error(c, bits)
    if not any(bits):  # intersectValues gives no index: PublicKey.aggregate throws
        raise BlsError("EMPTY_AGGREGATE_ARRAY")


def check_sets(sets: list[ISignatureSet]) -> None:
    """Caller-side checks of one verifySignatureSets call: PublicKey.aggregate
    throws EMPTY_AGGREGATE_ARRAY (chain/bls/utils.ts:11); a raw key must be a
    96-byte uncompressed point (compressed keys live in the table); a signing
    root is 32 bytes.  Pubkey indices past the table are reported per set by
    the device (BGV_INDEX_RANGE rejects only that job)."""
    for s in sets:
        if s.type == SignatureSetType.committee:
            _check_committee(s.committee, s.bits)
        else:
            pks = _set_keys(s)
            if s.type == SignatureSetType.aggregate and len(pks) == 0:
                raise BlsError("EMPTY_AGGREGATE_ARRAY")
            for pk in pks:
                _check_key(pk)
        if len(s.signingRoot) != 32:
            raise BlsError("signingRoot must be 32 bytes")


# ------------------------------------------------- same-message batches
def check_same_message(sets, message: bytes) -> None:
    """Caller-side checks of one verifySignatureSetsSameMessage call, as
    check_sets makes them: every set is (PublicKey, signature) with one key,
    a raw key is a 96-byte uncompressed point, the signing root is 32 bytes."""
    if len(message) != 32:
        raise BlsError("signingRoot must be 32 bytes")
    for pk, _sig in sets:
        _check_key(pk)


def _group_head(msgs: np.ndarray, g: int, message: bytes, sets) -> None:
    """what the group encoders check of a group before its sets, and its row of msgs"""
    if len(sets) == 0:
        raise BlsError("Empty signature set", 10)
    _put_root(msgs, g, message)


def encode_same_message(groups, scalars: np.ndarray | None = None) -> dict:
    """Flatten groups [(message, [(PublicKey, signature), ...]), ...] into the
    arrays of bgv_sm_batch (include/bgv.h): one message per group, one key and
    one signature per set.  An empty group is refused (the library would)."""
    n = sum(len(g[1]) for g in groups)
    acc = _SetArrays(n)
    msgs = np.zeros((max(len(groups), 1), 32), dtype=np.uint8)
    off = [0]
    for g, (message, sets) in enumerate(groups):
        _group_head(msgs, g, message, sets)
        for pk, sig in sets:
            acc.keys((pk,))
            acc.signature(sig)
        off.append(acc.n)
    return {"n_sets": n, "n_groups": len(groups), "group_offsets": np.array(off, dtype=np.uint32), **acc.finish(msgs, scalars)}


@dataclass(frozen=True)
class AggregateRequest:
    """What a verify_and_aggregate_same_message call adds to its sets: the
    pool's running aggregate (96 compressed bytes, None = none) and, per set,
    whether a valid set enters the aggregate (None = every set)."""

    previous: bytes | None = None
    take: tuple | None = None


@dataclass
class SameMessageAggregate:
    """Result of verify_and_aggregate_same_message: one boolean per set, the
    compressed sum of `previous` and the valid, taken signatures, and how many
    signatures were added."""

    valid: list
    aggregate: bytes
    count: int


def merge_same_message_groups(calls):
    """Merge calls [(sets, message[, AggregateRequest]), ...] into the groups of
    ONE device call: one group per call, and plain calls whose messages are
    byte-equal share a group (in order of first appearance).  A call with an
    AggregateRequest ALWAYS forms its own group: its aggregate is per call.
    Returns (groups, where, group_of) with where[k] the slice of the flattened
    sets that belongs to call k and group_of[k] the group of call k."""
    order: list = []  # a message (shared group), or the number of an aggregate call
    members: dict = {}
    for k, call in enumerate(calls):
        key = bytes(call[1]) if len(call) < 3 or call[2] is None else k
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(k)
    groups = []
    where: list = [None] * len(calls)
    group_of: list = [None] * len(calls)
    pos = 0
    for key in order:
        sets = []
        for k in members[key]:
            where[k] = slice(pos, pos + len(calls[k][0]))
            group_of[k] = len(groups)
            pos += len(calls[k][0])
            sets.extend(calls[k][0])
        groups.append((bytes(calls[members[key][0]][1]), sets))
    return groups, where, group_of


def merge_same_message(calls):
    """merge_same_message_groups without the group numbers: (groups, where)"""
    groups, where, _ = merge_same_message_groups(calls)
    return groups, where


def _add(metrics: dict, key: str, value) -> None:
    metrics[key] = metrics.get(key, 0) + value


def record_sm_retry(device, metrics: dict) -> None:
    """the retry of the device's last same-message call (bgv_sm_retry_stats) into sm_retry_subs / _leaves / _pairs:
    the subs a split retry formed, the sets decided by a check of their own, and the Miller pairs of the retry"""
    stats = getattr(device, "sm_retry_stats", None)
    if stats is None:
        return
    path = stats()
    for k in ("subs", "leaves", "pairs"):
        _add(metrics, "sm_retry_" + k, int(path[k]))


def _record_sm_call(device, metrics: dict, prefix: str, n_sets: int) -> None:
    """one same-message device call into <prefix>_sets_started, <prefix>_retries and the sm_retry_* counters; a
    device stand-in without last_sm_stats or sm_retry_stats reports no retry"""
    st = getattr(device, "last_sm_stats", None)
    _add(metrics, prefix + "_sets_started", n_sets)
    _add(metrics, prefix + "_retries", int(st.groups_retried) if st is not None else 0)
    record_sm_retry(device, metrics)


def _per_call(ok, where) -> list:
    ok = [bool(x) for x in ok]
    return [ok[w] for w in where]


def run_same_message_calls(device, calls, scalars_for=None, metrics: dict | None = None) -> list:
    """One device call (Device.verify_same_message) for the merged calls;
    returns list[bool] per call."""
    if any(len(c) > 2 and c[2] is not None for c in calls):
        return run_same_message_aggregate_calls(device, calls, scalars_for, metrics)
    groups, where = merge_same_message(calls)
    n = sum(len(g[1]) for g in groups)
    arrays = encode_same_message(groups, scalars_for(n) if scalars_for else None)
    ok, _codes = device.verify_same_message(arrays)
    if metrics is not None:
        _record_sm_call(device, metrics, "same_message", n)
    return _per_call(ok, where)


def check_aggregate_request(sets, agg: AggregateRequest) -> None:
    """Caller-side checks of verify_and_aggregate_same_message's own arguments"""
    if agg.previous is not None and len(agg.previous) != 96:
        raise BlsError("BLST_ERROR: BLST_INVALID_SIZE", 8)
    if agg.take is not None and len(agg.take) != len(sets):
        raise BlsError("take must have one entry per set")


def _aggregate_request(sets, message: bytes, previous, take) -> tuple:
    """What both verify_and_aggregate_same_message methods do first: (sets as a list, their AggregateRequest, the
    call's result when there is no set to verify, else None), after the caller-side checks of the request and sets."""
    sets = list(sets)
    agg = AggregateRequest(None if previous is None else bytes(previous), None if take is None else tuple(bool(t) for t in take))
    check_aggregate_request(sets, agg)
    if not sets:  # no device call: nothing is added, `previous` comes back as it is
        return sets, agg, SameMessageAggregate([], agg.previous or IDENTITY_SIG_96, 0)
    check_same_message(sets, message)
    return sets, agg, None


def run_same_message_aggregate_calls(device, calls, scalars_for=None, metrics: dict | None = None) -> list:
    """One device call (Device.verify_same_message_aggregate) for merged calls of
    which at least one asks for its aggregate.  Per call: list[bool], or for a
    call with an AggregateRequest a SameMessageAggregate, or a BlsError (returned,
    not raised: it rejects that call alone) when its `previous` did not decode."""
    groups, where, group_of = merge_same_message_groups(calls)
    n = sum(len(g[1]) for g in groups)
    arrays = encode_same_message(groups, scalars_for(n) if scalars_for else None)
    take = np.zeros(max(n, 1), dtype=np.uint8)  # plain calls: nothing to aggregate
    prev = np.tile(np.frombuffer(IDENTITY_SIG_96, dtype=np.uint8), (max(len(groups), 1), 1))
    for k, call in enumerate(calls):
        agg = call[2] if len(call) > 2 else None
        if agg is None:
            continue
        take[where[k]] = 1 if agg.take is None else np.array([1 if t else 0 for t in agg.take], dtype=np.uint8)
        if agg.previous is not None:
            prev[group_of[k]] = np.frombuffer(bytes(agg.previous), dtype=np.uint8)
    out = device.verify_same_message_aggregate(arrays, take=take, prev=prev)
    ok = [bool(x) for x in out["set_valid"]]
    res = []
    added = 0
    for k, call in enumerate(calls):
        if len(call) < 3 or call[2] is None:
            res.append(ok[where[k]])
            continue
        g = group_of[k]
        code = int(out["agg_code"][g])
        if code != 0:
            res.append(error_for_code(code))
            continue
        added += int(out["agg_count"][g])
        res.append(SameMessageAggregate(ok[where[k]], out["agg_sig"][g].tobytes(), int(out["agg_count"][g])))
    if metrics is not None:
        _record_sm_call(device, metrics, "same_message", n)
        _add(metrics, "same_message_aggregated_sigs", added)
    return res


@dataclass
class _SmJob:
    sets: list
    message: bytes
    future: asyncio.Future
    added: float
    agg: AggregateRequest | None = None  # verify_and_aggregate_same_message


class SameMessageQueue:
    """The queue of verifySignatureSetsSameMessage calls: batchable calls are
    buffered under the pool's rule (MAX_BUFFER_WAIT_MS, or more than
    MAX_BUFFERED_SIGS signatures waiting, multithread/index.ts:48-57) in a
    queue of their own; whatever is queued when the device side is free goes
    out as ONE merged device call (merge_same_message).  run_merged(calls) ->
    list[list[bool]] runs on `executor` (None: the loop's default)."""

    def __init__(self, run_merged, executor=None, max_sets: int = MAX_SETS_PER_DEVICE_BATCH):
        self._run_merged = run_merged
        self._executor = executor
        self._max_sets = max_sets
        self._jobs: list[_SmJob] = []
        self._buffered: list[_SmJob] = []
        self._buffered_sigs = 0
        self._handle = None
        self._running = False
        self._closed = False
        self.device_calls = 0

    def pending_jobs(self) -> int:
        return len(self._jobs) + len(self._buffered)

    def pending_sets(self) -> int:
        return sum(len(j.sets) for j in self._jobs + self._buffered)

    async def submit(self, sets, message: bytes, batchable: bool, agg: AggregateRequest | None = None):
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        loop = asyncio.get_running_loop()
        job = _SmJob(list(sets), bytes(message), loop.create_future(), time.monotonic(), agg)
        if batchable:
            if not self._buffered:
                self._handle = loop.call_later(MAX_BUFFER_WAIT_MS / 1000, self._flush)
            self._buffered.append(job)
            self._buffered_sigs += len(job.sets)
            if self._buffered_sigs > MAX_BUFFERED_SIGS:
                self._handle.cancel()
                self._flush()
        else:
            self._jobs.append(job)
            loop.call_soon(self._schedule)
        return await job.future

    def _flush(self):
        self._jobs.extend(self._buffered)
        self._buffered = []
        self._buffered_sigs = 0
        self._handle = None
        asyncio.get_running_loop().call_soon(self._schedule)

    def _schedule(self):
        if self._closed or self._running or not self._jobs:
            return
        take, n = [], 0
        while self._jobs and (n == 0 or n + len(self._jobs[0].sets) <= self._max_sets):
            j = self._jobs.pop(0)
            take.append(j)
            n += len(j.sets)
        self._running = True
        asyncio.ensure_future(self._run(take))

    async def _run(self, jobs: list):
        loop = asyncio.get_running_loop()
        try:
            self.device_calls += 1
            calls = [(j.sets, j.message) if j.agg is None else (j.sets, j.message, j.agg) for j in jobs]
            res = await loop.run_in_executor(self._executor, self._run_merged, calls)
            for j, r in zip(jobs, res):
                if j.future.done():
                    continue
                if isinstance(r, Exception):  # rejects this call alone (a `previous` that does not decode)
                    j.future.set_exception(r)
                else:
                    j.future.set_result(r)
        except Exception as e:  # noqa: BLE001 -- a device error rejects the merged calls
            for j in jobs:
                if not j.future.done():
                    j.future.set_exception(e)
        finally:
            self._running = False
            loop.call_soon(self._schedule)

    def abort(self):
        self._closed = True
        if self._handle is not None:
            self._handle.cancel()
            self._handle = None
        for j in self._jobs + self._buffered:
            if not j.future.done():
                j.future.set_exception(QueueError(QueueErrorCode.QUEUE_ABORTED))
        self._jobs.clear()
        self._buffered.clear()


# --------------------------------- same-message batches of aggregate sets
def _as_pubkeys(pks) -> list:
    """a set's keys: PublicKeys, or validator indices (ints, or an integer array)"""
    return [pk if isinstance(pk, PublicKey) else PublicKey(index=int(pk)) for pk in pks]


def check_aggregate_same_message(sets, message: bytes) -> None:
    """Caller-side checks of one verifyAggregateSetsSameMessage call, as
    check_sets makes them: every set is (pubkeys, signature) with at least one
    key (PublicKey.aggregate throws EMPTY_AGGREGATE_ARRAY), given as PublicKeys
    or as validator indices; a raw key is a 96-byte uncompressed point; the
    signing root is 32 bytes."""
    if len(message) != 32:
        raise BlsError("signingRoot must be 32 bytes")
    for pks, _sig in sets:
        if isinstance(pks, CommitteeKeys):
            _check_committee(pks.committee, pks.bits)
            continue
        if pks is None or len(pks) == 0:
            raise BlsError("EMPTY_AGGREGATE_ARRAY")
        for pk in pks:
            _check_key(pk if pk is None or isinstance(pk, PublicKey) else PublicKey(index=int(pk)))


def encode_same_message_agg(groups, scalars: np.ndarray | None = None) -> dict:
    """Flatten groups [(message, [(pubkeys, signature), ...]), ...] into the
    arrays of bgv_sma_batch (include/bgv.h): one message per group, a key list
    and one signature per set.  `pubkeys` holds PublicKeys or validator indices,
    as encode_jobs takes them from an aggregate set."""
    n = sum(len(g[1]) for g in groups)
    acc = _SetArrays(n, offsets=True)
    msgs = np.zeros((max(len(groups), 1), 32), dtype=np.uint8)
    off = [0]
    for g, (message, sets) in enumerate(groups):
        _group_head(msgs, g, message, sets)
        for pks, sig in sets:
            acc.keys(_as_pubkeys(pks))
            acc.signature(sig)
        off.append(acc.n)
    return {"n_sets": n, "n_groups": len(groups), "group_offsets": np.array(off, dtype=np.uint32), **acc.finish(msgs, scalars)}


def has_committee_keys(groups) -> bool:
    return any(isinstance(pks, CommitteeKeys) for _m, sets in groups for pks, _sig in sets)


def encode_same_message_bits(groups, scalars: np.ndarray | None = None) -> dict:
    """Flatten groups [(message, [(keys, signature), ...]), ...] into the arrays
    of bgv_smb_batch (include/bgv.h): `keys` is a CommitteeKeys (a list source
    over the packed bitfields) or a pubkey list as encode_same_message_agg takes
    it (a BGV_SRC_EXPLICIT run of pk_indices)."""
    n = sum(len(g[1]) for g in groups)
    acc = _SetArrays(n, sources=True)
    msgs = np.zeros((max(len(groups), 1), 32), dtype=np.uint8)
    off = [0]
    for g, (message, sets) in enumerate(groups):
        _group_head(msgs, g, message, sets)
        for pks, sig in sets:
            if isinstance(pks, CommitteeKeys):
                acc.committee(pks.committee, pks.bits)
            else:
                acc.keys(_as_pubkeys(pks))
            acc.signature(sig)
        off.append(acc.n)
    return {"n_sets": n, "n_groups": len(groups), "group_offsets": np.array(off, dtype=np.uint32), **acc.finish(msgs, scalars)}


def run_same_message_agg_calls(device, calls, scalars_for=None, metrics: dict | None = None) -> list:
    """One device call for the merged calls (merge_same_message: one group per
    call, equal messages share one); returns list[bool] per call.  The routing
    rule: a merged call that holds a committee set goes through
    Device.verify_same_message_bits (encode_same_message_bits arrays; the key
    count comes from the device's path counters); any other call takes exactly
    the path it took before (encode_same_message_agg, Device.verify_same_message_agg)."""
    groups, where = merge_same_message(calls)
    n = sum(len(g[1]) for g in groups)
    bits = has_committee_keys(groups)
    encode = encode_same_message_bits if bits else encode_same_message_agg
    arrays = encode(groups, scalars_for(n) if scalars_for else None)
    ok, _codes = (device.verify_same_message_bits if bits else device.verify_same_message_agg)(arrays)
    if metrics is not None:
        _record_sm_call(device, metrics, "same_message_agg", n)
        _add(metrics, "aggregated_pubkeys_total",
             int(device.bits_path_stats()["keys_expanded"]) if bits else int(arrays["pk_offsets"][-1]))
    return _per_call(ok, where)


# ----------------------------------------------------------------- verifier
@dataclass
class _Job:
    sets: list
    opts: VerifySignatureOpts
    future: asyncio.Future
    added: float


class BlsGpuVerifier:
    """``IBlsVerifier`` on one or more MI355X devices, one context per device
    (one host process owns them all, as the reference's pool owns its workers,
    chain/chain.ts:199-202).

    devices: HIP device ordinals; every device holds a replica of the pubkey
    table.  Every idle device takes a device batch of the queued jobs; a batch
    of >= ``shard_min_sets`` sets is split by job over all idle devices instead,
    each returning a partial Miller product (bgv_partial), combined by ONE
    final exponentiation (bgv_combine_final); when that check fails every
    shard localises its own failing jobs (bgv_partial_finish)."""

    def __init__(self, devices=(0,), metrics: dict | None = None, scalar_seed: int | None = None,
                 max_sets_per_device_batch: int = MAX_SETS_PER_DEVICE_BATCH, shard_min_sets: int = SHARD_MIN_SETS,
                 priority_cus: int | None = None, bls_verify_all_multi_thread: bool = False,
                 contexts_per_device: int = CONTEXTS_PER_DEVICE, pair_merge: bool = False, device_cfg: dict | None = None,
                 sm_retry: bool = False):
        # priority_cus CUs of the first device (a multiple of 8) are kept for
        # verifyOnMainThread (bgv_cfg.cu_split): its own context runs there,
        # the first bulk context leaves them free; 0 shares every CU.  Default:
        # PRIORITY_CUS on a pool of two or more devices (sharded batches give
        # device 0 a RESERVED_CAP-weighted shard), 0 on one device, whose bulk
        # batches would otherwise run ~13-20% slower.
        # bls_verify_all_multi_thread (chain/options.ts:14, multithread/index.ts:124):
        # verifyOnMainThread calls join the queue like any other, no CUs are
        # reserved and no priority context is opened
        devices = list(devices)
        if priority_cus is None:
            priority_cus = PRIORITY_CUS if len(devices) > 1 else 0
        if bls_verify_all_multi_thread:
            priority_cus = 0
        self.bls_verify_all_multi_thread = bls_verify_all_multi_thread
        self.priority_cus = priority_cus
        # contexts_per_device device batches in flight per GPU (one context
        # each, own table replica); every bulk context of the first device
        # leaves the reserved CUs free.  Context k runs on device entry _ctx_dev[k]
        if contexts_per_device < 1:
            raise ValueError(f"contexts_per_device {contexts_per_device}")
        self.contexts_per_device = contexts_per_device
        self.n_devices = len(devices)
        self._ctx_dev = [i for i in range(len(devices)) for _ in range(contexts_per_device)]
        # device_cfg: bgv_cfg overrides of the bulk contexts (tests and A/B tools only; production pools leave
        # every field at auto)
        bulk_cfg = dict(device_cfg or {})
        self.devices = [native.Device(devices[i], **{**bulk_cfg, "cu_split": -priority_cus}) if i == 0 and priority_cus > 0
                        else native.Device(devices[i], **bulk_cfg) for i in self._ctx_dev]
        if bls_verify_all_multi_thread:
            self.prio = None
        else:
            self.prio = native.Device(devices[0], cu_split=priority_cus) if priority_cus > 0 else native.Device(devices[0])
        self.prio_reserved = priority_cus > 0  # device 0's bulk context runs at RESERVED_CAP (shard_jobs caps)
        # pair_merge (bgv_pair_merge, off by default): every bulk context pairs once per distinct signing root of
        # a job where its batch runs the bulk layout's one-lane loop; the priority context serves latency batches
        self.pair_merge = bool(pair_merge)
        if self.pair_merge:
            for d in self.devices:
                d.pair_merge(True)
        # sm_retry (bgv_sm_retry, off by default): every context localises the failing sets of a same-message
        # call by subset checks (subs of 8, then the sets of the failing subs) instead of one-set jobs
        self.sm_retry = bool(sm_retry)
        if self.sm_retry:
            for d in self._contexts():
                d.sm_retry(1)
        if self.prio is not None:
            self._warm_priority()
        self._prio_lock = threading.Lock()
        self._shard_min = shard_min_sets
        self._idle = [True] * len(self.devices)
        self.table = PubkeyTable(self._contexts())
        self.metrics = metrics if metrics is not None else _new_metrics()
        self._rng = np.random.default_rng(scalar_seed) if scalar_seed is not None else None
        self._max_batch = max_sets_per_device_batch
        self._jobs: list[_Job] = []
        self._buffered: list[_Job] = []
        self._buffered_sigs = 0
        self._buffer_handle = None
        self._closed = False
        self._busy = 0
        self._exec = ThreadPoolExecutor(max_workers=len(self.devices) + 1)  # + the main-thread path
        self._dev_locks = [threading.Lock() for _ in self.devices]
        self._sm = SameMessageQueue(self._run_same_message, self._exec, max_sets_per_device_batch)
        self._sma = SameMessageQueue(self._run_same_message_agg, self._exec, max_sets_per_device_batch)

    def set_index_list(self, list_id: int, indices, sums: bool = False) -> None:
        """Upload a resident index list (an epoch's shuffling, a sync committee)
        to every context, like the pubkey table (bgv_index_list_set); an empty
        list drops it.  Committee sets refer to it by CommitteeRef.list_id.
        sums: also build the list's resident prefix sums (bgv_index_list_sums),
        so nearly full committees are taken as window sum minus absent members;
        every entry must then be a row the table already holds."""
        arr = np.ascontiguousarray(indices, dtype=np.uint32)
        for k, d in enumerate(self.devices):
            with self._dev_locks[k]:
                d.index_list_set(list_id, arr)
                if sums and arr.size:
                    d.index_list_sums(list_id, True)
        if self.prio is not None:
            with self._prio_lock:
                self.prio.index_list_set(list_id, arr)
                if sums and arr.size:
                    self.prio.index_list_sums(list_id, True)

    # -- IBlsVerifier ---------------------------------------------------
    def can_accept_work(self) -> bool:
        """multithread/index.ts:143-149.  A queued job joins the next device
        batch, so work is accepted while the queue holds fewer than
        MAX_JOBS_CAN_ACCEPT_WORK jobs and less than one full device batch of
        sets, whether or not a batch is in flight (a GPU wants large batches;
        gating on idle devices would stall the network processor for every
        batch, network/processor/index.ts:406)."""
        return (not self._closed
                and len(self._jobs) + self._sm.pending_jobs() + self._sma.pending_jobs() < MAX_JOBS_CAN_ACCEPT_WORK
                and sum(len(j.sets) for j in self._jobs) + self._sm.pending_sets() + self._sma.pending_sets() < self._max_batch)

    async def verify_signature_sets_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None) -> list:
        """IBlsVerifier.verifySignatureSetsSameMessage (upstream Lodestar; the
        call site is gossip attestation validation, chain/validation/
        attestation.ts:271): `sets` is a list of (PublicKey, signature) that
        all sign `message`; one boolean per set.  Batchable calls wait in a
        buffer of their own and are merged into one device call
        (bgv_verify_same_message) on one bulk context, one group per call."""
        opts = opts or VerifySignatureOpts()
        sets = list(sets)
        if not sets:
            return []
        check_same_message(sets, message)
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        return await self._sm.submit(sets, message, opts.batchable)

    async def verify_and_aggregate_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None,
                                                previous: bytes | None = None, take=None) -> SameMessageAggregate:
        """verify_signature_sets_same_message that also returns what the caller's
        pre-aggregation pool would compute next (chain/opPools/
        attestationPool.ts:182-199, syncCommitteeMessagePool.ts:139): the
        compressed sum of `previous` (the pool's running aggregate, 96 bytes) and
        the signatures of the valid sets whose `take` entry is true (None: all).
        The call rides the queue and buffer of verify_signature_sets_same_message
        and always forms its own group of the merged device call
        (bgv_verify_same_message_aggregate).  A `previous` that does not decode
        rejects this call alone with BLST_ERROR: BLST_<NAME>."""
        opts = opts or VerifySignatureOpts()
        sets, agg, nothing = _aggregate_request(sets, message, previous, take)
        if nothing is not None:
            return nothing
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        return await self._sm.submit(sets, message, opts.batchable, agg)

    async def verify_aggregate_sets_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None) -> list:
        """verifySignatureSetsSameMessage for aggregate sets: `sets` is a list of
        (pubkeys, signature) that all sign `message` (the aggregates of gossip
        beacon_aggregate_and_proof objects, chain/validation/
        aggregateAndProof.ts:164-179, or of one block's attestations for one
        committee and data); one boolean per set, False for a rejected set.
        Batchable calls wait in a buffer of their own, apart from the single-key
        one, and are merged into one device call
        (bgv_verify_same_message_agg), one group per call.  A set's `pubkeys`
        may be a CommitteeKeys (a committee of a resident index list and its
        participation bits): a merged call that holds one goes through
        bgv_verify_same_message_bits (run_same_message_agg_calls)."""
        opts = opts or VerifySignatureOpts()
        sets = list(sets)
        if not sets:
            return []
        check_aggregate_same_message(sets, message)
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        return await self._sma.submit(sets, message, opts.batchable)

    async def verify_signature_sets(self, sets: list[ISignatureSet], opts: VerifySignatureOpts | None = None) -> bool:
        opts = opts or VerifySignatureOpts()
        self.metrics["aggregated_pubkeys_total"] += get_aggregated_pubkeys_count(sets)
        # the checks the reference makes on the caller's side before queueing
        # (getAggregatedPubkey, utils.ts:5-16), so a bad call cannot fail a
        # device batch it shares with other callers
        check_sets(sets)
        if opts.verifyOnMainThread and not self.bls_verify_all_multi_thread:
            # unbuffered, high priority (multithread/index.ts:155-167): one
            # device batch on the priority context, off the event loop; it
            # never waits for the bulk contexts' locks or waves
            r = await asyncio.get_running_loop().run_in_executor(self._exec, self._run_priority, sets)
            if isinstance(r, Exception):
                raise r
            return r
        chunks = chunkify_maximize_chunk_size(sets, MAX_SIGNATURE_SETS_PER_JOB)
        results = await asyncio.gather(*[self._queue_work(c, opts) for c in chunks])
        if len(results) == 0:
            raise BlsError("Empty results array")
        return all(r is True for r in results)

    async def close(self):
        self._closed = True
        if self._buffer_handle is not None:
            self._buffer_handle.cancel()
            self._buffer_handle = None
        for j in self._jobs + self._buffered:
            if not j.future.done():
                j.future.set_exception(QueueError(QueueErrorCode.QUEUE_ABORTED))
        self._jobs.clear()
        self._buffered.clear()
        self._sm.abort()
        self._sma.abort()
        self._exec.shutdown(wait=True)
        for d in self._contexts():
            d.close()

    # -- synchronous helpers ------------------------------------------------
    def verify_signature_sets_maybe_batch(self, sets: list[ISignatureSet]) -> bool:
        """maybeBatch.ts:16-38 for one job, synchronously (BlsSingleThreadVerifier
        path, singleThread.ts:14-35)."""
        check_sets(sets)
        r = self._run_device_batch([sets], [0])[0]
        if isinstance(r, Exception):
            raise r
        return r

    def verify_signature_set(self, s: ISignatureSet) -> bool:
        """util/signatureSets.ts:24-38 verifySignatureSet: the signature is
        parsed and group-checked; single -> verify(pk, root), aggregate ->
        verifyAggregate(pks, root).  One set, one device batch (n = 1): the
        random scalar of the batch equation cannot change the verdict (GT has
        prime order r and the scalar is nonzero mod r)."""
        if s.type == SignatureSetType.aggregate and len(s.pubkeys) == 0:
            raise BlsError("EMPTY_AGGREGATE_ARRAY")
        return self.verify_signature_sets_maybe_batch([s])

    def is_valid_bls_aggregate(self, public_keys: list[PublicKey], message: bytes, signature: bytes) -> bool:
        """light-client/src/validation.ts:152-175 isValidBlsAggregate: aggregate
        the keys, deserialize + group-check the signature, verify; each failure
        re-thrown with the reference's prefix."""
        if len(public_keys) == 0:
            raise BlsError("Error aggregating pubkeys: EMPTY_AGGREGATE_ARRAY")
        s = create_aggregate_signature_set_from_components(list(public_keys), message, signature)
        try:
            return self.verify_signature_sets_maybe_batch([s])
        except BlsError as e:
            raise BlsError(f"Error deserializing signature: {e}", getattr(e, "code", None)) from e

    # -- queueing -------------------------------------------------------------
    async def _queue_work(self, sets, opts) -> bool:
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        loop = asyncio.get_running_loop()
        job = _Job(sets, opts, loop.create_future(), time.monotonic())
        if opts.batchable:
            if not self._buffered:
                self._buffer_handle = loop.call_later(MAX_BUFFER_WAIT_MS / 1000, self._run_buffered)
            self._buffered.append(job)
            self._buffered_sigs += len(sets)
            if self._buffered_sigs > MAX_BUFFERED_SIGS:
                self._buffer_handle.cancel()
                self._run_buffered()
        else:
            self._jobs.append(job)
            loop.call_soon(self._schedule)
        return await job.future

    def _run_buffered(self):
        self._jobs.extend(self._buffered)
        self._buffered = []
        self._buffered_sigs = 0
        self._buffer_handle = None
        asyncio.get_running_loop().call_soon(self._schedule)

    def _schedule(self):
        """every idle device takes a device batch of the queued jobs; a large
        batch is split over all idle devices (SHARD_MIN_SETS)"""
        while not self._closed and self._jobs and any(self._idle):
            take, n = [], 0
            while self._jobs and (n == 0 or n + len(self._jobs[0].sets) <= self._max_batch):
                j = self._jobs.pop(0)
                take.append(j)
                n += len(j.sets)
            idle = self._spread_contexts(idle_only=True)
            devs = idle if (len(idle) > 1 and len(take) > 1 and n >= self._shard_min) else [self._best_idle_context()]
            for d in devs:
                self._idle[d] = False
            self._busy += 1
            self.peak_busy = max(getattr(self, "peak_busy", 0), self._busy)  # batches in flight at once (test hook)
            asyncio.ensure_future(self._run(take, devs))

    async def _run(self, jobs: list[_Job], devs: list[int]):
        loop = asyncio.get_running_loop()
        try:
            now = time.monotonic()
            for j in jobs:
                self.metrics["job_wait_time_s"].append(now - j.added)
            results = await loop.run_in_executor(self._exec, self._run_device_batch, [j.sets for j in jobs], devs)
            for j, r in zip(jobs, results):
                if j.future.done():
                    continue
                if isinstance(r, Exception):
                    j.future.set_exception(r)
                else:
                    j.future.set_result(r)
        except Exception as e:  # device failure rejects the whole package (index.ts:386-393)
            for j in jobs:
                if not j.future.done():
                    j.future.set_exception(e)
        finally:
            self._busy -= 1
            for d in devs:
                self._idle[d] = True
            loop.call_soon(self._schedule)

    # -- device -------------------------------------------------------------
    def _scalars(self, n: int) -> np.ndarray | None:
        if self._rng is None:
            return None  # drawn inside the library (device ChaCha20 keyed by getrandom)
        s = self._rng.integers(1, 2**64 - 1, size=max(n, 1), dtype=np.uint64, endpoint=True)
        return s

    @staticmethod
    def _verdict(r: int):
        return True if r == 1 else False if r == 0 else error_for_code(-r)

    def _record(self, st: native.BgvStats, seconds: float):
        self.metrics["batch_retries"] += int(st.batch_retries)
        self.metrics["batch_sigs_success"] += int(st.batch_sigs_success)
        self.metrics["device_time_s"] += seconds

    def _record_hashes(self, hs: list[dict | None]):
        """hash_to_G2 per device batch (bgv_hash_stats of each context that ran a part of it): the sets that
        needed H(m) and the evaluations made, fewer where a bulk-layout batch repeats signing roots.  Both keys
        appear with the first batch that reports them; sharded batches add up their shards.  Beside them the set
        pairs of the Miller stage (bgv_pair_stats): the sets that needed a pair and the pairs run, fewer where a
        context with pair_merge met repeated roots inside a job."""
        for h in hs:
            if h:
                _add(self.metrics, "hash_to_g2_sets", int(h["sets"]))
                _add(self.metrics, "hash_to_g2_evaluated", int(h["hashes"]))
                pp = h.get("pair")
                if pp:
                    _add(self.metrics, "miller_pairs_sets", int(pp["sets"]))
                    _add(self.metrics, "miller_pairs_evaluated", int(pp["pairs"]))

    @staticmethod
    def _hash_stats(dev) -> dict | None:
        """read under the context's lock, right after its call (a device stand-in without the getter reports nothing)"""
        get = getattr(dev, "hash_stats", None)
        if get is None:
            return None
        out = dict(get())
        pair = getattr(dev, "pair_stats", None)
        if pair is not None:
            out["pair"] = pair()
        return out

    def _warm_priority(self):
        """sizes the priority context's work buffers for a full job (128 sets)
        at construction, so a verifyOnMainThread call never frees and regrows
        them (a hipFree synchronises the device and would wait for the bulk
        contexts' batches).  One dummy job: the G1 generator as a raw key and
        the identity signature; its verdict is ignored."""
        one = create_single_signature_set_from_components(PublicKey(raw=G1_GENERATOR_96), bytes(32), IDENTITY_SIG_96)
        self.prio.verify(encode_jobs([[one] * MAX_SIGNATURE_SETS_PER_JOB], np.ones(MAX_SIGNATURE_SETS_PER_JOB, np.uint64)),
                         want_set_codes=False)

    def _contexts(self) -> list:
        return self.devices + ([self.prio] if self.prio is not None else [])

    def _spread_contexts(self, idle_only: bool = False) -> list[int]:
        """the first (idle) context of each device: where a sharded batch goes"""
        out, seen = [], set()
        for k, dv in enumerate(self._ctx_dev):
            if dv not in seen and (not idle_only or self._idle[k]):
                seen.add(dv)
                out.append(k)
        return out

    def _best_idle_context(self) -> int:
        """an idle context on the device with the fewest batches in flight"""
        busy = [0] * self.n_devices
        for k, f in enumerate(self._idle):
            if not f:
                busy[self._ctx_dev[k]] += 1
        return min((k for k, f in enumerate(self._idle) if f), key=lambda k: (busy[self._ctx_dev[k]], k))

    def _run_priority(self, sets: list[ISignatureSet]):
        """verifyOnMainThread's device batch on the priority context"""
        t0 = time.perf_counter()
        try:
            use_bits, arrays = encode_device_batch([sets], self._scalars(len(sets)))
            with self._prio_lock:
                t1 = time.perf_counter()
                jr, _ = (self.prio.verify_bits if use_bits else self.prio.verify)(arrays, want_set_codes=False)
                self._record(self.prio.last_stats, time.perf_counter() - t1)
                self._record_hashes([self._hash_stats(self.prio)])
        except Exception as e:  # noqa: BLE001 -- a device error rejects the call
            return e
        finally:
            # mainThreadDurationInThreadPool (multithread/index.ts:156-167): timed
            # in a finally, so calls that throw are observed too
            self.metrics["main_thread_time_s"] += time.perf_counter() - t0
            self.metrics["main_thread_calls"] += 1
        return self._verdict(int(jr[0]))

    def _run_on_bulk_context(self, runner, calls) -> list:
        """runner (run_same_message_calls or run_same_message_agg_calls) for the merged calls on the first idle
        bulk context, or on the first one when none is idle (no sharding)"""
        idle = [k for k, f in enumerate(self._idle) if f]
        d = idle[0] if idle else 0
        with self._dev_locks[d]:
            t0 = time.perf_counter()
            out = runner(self.devices[d], calls, self._scalars if self._rng is not None else None, self.metrics)
            _add(self.metrics, "device_time_s", time.perf_counter() - t0)
        return out

    def _run_same_message(self, calls) -> list:
        return self._run_on_bulk_context(run_same_message_calls, calls)

    def _run_same_message_agg(self, calls) -> list:
        return self._run_on_bulk_context(run_same_message_agg_calls, calls)

    def _run_device_batch(self, jobs: list[list[ISignatureSet]], devs: list[int] | None = None) -> list:
        """Verify a list of jobs on the devices `devs` (default: all); returns
        per job True / False / BlsError.  One device: bgv_verify.  Several: the
        jobs are sharded by work, sets + pubkey references (dist.job_work,
        dist.shard_jobs), every shard reduced to
        a partial Miller product, the partials combined by one final
        exponentiation, and only when that fails each shard localised on its
        own device."""
        if not jobs:
            return []
        devs = self._spread_contexts() if devs is None else list(devs)
        if len(devs) > 1 and has_committee_sets(jobs):
            devs = devs[:1]  # bgv_partial takes no bitfields: the batch goes whole to one context
        if len(devs) > 1:
            refs = [sum(1 if s.type == SignatureSetType.single else len(s.pubkeys) for s in j) for j in jobs]
            caps = [RESERVED_CAP if self._ctx_dev[d] == 0 and self.prio_reserved else 1.0 for d in devs]
            shards = shard_jobs(job_work([len(j) for j in jobs], refs), len(devs), caps)
        else:
            shards = [list(range(len(jobs)))]
        live = [(devs[r], ids) for r, ids in enumerate(shards) if ids]
        out: list = [None] * len(jobs)
        self.metrics["sets_started"] += sum(len(j) for j in jobs)
        self.metrics["jobs_started"] += len(jobs)
        if len(live) == 1:
            d, ids = live[0]
            try:
                use_bits, arrays = encode_device_batch(jobs, self._scalars(sum(len(j) for j in jobs)))
                with self._dev_locks[d]:
                    t0 = time.perf_counter()
                    jr, _ = (self.devices[d].verify_bits if use_bits else self.devices[d].verify)(arrays, want_set_codes=False)
                    self._record(self.devices[d].last_stats, time.perf_counter() - t0)
                    self._record_hashes([self._hash_stats(self.devices[d])])
            except Exception as e:  # noqa: BLE001 -- a device error rejects the package (index.ts:386-393)
                return [e] * len(jobs)
            return [self._verdict(r) for r in jr.tolist()]
        # every participating context stays locked from its partial to its
        # localisation (the partial's intermediates live on the context)
        locks = [self._dev_locks[d] for d, _ in sorted(live)]
        for lk in locks:
            lk.acquire()
        try:
            t0 = time.perf_counter()
            parts: list = [None] * len(live)
            hashed: list = [None] * len(live)

            def run_partial(k):
                d, ids = live[k]
                try:
                    sub = [jobs[i] for i in ids]
                    parts[k] = self.devices[d].partial(encode_jobs(sub, self._scalars(sum(len(j) for j in sub))))
                    hashed[k] = self._hash_stats(self.devices[d])
                except Exception as e:  # noqa: BLE001
                    parts[k] = e

            self._parallel(run_partial, len(live))
            self._record_hashes(hashed)
            failed = [k for k in range(len(live)) if isinstance(parts[k], Exception)]
            for k in failed:  # a device error rejects that shard's jobs
                for i in live[k][1]:
                    out[i] = parts[k]
            ok_shards = [k for k in range(len(live)) if k not in failed]
            if not ok_shards:
                return out
            d0 = live[ok_shards[0]][0]
            valid = self.devices[d0].combine_final([parts[k][0] for k in ok_shards])
            finals: list = [None] * len(live)
            if valid:
                for k in ok_shards:
                    finals[k] = parts[k][2]  # provisional: 1, or -code for a rejected job (final)
            else:
                def run_finish(k):
                    try:
                        finals[k] = self.devices[live[k][0]].partial_finish()
                    except Exception as e:  # noqa: BLE001
                        finals[k] = e

                self._parallel(run_finish, len(live), only=ok_shards)
            valid_sets = 0
            for k in ok_shards:
                ids = live[k][1]
                if isinstance(finals[k], Exception):
                    for i in ids:
                        out[i] = finals[k]
                    continue
                for i, r in zip(ids, np.asarray(finals[k]).tolist()):
                    out[i] = self._verdict(int(r))
                    if valid and r == 1:
                        valid_sets += len(jobs[i])
            self.metrics["batch_retries"] += 0 if valid else 1
            self.metrics["batch_sigs_success"] += valid_sets
            self.metrics["device_time_s"] += time.perf_counter() - t0
        finally:
            for lk in locks:
                lk.release()
        return out

    @staticmethod
    def _parallel(fn, n: int, only=None):
        ks = list(range(n)) if only is None else list(only)
        if len(ks) == 1:
            fn(ks[0])
            return
        ths = [threading.Thread(target=fn, args=(k,)) for k in ks]
        for t in ths:
            t.start()
        for t in ths:
            t.join()


class BlsGpuSingleThreadVerifier:
    """BlsSingleThreadVerifier (chain/bls/singleThread.ts:7-46), which
    chain.ts:200-202 builds instead of the pool when blsVerifyAllMainThread is
    set: maybeBatch on one device context in the calling thread (the event loop
    waits, as it does for blst on the main thread); can_accept_work() is always
    True.  Its pubkey table is its own replica."""

    def __init__(self, device: int = 0, metrics: dict | None = None, pair_merge: bool = False, sm_retry: bool = False):
        self.device = native.Device(device)
        if sm_retry:  # bgv_sm_retry: the split retry of the same-message entries
            self.device.sm_retry(1)
        if pair_merge:  # bgv_pair_merge: one pair per distinct root of a job in bulk-layout batches
            self.device.pair_merge(True)
        self.table = PubkeyTable([self.device])
        self.metrics = metrics if metrics is not None else {"aggregated_pubkeys_total": 0, "main_thread_time_s": 0.0,
                                                            "main_thread_calls": 0}
        self._closed = False

    async def verify_signature_sets(self, sets: list[ISignatureSet], opts: VerifySignatureOpts | None = None) -> bool:
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        self.metrics["aggregated_pubkeys_total"] += get_aggregated_pubkeys_count(sets)
        check_sets(sets)  # getAggregatedPubkey's checks (utils.ts:5-16)
        t0 = time.perf_counter()
        jr = verify_device_batch(self.device, [sets])
        r = BlsGpuVerifier._verdict(int(jr[0]))
        if isinstance(r, Exception):
            raise r  # only runs without exceptions are timed, as in the reference
        self.metrics["main_thread_time_s"] += time.perf_counter() - t0
        self.metrics["main_thread_calls"] += 1
        return r

    async def verify_signature_sets_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None) -> list:
        """verifySignatureSetsSameMessage in the calling thread: one device call, one group"""
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        sets = list(sets)
        if not sets:
            return []
        check_same_message(sets, message)
        return run_same_message_calls(self.device, [(sets, message)], None, self.metrics)[0]

    async def verify_and_aggregate_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None,
                                                previous: bytes | None = None, take=None) -> SameMessageAggregate:
        """verify_and_aggregate_same_message in the calling thread: one device call, one group"""
        sets, agg, nothing = _aggregate_request(sets, message, previous, take)
        if nothing is not None:
            return nothing
        r = run_same_message_calls(self.device, [(sets, message, agg)], None, self.metrics)[0]
        if isinstance(r, Exception):
            raise r
        return r

    async def verify_aggregate_sets_same_message(self, sets, message: bytes, opts: VerifySignatureOpts | None = None) -> list:
        """verify_aggregate_sets_same_message in the calling thread: one device call, one group"""
        if self._closed:
            raise QueueError(QueueErrorCode.QUEUE_ABORTED)
        sets = list(sets)
        if not sets:
            return []
        check_aggregate_same_message(sets, message)
        return run_same_message_agg_calls(self.device, [(sets, message)], None, self.metrics)[0]

    def set_index_list(self, list_id: int, indices, sums: bool = False) -> None:
        """bgv_index_list_set (and, with sums, bgv_index_list_sums) on this
        verifier's context (see BlsGpuVerifier.set_index_list)"""
        arr = np.ascontiguousarray(indices, dtype=np.uint32)
        self.device.index_list_set(list_id, arr)
        if sums and arr.size:
            self.device.index_list_sums(list_id, True)

    def can_accept_work(self) -> bool:
        return True

    async def close(self):
        if not self._closed:
            self._closed = True
            self.device.close()


async def reject_first_invalid_resolve_all_valid(is_valid_awaitables) -> dict:
    """chain/blocks/verifyBlocksSignatures.ts:69-89: resolves {"allValid": False,
    "index": i} at the first False to arrive, {"allValid": True} when all are
    True; an exception rejects."""
    tasks = [asyncio.ensure_future(a) for a in is_valid_awaitables]
    idx = {t: i for i, t in enumerate(tasks)}
    pending = set(tasks)
    try:
        while pending:
            done, pending = await asyncio.wait(pending, return_when=asyncio.FIRST_COMPLETED)
            for t in sorted(done, key=lambda t: idx[t]):
                if not t.result():
                    return {"allValid": False, "index": idx[t]}
        return {"allValid": True}
    finally:
        for t in pending:
            t.cancel()


async def verify_blocks_signatures(bls: "BlsGpuVerifier", blocks_sets: list[list[ISignatureSet]],
                                   coalesce: bool = True) -> dict:
    """verifyBlocksSignatures (chain/blocks/verifyBlocksSignatures.ts:16-60) for
    a segment of blocks.  coalesce=False issues one verifySignatureSets per
    block exactly like the reference; coalesce=True sends
    the whole segment as ONE device batch with one job per block (each block
    <= 128 sets is exactly one reference job), so the per-block verdicts come
    from a single whole-segment pairing check plus per-block checks only on
    failure.  Verdict semantics are the same; with every block result
    arriving at once, the first invalid block by index is reported."""
    if not coalesce:
        return await reject_first_invalid_resolve_all_valid([bls.verify_signature_sets(s) for s in blocks_sets])
    jobs = []
    owner = []
    for b, sets in enumerate(blocks_sets):
        check_sets(sets)
        for chunk in chunkify_maximize_chunk_size(sets, MAX_SIGNATURE_SETS_PER_JOB):
            jobs.append(chunk)
            owner.append(b)
    res = await asyncio.get_running_loop().run_in_executor(bls._exec, bls._run_device_batch, jobs, None)
    ok = [True] * len(blocks_sets)
    for b, r in zip(owner, res):
        if isinstance(r, Exception):
            raise r
        ok[b] = ok[b] and r
    for b, v in enumerate(ok):
        if not v:
            return {"allValid": False, "index": b}
    return {"allValid": True}


def _new_metrics() -> dict:
    """Counterparts of lodestar_bls_thread_pool_* (metrics/metrics/lodestar.ts:350-430)."""
    return {
        "aggregated_pubkeys_total": 0,
        "jobs_started": 0,
        "main_thread_time_s": 0.0,
        "main_thread_calls": 0,
        "sets_started": 0,
        "batch_retries": 0,
        "batch_sigs_success": 0,
        "device_time_s": 0.0,
        "job_wait_time_s": [],
        "same_message_sets_started": 0,
        "same_message_retries": 0,
        "same_message_aggregated_sigs": 0,
        "same_message_agg_sets_started": 0,
        "same_message_agg_retries": 0,
        "sm_retry_subs": 0,
        "sm_retry_leaves": 0,
        "sm_retry_pairs": 0,
    }
