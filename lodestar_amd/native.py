"""ctypes binding of the C ABI in include/bgv.h (lodestar_amd/libbgv.so).

This is the Python counterpart of the N-API addon described in
INTEGRATION.md: plain pointers and sizes cross the boundary, nothing else.
There is no CPU fallback: if the gfx950 library is missing or no HIP device
is visible, every entry point raises ``BgvNativeError``.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BGV_LIB", os.path.join(HERE, "libbgv.so"))

# include/bgv.h enums
BGV_OK = 0
BGV_E_INVALID_ARG = -1
BGV_E_HIP = -2
BGV_E_NO_DEVICE = -3
BGV_E_TABLE_RANGE = -4
BGV_E_EMPTY_SET = -5
BGV_E_BAD_PUBKEY = -6
BGV_E_STATE = -7
ABI_VERSION = 4

SET_CODE_NAMES = {
    0: "BLST_SUCCESS",
    1: "BLST_BAD_ENCODING",
    2: "BLST_POINT_NOT_ON_CURVE",
    3: "BLST_POINT_NOT_IN_GROUP",
    4: "BLST_AGGR_TYPE_MISMATCH",
    5: "BLST_VERIFY_FAIL",
    6: "BLST_PK_IS_INFINITY",
    7: "BLST_BAD_SCALAR",
    8: "BLST_INVALID_SIZE",
    9: "BGV_INDEX_RANGE",
    10: "EMPTY_SIGNATURE_SET",
}

PK_COMPRESSED_48 = 0
PK_UNCOMPRESSED_96 = 1
N_STAGES = 16

EXPORTS = [
    "bgv_abi_version", "bgv_build_id", "bgv_set_code_name", "bgv_stage_name", "bgv_last_error", "bgv_open", "bgv_open_cfg",
    "bgv_cfg_default", "bgv_close",
    "bgv_pubkeys_set", "bgv_pubkeys_count", "bgv_pubkeys_get", "bgv_pubkeys_validate", "bgv_verify", "bgv_last_stats",
    "bgv_partial", "bgv_partial_finish", "bgv_combine_final", "bgv_debug_stages", "bgv_gen_keys", "bgv_gen_sign", "bgv_bench_fpmul",
    "bgv_bench_mad", "bgv_debug_fp_ops", "bgv_debug_g2_decode",
    "bgv_verify_same_message", "bgv_sm_check", "bgv_debug_same_message",
    "bgv_verify_same_message_agg", "bgv_sma_check", "bgv_debug_same_message_agg",
    "bgv_index_list_set", "bgv_index_list_len", "bgv_verify_bits", "bgv_bits_check", "bgv_debug_bits_expand",
    "bgv_bits_expand_ms",
    "bgv_index_list_sums", "bgv_index_list_has_sums", "bgv_bits_path_stats", "bgv_bits_plan", "bgv_debug_bits_keys",
    "bgv_debug_index_list_sums", "bgv_index_list_sums_ms",
    "bgv_verify_same_message_bits", "bgv_smb_check", "bgv_debug_same_message_bits",
    "bgv_hash_stats", "bgv_miller_path_stats",
    "bgv_verify_same_message_aggregate", "bgv_sm_agg_check", "bgv_sm_agg_ms",
    "bgv_pair_merge", "bgv_pair_stats", "bgv_debug_pair_classes",
    "bgv_batch_tail", "bgv_tail_stats",
    "bgv_sm_retry", "bgv_sm_retry_stats",
]
# exported too, listed apart: the one entry that returns a count (uint32_t), not a status
EXPORTS_U32 = ["bgv_sm_split_plan"]
MAX_INDEX_LISTS = 8
SRC_EXPLICIT = 0xFFFFFFFF
# bgv_set_src as a numpy record: (list, off, len, bits_off), 16 B per set
SET_SRC_DTYPE = np.dtype([("list", "<u4"), ("off", "<u4"), ("len", "<u4"), ("bits_off", "<u4")])
FP_OPS_N = 13


class BgvNativeError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"bgv status {status}: {msg}")
        self.status = status


class BgvBatch(ctypes.Structure):
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_jobs", ctypes.c_uint32),
        ("job_offsets", ctypes.c_void_p),
        ("pk_offsets", ctypes.c_void_p),
        ("pk_indices", ctypes.c_void_p),
        ("raw_pks", ctypes.c_void_p),
        ("n_raw", ctypes.c_uint32),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("scalars", ctypes.c_void_p),
        ("on_device", ctypes.c_uint32),
    ]


class BgvStats(ctypes.Structure):
    _fields_ = [
        ("stage_ms", ctypes.c_float * N_STAGES),
        ("total_ms", ctypes.c_float),
        ("batch_retries", ctypes.c_uint32),
        ("batch_sigs_success", ctypes.c_uint32),
        ("n_sets", ctypes.c_uint32),
        ("n_jobs", ctypes.c_uint32),
        ("pubkeys_aggregated", ctypes.c_uint64),
        ("split", ctypes.c_uint32),
        ("miller_lanes", ctypes.c_uint32),
        ("pairs_per_item", ctypes.c_uint32),
        ("msm", ctypes.c_uint32),
        ("lines", ctypes.c_uint32),
        ("defer_from", ctypes.c_uint32),
        ("clear_lanes", ctypes.c_uint32),
        ("miller_kv", ctypes.c_uint32),
    ]
    LAYOUT = ("split", "miller_lanes", "pairs_per_item", "msm", "lines", "defer_from", "clear_lanes", "miller_kv")

    def as_dict(self, lib=None):
        names = [lib.stage_name(i) for i in range(N_STAGES)] if lib else [str(i) for i in range(N_STAGES)]
        return {
            "stage_ms": dict(zip(names, [float(x) for x in self.stage_ms])),
            "total_ms": float(self.total_ms),
            "batch_retries": int(self.batch_retries),
            "batch_sigs_success": int(self.batch_sigs_success),
            "n_sets": int(self.n_sets),
            "n_jobs": int(self.n_jobs),
            "pubkeys_aggregated": int(self.pubkeys_aggregated),
            "layout": self.layout(),
        }

    def layout(self) -> dict:
        """the pipeline variant the last batch ran with (prepare() in bgv_api.hip)"""
        return {k: int(getattr(self, k)) for k in self.LAYOUT}


class BgvSmBatch(ctypes.Structure):
    """bgv_sm_batch (include/bgv.h): single-pubkey sets grouped by message."""
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_groups", ctypes.c_uint32),
        ("group_offsets", ctypes.c_void_p),
        ("pk_indices", ctypes.c_void_p),
        ("raw_pks", ctypes.c_void_p),
        ("n_raw", ctypes.c_uint32),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("scalars", ctypes.c_void_p),
        ("on_device", ctypes.c_uint32),
    ]


class BgvSmAgg(ctypes.Structure):
    """bgv_sm_agg (include/bgv.h): what bgv_verify_same_message_aggregate takes
    and returns beside the batch."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("take", "prev_sig96", "agg_sig96", "agg_count", "agg_code")]


class BgvSmaBatch(ctypes.Structure):
    """bgv_sma_batch (include/bgv.h): aggregate sets grouped by message."""
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_groups", ctypes.c_uint32),
        ("group_offsets", ctypes.c_void_p),
        ("pk_offsets", ctypes.c_void_p),
        ("pk_indices", ctypes.c_void_p),
        ("raw_pks", ctypes.c_void_p),
        ("n_raw", ctypes.c_uint32),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("scalars", ctypes.c_void_p),
        ("on_device", ctypes.c_uint32),
    ]


class BgvBitsBatch(ctypes.Structure):
    """bgv_bits_batch (include/bgv.h): sets given as committee bitfields over
    resident index lists, or as explicit index runs."""
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_jobs", ctypes.c_uint32),
        ("job_offsets", ctypes.c_void_p),
        ("src", ctypes.c_void_p),
        ("bits", ctypes.c_void_p),
        ("bits_len", ctypes.c_uint32),
        ("pk_indices", ctypes.c_void_p),
        ("n_indices", ctypes.c_uint32),
        ("raw_pks", ctypes.c_void_p),
        ("n_raw", ctypes.c_uint32),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("scalars", ctypes.c_void_p),
        ("on_device", ctypes.c_uint32),
    ]


class BgvSmbBatch(ctypes.Structure):
    """bgv_smb_batch (include/bgv.h): sets grouped by message, their keys given
    as committee bitfields over resident index lists or as explicit index runs."""
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_groups", ctypes.c_uint32),
        ("group_offsets", ctypes.c_void_p),
        ("src", ctypes.c_void_p),
        ("bits", ctypes.c_void_p),
        ("bits_len", ctypes.c_uint32),
        ("pk_indices", ctypes.c_void_p),
        ("n_indices", ctypes.c_uint32),
        ("raw_pks", ctypes.c_void_p),
        ("n_raw", ctypes.c_uint32),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("scalars", ctypes.c_void_p),
        ("on_device", ctypes.c_uint32),
    ]


class _Counters(ctypes.Structure):
    """base of the structs of plain counters the library fills: uint32 fields (and bgv_sm_stats' float total_ms)"""

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}  # ctypes hands back int for uint32, float for float


class BgvSmStats(_Counters):
    """bgv_sm_stats (include/bgv.h): counters that show which path ran."""
    _fields_ = [(k, ctypes.c_uint32) for k in
                ("n_sets", "n_groups", "n_segments", "hashes", "pairs", "groups_retried", "sets_retried")] + [
        ("total_ms", ctypes.c_float)]


class BgvCfg(ctypes.Structure):
    """bgv_cfg (include/bgv.h): pipeline overrides for tests and A/B tools.
    Production contexts use the defaults (every field "auto")."""
    _fields_ = [("struct_size", ctypes.c_uint32)] + [
        (k, ctypes.c_int32) for k in
        ("split", "miller", "job_lanes", "msm", "pairs", "prefold", "lines", "defer_pct", "timing", "clear_lanes",
         "miller_kv", "cu_split", "miller_steps", "hash_dedup")]
    AUTO = {"split": -1, "miller": -1, "job_lanes": 0, "msm": -1, "pairs": 0, "prefold": -1, "lines": -1,
            "defer_pct": -1, "timing": -1, "clear_lanes": -1, "miller_kv": -1, "cu_split": 0, "miller_steps": -1,
            "hash_dedup": -1}

    @classmethod
    def make(cls, **over) -> "BgvCfg":
        bad = set(over) - set(cls.AUTO)
        if bad:
            raise ValueError(f"unknown bgv_cfg fields {sorted(bad)}")
        c = cls(struct_size=ctypes.sizeof(cls), **{**cls.AUTO, **over})
        return c


class BgvDebug(ctypes.Structure):
    """bgv_debug (include/bgv.h): host buffers for bgv_debug_stages."""
    _fields_ = [(k, ctypes.c_void_p) for k in
                ("sig_aff", "h_aff", "pk_agg", "rpk_aff", "s_aff", "pair_fe", "job_fe", "batch_fe")]


_lib = None
_lib_lock = threading.Lock()

ROOT = os.path.dirname(HERE)


def source_files(root: str = ROOT) -> list[str]:
    """The sources libbgv.so is compiled from, relative to the repo root."""
    csrc = os.path.join(root, "lodestar_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".h", ".hip")))
    return [os.path.join("lodestar_amd", "csrc", f) for f in names] + [os.path.join("include", "bgv.h")]


class BgvBitsPath(_Counters):
    """bgv_bits_path (include/bgv.h): path counters of the last bgv_verify_bits"""
    _fields_ = [("sets_complement", ctypes.c_uint32), ("keys_expanded", ctypes.c_uint32), ("keys_gathered", ctypes.c_uint32)]


class BgvHashPath(_Counters):
    """bgv_hash_path (include/bgv.h): hash_to_G2 evaluations of the last ordinary batch"""
    _fields_ = [("sets", ctypes.c_uint32), ("hashes", ctypes.c_uint32), ("dedup", ctypes.c_uint32)]


class BgvMillerPath(_Counters):
    """bgv_miller_path (include/bgv.h): how the Miller stage of the last batch ran"""
    _fields_ = [("steps", ctypes.c_uint32), ("slice_sets", ctypes.c_uint32), ("items", ctypes.c_uint32)]


class BgvTailPath(_Counters):
    """bgv_tail_path (include/bgv.h): the tail the last ordinary batch ran"""
    _fields_ = [("batch_first", ctypes.c_uint32), ("retried", ctypes.c_uint32)]


class BgvPairPath(_Counters):
    """bgv_pair_path (include/bgv.h): the set pairs the Miller stage of the last ordinary batch ran"""
    _fields_ = [("sets", ctypes.c_uint32), ("pairs", ctypes.c_uint32), ("merged", ctypes.c_uint32),
                ("fallback", ctypes.c_uint32)]


class BgvSmRetryPath(_Counters):
    """bgv_sm_retry_path (include/bgv.h): the retry the last same-message call ran"""
    _fields_ = [("mode", ctypes.c_uint32), ("segments", ctypes.c_uint32), ("subs", ctypes.c_uint32),
                ("subs_failed", ctypes.c_uint32), ("leaves", ctypes.c_uint32), ("pairs", ctypes.c_uint32),
                ("hashes", ctypes.c_uint32)]


SM_SUB = 8  # BGV_SM_SUB
SM_PLAN_FAIL = 0xFFFFFFFF


def source_hash(root: str = ROOT) -> str:
    """SHA-256 over (path, content) of source_files(): the id tools/build.py
    compiles into the library (bgv_build_id) and load_library checks."""
    import hashlib

    h = hashlib.sha256()
    for rel in source_files(root):
        with open(os.path.join(root, rel), "rb") as f:
            data = f.read()
        h.update(rel.replace(os.sep, "/").encode() + b"\0" + len(data).to_bytes(8, "little") + data)
    return h.hexdigest()


def check_build_id(lib_id: str, root: str = ROOT) -> None:
    """A library compiled from other sources than the tree beside it is
    refused (variant builds carry the id plus '+' and their defines).  An
    install that ships the library without its csrc tree has nothing to
    compare against: the check is skipped with a warning."""
    try:
        want = source_hash(root)
    except OSError as e:
        import warnings
        warnings.warn(f"libbgv.so build id not checked: sources not readable ({e})", RuntimeWarning, stacklevel=2)
        return
    if lib_id != want and not lib_id.startswith(want + "+"):
        raise BgvNativeError(BGV_E_INVALID_ARG,
                             f"libbgv.so was built from other sources (id {lib_id[:16]}, tree {want[:16]}): "
                             "rebuild with __graft_entry__.build()")


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libbgv.so (no compute). Raises BgvNativeError when absent or when
    it was not compiled from the sources in this tree."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise BgvNativeError(BGV_E_NO_DEVICE, f"{path} not built (run __graft_entry__.build())")
        # One HIP runtime per process: torch ships its own libamdhip64 with the
        # same soname as /opt/rocm's.  Loaded first, torch's copy satisfies
        # libbgv's dependency; loaded after libbgv, torch brings a second
        # runtime that cannot open the GPU ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            lib = ctypes.CDLL(path)
            build_id_fn = lib.bgv_build_id
        except (OSError, AttributeError) as e:
            raise BgvNativeError(BGV_E_INVALID_ARG, f"{path}: not a loadable libbgv.so of this ABI ({e}): rebuild") from e
        build_id_fn.argtypes = []
        build_id_fn.restype = ctypes.c_char_p
        check_build_id(build_id_fn().decode())
        P = ctypes.c_void_p
        u32, i32, u64 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
        sig = {
            "bgv_abi_version": ([], ctypes.c_int),
            "bgv_set_code_name": ([ctypes.c_int], ctypes.c_char_p),
            "bgv_stage_name": ([ctypes.c_int], ctypes.c_char_p),
            "bgv_last_error": ([], ctypes.c_char_p),
            "bgv_open": ([ctypes.c_int, ctypes.POINTER(P)], ctypes.c_int),
            "bgv_open_cfg": ([ctypes.c_int, ctypes.POINTER(BgvCfg), ctypes.POINTER(P)], ctypes.c_int),
            "bgv_cfg_default": ([ctypes.POINTER(BgvCfg)], None),
            "bgv_close": ([P], ctypes.c_int),
            "bgv_pubkeys_set": ([P, u32, u32, P, u32], ctypes.c_int),
            "bgv_pubkeys_count": ([P, ctypes.POINTER(u32)], ctypes.c_int),
            "bgv_pubkeys_get": ([P, u32, u32, P], ctypes.c_int),
            "bgv_pubkeys_validate": ([P, P, u32, P], ctypes.c_int),
            "bgv_verify": ([P, ctypes.POINTER(BgvBatch), P, P, ctypes.POINTER(BgvStats)], ctypes.c_int),
            "bgv_partial": ([P, ctypes.POINTER(BgvBatch), P, P, P, ctypes.POINTER(i32)], ctypes.c_int),
            "bgv_partial_finish": ([P, P, ctypes.POINTER(BgvStats)], ctypes.c_int),
            "bgv_last_stats": ([P, ctypes.POINTER(BgvStats)], ctypes.c_int),
            "bgv_debug_stages": ([P, ctypes.POINTER(BgvBatch), P, P, ctypes.POINTER(BgvDebug)], ctypes.c_int),
            "bgv_combine_final": ([P, P, u32, ctypes.POINTER(i32)], ctypes.c_int),
            "bgv_gen_keys": ([P, u32, u32, u64], ctypes.c_int),
            "bgv_gen_sign": ([P, ctypes.POINTER(BgvBatch), P], ctypes.c_int),
            "bgv_bench_fpmul": ([P, u32, u32, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
            "bgv_bench_mad": ([P, u32, u32, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
            "bgv_debug_fp_ops": ([P, P, u32, P], ctypes.c_int),
            "bgv_debug_g2_decode": ([P, P, P, u32, P, P], ctypes.c_int),
            "bgv_verify_same_message": ([P, ctypes.POINTER(BgvSmBatch), P, P, ctypes.POINTER(BgvSmStats)], ctypes.c_int),
            "bgv_sm_check": ([ctypes.POINTER(BgvSmBatch)], ctypes.c_int),
            "bgv_debug_same_message": ([P, ctypes.POINTER(BgvSmBatch), P, P, ctypes.POINTER(BgvSmStats), P, P, P], ctypes.c_int),
            "bgv_verify_same_message_agg": ([P, ctypes.POINTER(BgvSmaBatch), P, P, ctypes.POINTER(BgvSmStats)], ctypes.c_int),
            "bgv_sma_check": ([ctypes.POINTER(BgvSmaBatch)], ctypes.c_int),
            "bgv_debug_same_message_agg": ([P, ctypes.POINTER(BgvSmaBatch), P, P, ctypes.POINTER(BgvSmStats), P, P, P, P],
                                           ctypes.c_int),
            "bgv_index_list_set": ([P, u32, P, u32], ctypes.c_int),
            "bgv_index_list_len": ([P, u32, ctypes.POINTER(u32)], ctypes.c_int),
            "bgv_verify_bits": ([P, ctypes.POINTER(BgvBitsBatch), P, P, ctypes.POINTER(BgvStats)], ctypes.c_int),
            "bgv_bits_check": ([ctypes.POINTER(BgvBitsBatch), P], ctypes.c_int),
            "bgv_debug_bits_expand": ([P, ctypes.POINTER(BgvBitsBatch), P, P, u32, ctypes.POINTER(u32)], ctypes.c_int),
            "bgv_bits_expand_ms": ([P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
            "bgv_index_list_sums": ([P, u32, u32], ctypes.c_int),
            "bgv_index_list_has_sums": ([P, u32, ctypes.POINTER(u32)], ctypes.c_int),
            "bgv_index_list_sums_ms": ([P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
            "bgv_bits_path_stats": ([P, ctypes.POINTER(BgvBitsPath)], ctypes.c_int),
            "bgv_hash_stats": ([P, ctypes.POINTER(BgvHashPath)], ctypes.c_int),
            "bgv_miller_path_stats": ([P, ctypes.POINTER(BgvMillerPath)], ctypes.c_int),
            "bgv_pair_merge": ([P, ctypes.c_int32], ctypes.c_int),
            "bgv_pair_stats": ([P, ctypes.POINTER(BgvPairPath)], ctypes.c_int),
            "bgv_sm_retry": ([P, ctypes.c_int32], ctypes.c_int),
            "bgv_sm_retry_stats": ([P, ctypes.POINTER(BgvSmRetryPath)], ctypes.c_int),
            "bgv_sm_split_plan": ([ctypes.c_uint32, P, ctypes.c_uint32], ctypes.c_uint32),
            "bgv_batch_tail": ([P, ctypes.c_int32], ctypes.c_int),
            "bgv_tail_stats": ([P, ctypes.POINTER(BgvTailPath)], ctypes.c_int),
            "bgv_debug_pair_classes": ([P, ctypes.POINTER(BgvBatch), P, P, P, P, P, P, P], ctypes.c_int),
            "bgv_bits_plan": ([ctypes.POINTER(BgvBitsBatch), P, P, P, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
            "bgv_debug_bits_keys": ([P, ctypes.POINTER(BgvBitsBatch), P, P, P], ctypes.c_int),
            "bgv_debug_index_list_sums": ([P, u32, u32, u32, P], ctypes.c_int),
            "bgv_verify_same_message_bits": ([P, ctypes.POINTER(BgvSmbBatch), P, P, ctypes.POINTER(BgvSmStats)], ctypes.c_int),
            "bgv_smb_check": ([ctypes.POINTER(BgvSmbBatch), P], ctypes.c_int),
            "bgv_debug_same_message_bits": ([P, ctypes.POINTER(BgvSmbBatch), P, P, ctypes.POINTER(BgvSmStats), P, P, P, P, P],
                                            ctypes.c_int),
            "bgv_verify_same_message_aggregate": ([P, ctypes.POINTER(BgvSmBatch), ctypes.POINTER(BgvSmAgg), P, P,
                                                   ctypes.POINTER(BgvSmStats)], ctypes.c_int),
            "bgv_sm_agg_check": ([ctypes.POINTER(BgvSmBatch), ctypes.POINTER(BgvSmAgg)], ctypes.c_int),
            "bgv_sm_agg_ms": ([P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = res
        if lib.bgv_abi_version() != ABI_VERSION:
            raise BgvNativeError(BGV_E_INVALID_ARG, f"{path}: ABI {lib.bgv_abi_version()}, expected {ABI_VERSION} (rebuild)")
        _lib = lib
        return lib


def _ptr(a) -> int | None:
    """address of a numpy array / torch tensor / None"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())  # torch tensor (device-resident)


def _sync_producers(*objs) -> None:
    """Device-resident inputs must be complete before the library reads them
    (include/bgv.h, bgv_batch.on_device): the library runs on its own streams,
    which do not wait for the stream that produced a torch tensor.  Wait for
    the current torch stream of every device a tensor argument lives on (a
    tensor filled by torch.full / torch.zeros / a copy is otherwise still being
    written when the library's kernels read it, or -- for an output buffer --
    overwrites what they wrote)."""
    seen = set()
    for o in objs:
        vals = o.values() if isinstance(o, dict) else (o,)
        for a in vals:
            if a is None or isinstance(a, (np.ndarray, bytes, bytearray, int, float, str)):
                continue
            dev = getattr(a, "device", None)
            if dev is None or getattr(dev, "type", "") != "cuda":
                continue
            key = getattr(dev, "index", None)
            if key in seen:
                continue
            seen.add(key)
            import torch
            torch.cuda.current_stream(dev).synchronize()


# the compressed identity of G2: "no running aggregate" as prev, and the aggregate of no set
G2_IDENTITY_96 = bytes([0xC0]) + bytes(95)


def sm_agg_check(arrays: dict, take=None, prev=None, on_device: bool = False, agg_sig=True) -> tuple[int, str]:
    """bgv_sm_agg_check: the host-side contract of bgv_verify_same_message_aggregate,
    without a device.  agg_sig=False passes a NULL output.  (status, bgv_last_error()
    text); the text is empty for BGV_OK."""
    lib = load_library()
    b = Device.make_sm_batch(arrays, on_device, sync_inputs=False)
    out = np.zeros((max(b.n_groups, 1), 96), np.uint8)
    a = BgvSmAgg(take=_ptr(take), prev_sig96=_ptr(prev), agg_sig96=out.ctypes.data if agg_sig else None)
    st = lib.bgv_sm_agg_check(ctypes.byref(b), ctypes.byref(a))
    return st, ("" if st == BGV_OK else lib.bgv_last_error().decode())


def sma_check(arrays: dict, on_device: bool = False) -> tuple[int, str]:
    """bgv_sma_check: the host-side contract of bgv_verify_same_message_agg, without
    a device.  (status, bgv_last_error() text); the text is empty for BGV_OK."""
    lib = load_library()
    b = Device.make_sma_batch(arrays, on_device, sync_inputs=False)
    st = lib.bgv_sma_check(ctypes.byref(b))
    return st, ("" if st == BGV_OK else lib.bgv_last_error().decode())


def _count(a, width: int = 1) -> int:
    """entries of a numpy array / torch tensor / None (bytes / width for u8 views)"""
    if a is None:
        return 0
    n = a.size if isinstance(a, np.ndarray) else a.numel()
    return int(n) // width


# The keys of `arrays` each batch struct cannot do without: a missing one raises KeyError.  Every other pointer
# is NULL and every other count 0 when its key is absent, and the two derived counts default to their array's size.
_REQUIRED = {
    BgvBatch: ("n_sets", "n_jobs", "job_offsets", "pk_offsets", "pk_indices", "msgs"),
    BgvSmBatch: ("n_sets", "n_groups", "group_offsets", "pk_indices", "msgs", "sigs", "sig_len"),
    BgvSmaBatch: ("n_sets", "n_groups", "group_offsets", "pk_offsets", "pk_indices", "msgs", "sigs", "sig_len"),
    BgvBitsBatch: ("n_sets", "n_jobs", "job_offsets", "src"),
    BgvSmbBatch: ("n_sets", "n_groups", "group_offsets", "src"),
}
_DERIVED_COUNT = {"bits_len": "bits", "n_indices": "pk_indices"}


def _fill(struct_cls, arrays: dict, on_device: bool, sync_inputs: bool):
    """A batch struct of include/bgv.h from `arrays` (what the verifier.encode_* function of the same family
    returns, as numpy arrays or, for an on_device batch, torch tensors), field by field in the struct's own order:
    a pointer field takes its entry's address, a uint32 field its value.  An on_device batch waits for the
    producers of its tensors unless sync_inputs is False (Device.make_batch says when that is safe)."""
    b = struct_cls()
    required = _REQUIRED[struct_cls]
    for name, ctype in struct_cls._fields_:
        if name == "on_device":
            b.on_device = 1 if on_device else 0
        elif ctype is ctypes.c_void_p:
            setattr(b, name, _ptr(arrays[name] if name in required else arrays.get(name)))
        elif name in _DERIVED_COUNT and name not in arrays:
            setattr(b, name, _count(arrays.get(_DERIVED_COUNT[name])))
        else:
            setattr(b, name, int(arrays[name] if name in required else arrays.get(name, 0)))
    if on_device and sync_inputs:
        _sync_producers(arrays)
    return b


def _per_list(values, dtype, via=None) -> np.ndarray:
    """one entry per index list from the caller's shorter sequence, zero for the lists it does not reach"""
    out = np.zeros(MAX_INDEX_LISTS, dtype)
    out[: len(values)] = np.asarray(values, via or dtype)
    return out


def make_bits_batch(arrays: dict, on_device: bool = False, sync_inputs: bool = True) -> BgvBitsBatch:
    """arrays as verifier.encode_jobs_bits returns them: src is a SET_SRC_DTYPE
    record array (or an (n_sets, 4) uint32 array / tensor), bits a uint8 array;
    bits_len and n_indices default to the arrays' sizes"""
    return _fill(BgvBitsBatch, arrays, on_device, sync_inputs)


def bits_check(arrays: dict, list_len, on_device: bool = False) -> tuple[int, str]:
    """bgv_bits_check: the host-side contract of bgv_verify_bits, without a
    device.  list_len: the lengths of the index lists (0: not set).  Returns
    (status, bgv_last_error() text); the text is empty for BGV_OK."""
    lib = load_library()
    b = make_bits_batch(arrays, on_device, sync_inputs=False)
    ll = _per_list(list_len, np.uint32)
    st = lib.bgv_bits_check(ctypes.byref(b), ll.ctypes.data)
    return st, ("" if st == BGV_OK else lib.bgv_last_error().decode())


def make_smb_batch(arrays: dict, on_device: bool = False, sync_inputs: bool = True) -> BgvSmbBatch:
    """arrays as verifier.encode_same_message_bits returns them: the groups of a
    same-message batch, the sources of a bits batch; bits_len and n_indices
    default to the arrays' sizes"""
    return _fill(BgvSmbBatch, arrays, on_device, sync_inputs)


def smb_check(arrays: dict, list_len, on_device: bool = False) -> tuple[int, str]:
    """bgv_smb_check: the host-side contract of bgv_verify_same_message_bits,
    without a device.  list_len: the lengths of the index lists (0: not set).
    Returns (status, bgv_last_error() text); the text is empty for BGV_OK."""
    lib = load_library()
    b = make_smb_batch(arrays, on_device, sync_inputs=False)
    ll = _per_list(list_len, np.uint32)
    st = lib.bgv_smb_check(ctypes.byref(b), ll.ctypes.data)
    return st, ("" if st == BGV_OK else lib.bgv_last_error().decode())


def bits_plan(arrays: dict, list_len, list_has_sums=None, on_device: bool = False):
    """bgv_bits_plan: bgv_bits_check's checks, then the complement rule of
    bgv_index_list_sums, without a device.  list_has_sums: one flag per list
    (None: no list has sums).  Returns (status, error text, path uint8[n_sets],
    keys_gathered); path and keys_gathered are meaningful for BGV_OK on a host
    batch only."""
    lib = load_library()
    b = make_bits_batch(arrays, on_device, sync_inputs=False)
    ll = _per_list(list_len, np.uint32)
    hs = _per_list(() if list_has_sums is None else list_has_sums, np.uint8, bool)
    path = np.zeros(max(b.n_sets, 1), np.uint8)
    kg = ctypes.c_uint64()
    st = lib.bgv_bits_plan(ctypes.byref(b), ll.ctypes.data, hs.ctypes.data, path.ctypes.data, ctypes.byref(kg))
    return st, ("" if st == BGV_OK else lib.bgv_last_error().decode()), path[: b.n_sets], int(kg.value)


class Device:
    """One bgv_ctx: a HIP device, its stream and its HBM pubkey table."""

    def __init__(self, device: int = 0, **cfg):
        """cfg: bgv_cfg overrides (tests and A/B tools only), e.g. miller=36, split=0"""
        self.lib = load_library()
        h = ctypes.c_void_p()
        pair_merge = cfg.pop("pair_merge", None)  # a context call, not a bgv_cfg field (bgv_pair_merge)
        sm_retry = cfg.pop("sm_retry", None)      # likewise (bgv_sm_retry)
        if cfg:
            self._check(self.lib.bgv_open_cfg(device, ctypes.byref(BgvCfg.make(**cfg)), ctypes.byref(h)))
        else:
            self._check(self.lib.bgv_open(device, ctypes.byref(h)))
        self.h = h
        self.device = device
        self.last_stats = BgvStats()
        if pair_merge is not None:
            self.pair_merge(pair_merge)
        if sm_retry is not None:
            self.sm_retry(sm_retry)

    # -------------------------------------------------------------- helpers
    def _check(self, st: int):
        if st != BGV_OK:
            raise BgvNativeError(st, self.lib.bgv_last_error().decode())

    def _read(self, fn, struct_cls) -> dict:
        """a counter struct of the context, read by the getter fn(ctx, out), as a dict"""
        out = struct_cls()
        self._check(fn(self.h, ctypes.byref(out)))
        return out.as_dict()

    def stage_name(self, i: int) -> str:
        return self.lib.bgv_stage_name(i).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.bgv_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- pubkey table
    def pubkeys_set(self, first: int, data: bytes | np.ndarray, fmt: int):
        w = 48 if fmt == PK_COMPRESSED_48 else 96
        arr = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        n = arr.size // w
        self._check(self.lib.bgv_pubkeys_set(self.h, first, n, arr.ctypes.data, fmt))

    def pubkeys_count(self) -> int:
        c = ctypes.c_uint32()
        self._check(self.lib.bgv_pubkeys_count(self.h, ctypes.byref(c)))
        return c.value

    def pubkeys_get(self, first: int, n: int) -> bytes:
        out = np.zeros(n * 96, dtype=np.uint8)
        self._check(self.lib.bgv_pubkeys_get(self.h, first, n, out.ctypes.data))
        return out.tobytes()

    def pubkeys_validate(self, pk48: bytes) -> np.ndarray:
        """PublicKey.fromBytes(pk, affine, validate=true) for each 48-byte key
        (processDeposit.ts:59): per-key bgv_set_code (0 = valid)."""
        n = len(pk48) // 48
        buf = np.frombuffer(pk48, dtype=np.uint8).copy()
        codes = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.lib.bgv_pubkeys_validate(self.h, buf.ctypes.data, n, codes.ctypes.data))
        return codes[:n]

    def gen_keys(self, first: int, n: int, seed: int):
        self._check(self.lib.bgv_gen_keys(self.h, first, n, seed))

    # --------------------------------------------------------------- batches
    @staticmethod
    def make_batch(arrays: dict, on_device: bool = False, sync_inputs: bool = True) -> BgvBatch:
        """sync_inputs=False: the caller guarantees device-resident inputs are
        complete (e.g. one torch.cuda.synchronize() after they were written, for
        inputs that are only read afterwards), and the per-call wait for torch's
        current stream is skipped; that wait can sit behind other contexts'
        kernels on a shared hardware queue."""
        return _fill(BgvBatch, arrays, on_device, sync_inputs)

    def verify(self, arrays: dict, on_device: bool = False, want_set_codes: bool = True, sync_inputs: bool = True):
        """returns (job_result int32[n_jobs], set_code int32[n_sets] | None)"""
        b = self.make_batch(arrays, on_device, sync_inputs)
        jr = np.zeros(max(b.n_jobs, 1), dtype=np.int32)
        sc = np.zeros(max(b.n_sets, 1), dtype=np.int32) if want_set_codes else None
        self._check(self.lib.bgv_verify(self.h, ctypes.byref(b), jr.ctypes.data,
                                        sc.ctypes.data if sc is not None else None, ctypes.byref(self.last_stats)))
        return jr[: b.n_jobs], (sc[: b.n_sets] if sc is not None else None)

    @staticmethod
    def make_sm_batch(arrays: dict, on_device: bool = False, sync_inputs: bool = True) -> BgvSmBatch:
        """arrays as verifier.encode_same_message returns them"""
        return _fill(BgvSmBatch, arrays, on_device, sync_inputs)

    def _sm_call(self, fn, b, outs=(), agg=None) -> dict:
        """One call of a same-message entry.  Allocates set_valid, set_code and the entry's own outputs `outs`
        ((key, "n" or "G", row shape, dtype): one row per set or per group), resets last_sm_stats and calls
        fn(ctx, batch, set_valid, set_code, stats, *outs); returns every buffer cut to the batch's n sets and G
        groups, set_valid as bool.  agg: builds the bgv_sm_agg of the aggregate entry from the buffers, which then
        carries `outs` to the library as the argument after the batch."""
        rows = {"n": b.n_sets, "G": b.n_groups}
        spec = (("set_valid", "n", (), np.uint8), ("set_code", "n", (), np.int32)) + tuple(outs)
        buf = {k: np.zeros((max(rows[r], 1),) + shape, dt) for k, r, shape, dt in spec}
        self.last_sm_stats = BgvSmStats()
        a = agg(buf) if agg else None
        self._check(fn(self.h, ctypes.byref(b), *((ctypes.byref(a),) if agg else ()), buf["set_valid"].ctypes.data,
                       buf["set_code"].ctypes.data, ctypes.byref(self.last_sm_stats),
                       *(() if agg else [buf[k].ctypes.data for k, *_ in outs])))
        out = {k: buf[k][: rows[r]] for k, r, _shape, _dt in spec}
        out["set_valid"] = out["set_valid"].astype(bool)
        return out

    # the per-group and per-set values the debug entries return beside the verdicts
    _GROUP_OUTS = (("p_group", "G", (96,), np.uint8), ("s_group", "G", (192,), np.uint8), ("h_group", "G", (192,), np.uint8))
    _PK_SET_OUT = ("pk_set", "n", (96,), np.uint8)

    def verify_same_message(self, arrays: dict, on_device: bool = False, sync_inputs: bool = True):
        """bgv_verify_same_message: (set_valid bool[n_sets], set_code int32[n_sets]);
        the counters of the call are left in last_sm_stats"""
        o = self._sm_call(self.lib.bgv_verify_same_message, self.make_sm_batch(arrays, on_device, sync_inputs))
        return o["set_valid"], o["set_code"]

    def verify_same_message_aggregate(self, arrays: dict, take=None, prev=None, on_device: bool = False,
                                      sync_inputs: bool = True) -> dict:
        """bgv_verify_same_message_aggregate: the verdicts of verify_same_message plus,
        per group, the compressed sum of prev and the signatures of its sets with
        set_valid = 1 and take != 0.  take: uint8[n_sets] or None (every set); prev:
        uint8[n_groups, 96] or None; both device tensors for an on_device batch.
        Returns set_valid, set_code, agg_sig (G, 96) uint8, agg_count, agg_code, stats."""
        b = self.make_sm_batch(arrays, on_device, sync_inputs)
        if not on_device:
            take = None if take is None else np.ascontiguousarray(take, np.uint8)
            prev = None if prev is None else np.ascontiguousarray(prev, np.uint8)
        elif sync_inputs:
            _sync_producers(take, prev)
        outs = (("agg_sig", "G", (96,), np.uint8), ("agg_count", "G", (), np.uint32), ("agg_code", "G", (), np.int32))
        o = self._sm_call(self.lib.bgv_verify_same_message_aggregate, b, outs, agg=lambda buf: BgvSmAgg(
            take=_ptr(take), prev_sig96=_ptr(prev), agg_sig96=buf["agg_sig"].ctypes.data,
            agg_count=buf["agg_count"].ctypes.data, agg_code=buf["agg_code"].ctypes.data))
        return {**o, "stats": self.last_sm_stats.as_dict()}

    def sm_agg_ms(self) -> float:
        """bgv_sm_agg_ms: device time of the two sum kernels in the first pass of the last
        verify_same_message_aggregate"""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.bgv_sm_agg_ms(self.h, ctypes.byref(ms)))
        return float(ms.value)

    def debug_same_message(self, arrays: dict, on_device: bool = False) -> dict:
        """bgv_debug_same_message (test only): the verdicts plus P_g, S_g and H(m_g) per group"""
        o = self._sm_call(self.lib.bgv_debug_same_message, self.make_sm_batch(arrays, on_device), self._GROUP_OUTS)
        return {**o, "stats": self.last_sm_stats.as_dict()}

    @staticmethod
    def make_sma_batch(arrays: dict, on_device: bool = False, sync_inputs: bool = True) -> BgvSmaBatch:
        """arrays as verifier.encode_same_message_agg returns them"""
        return _fill(BgvSmaBatch, arrays, on_device, sync_inputs)

    def verify_same_message_agg(self, arrays: dict, on_device: bool = False, sync_inputs: bool = True):
        """bgv_verify_same_message_agg: (set_valid bool[n_sets], set_code int32[n_sets]);
        the counters of the call are left in last_sm_stats"""
        o = self._sm_call(self.lib.bgv_verify_same_message_agg, self.make_sma_batch(arrays, on_device, sync_inputs))
        return o["set_valid"], o["set_code"]

    def debug_same_message_agg(self, arrays: dict, on_device: bool = False) -> dict:
        """bgv_debug_same_message_agg (test only): the verdicts plus PK_i per set and
        P_g, S_g and H(m_g) per group"""
        o = self._sm_call(self.lib.bgv_debug_same_message_agg, self.make_sma_batch(arrays, on_device),
                          (self._PK_SET_OUT,) + self._GROUP_OUTS)
        return {**o, "stats": self.last_sm_stats.as_dict()}

    make_smb_batch = staticmethod(make_smb_batch)

    def verify_same_message_bits(self, arrays: dict, on_device: bool = False, sync_inputs: bool = True):
        """bgv_verify_same_message_bits: (set_valid bool[n_sets], set_code int32[n_sets]);
        the counters of the call are left in last_sm_stats, its key counts in bits_path_stats()"""
        o = self._sm_call(self.lib.bgv_verify_same_message_bits, make_smb_batch(arrays, on_device, sync_inputs))
        return o["set_valid"], o["set_code"]

    def debug_same_message_bits(self, arrays: dict, on_device: bool = False) -> dict:
        """bgv_debug_same_message_bits (test only): the outputs of debug_same_message_agg
        plus path uint8[n_sets] (1: complement path)"""
        o = self._sm_call(self.lib.bgv_debug_same_message_bits, make_smb_batch(arrays, on_device),
                          (self._PK_SET_OUT, ("path", "n", (), np.uint8)) + self._GROUP_OUTS)
        return {**o, "stats": self.last_sm_stats.as_dict()}

    # ------------------------------------------- committee bitfields (bgv_verify_bits)
    def index_list_set(self, list_id: int, indices) -> None:
        """bgv_index_list_set: replace resident index list list_id (an empty one drops it)"""
        arr = np.ascontiguousarray(indices, dtype=np.uint32)
        self._check(self.lib.bgv_index_list_set(self.h, list_id, arr.ctypes.data if arr.size else None, arr.size))

    def index_list_len(self, list_id: int) -> int:
        n = ctypes.c_uint32()
        self._check(self.lib.bgv_index_list_len(self.h, list_id, ctypes.byref(n)))
        return n.value

    def index_list_sums(self, list_id: int, enable: bool = True) -> None:
        """bgv_index_list_sums: build (or drop) the resident prefix sums of a list"""
        self._check(self.lib.bgv_index_list_sums(self.h, list_id, 1 if enable else 0))

    def index_list_sums_ms(self) -> float:
        """device time of this context's last index_list_sums build (HIP events)"""
        ms = ctypes.c_float()
        self._check(self.lib.bgv_index_list_sums_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def index_list_has_sums(self, list_id: int) -> bool:
        has = ctypes.c_uint32()
        self._check(self.lib.bgv_index_list_has_sums(self.h, list_id, ctypes.byref(has)))
        return bool(has.value)

    def hash_stats(self) -> dict:
        """bgv_hash_stats: {sets, hashes, dedup} of the last verify, verify_bits, partial or
        debug_stages on the context (hashes: the hash_to_G2 evaluations, the distinct signing
        roots when dedup is 1); zeros after a same-message call"""
        return self._read(self.lib.bgv_hash_stats, BgvHashPath)

    def pair_merge(self, on) -> None:
        """bgv_pair_merge: one Miller pair per distinct signing root of a job, from the next
        call on (bulk layout, one-lane loop; off by default).  on: bool, or 0 / 1."""
        self._check(self.lib.bgv_pair_merge(self.h, int(on)))

    def pair_stats(self) -> dict:
        """bgv_pair_stats: {sets, pairs, merged, fallback} of the last verify, verify_bits or
        partial on the context (pairs: the classes when merged is 1, else sets); zeros after
        any other entry"""
        return self._read(self.lib.bgv_pair_stats, BgvPairPath)

    def sm_retry(self, mode) -> None:
        """bgv_sm_retry: the retry of the same-message entries, from the next call on: 0 every
        surviving set of a failing segment as a one-set job (the default), 1 the split retry
        (subs of 8, then the sets of the failing subs).  mode: bool, or 0 / 1."""
        self._check(self.lib.bgv_sm_retry(self.h, int(mode)))

    def sm_retry_stats(self) -> dict:
        """bgv_sm_retry_stats: {mode, segments, subs, subs_failed, leaves, pairs, hashes} of the
        retry of the last same-message call on the context"""
        return self._read(self.lib.bgv_sm_retry_stats, BgvSmRetryPath)

    def batch_tail(self, mode) -> None:
        """bgv_batch_tail: the batch-first tail of the steps path, from the next call on:
        -1 auto (on wherever the steps path is), 0 off, 1 on."""
        self._check(self.lib.bgv_batch_tail(self.h, int(mode)))

    def tail_path(self) -> dict:
        """bgv_tail_stats: {batch_first, retried} of the last verify, verify_bits or partial
        (+ partial_finish) on the context"""
        return self._read(self.lib.bgv_tail_stats, BgvTailPath)

    def debug_pair_classes(self, arrays: dict, on_device: bool = False) -> dict:
        """bgv_debug_pair_classes (test only): verify through the merged path plus cls
        uint32[n_sets], class_off uint32[n_jobs + 1], p_class uint8[classes, 96], job_fe
        uint8[n_jobs, 576], batch_fe uint8[576], job_result, set_code"""
        b = self.make_batch(arrays, on_device)
        n, J = b.n_sets, b.n_jobs
        jr = np.zeros(max(J, 1), np.int32)
        sc = np.zeros(max(n, 1), np.int32)
        cls = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(J + 1, np.uint32)
        pc = np.zeros((max(n, 1), 96), np.uint8)
        jfe = np.zeros((max(J, 1), 576), np.uint8)
        bfe = np.zeros(576, np.uint8)
        self._check(self.lib.bgv_debug_pair_classes(self.h, ctypes.byref(b), jr.ctypes.data, sc.ctypes.data, cls.ctypes.data,
                                                    off.ctypes.data, pc.ctypes.data, jfe.ctypes.data, bfe.ctypes.data))
        return {"job_result": jr[:J], "set_code": sc[:n], "cls": cls[:n], "class_off": off, "p_class": pc[: int(off[J])],
                "job_fe": jfe[:J], "batch_fe": bfe}

    def miller_path(self) -> dict:
        """bgv_miller_path_stats: {steps, slice_sets, items} of the last verify, verify_bits,
        partial or debug_stages on the context (steps 1: per-step line products, bgv_cfg.miller_steps)"""
        return self._read(self.lib.bgv_miller_path_stats, BgvMillerPath)

    def bits_path_stats(self) -> dict:
        """bgv_bits_path_stats: {sets_complement, keys_expanded, keys_gathered} of the last
        verify_bits or verify_same_message_bits"""
        return self._read(self.lib.bgv_bits_path_stats, BgvBitsPath)

    bits_plan = staticmethod(bits_plan)

    def debug_bits_keys(self, arrays: dict, on_device: bool = False):
        """bgv_debug_bits_keys (test only): (pk_agg uint8[n_sets, 96], path uint8[n_sets], pk_code int32[n_sets])"""
        b = make_bits_batch(arrays, on_device)
        n = b.n_sets
        pk = np.zeros((max(n, 1), 96), np.uint8)
        path = np.zeros(max(n, 1), np.uint8)
        code = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.bgv_debug_bits_keys(self.h, ctypes.byref(b), pk.ctypes.data, path.ctypes.data, code.ctypes.data))
        return pk[:n], path[:n], code[:n]

    def debug_index_list_sums(self, list_id: int, first: int, n: int) -> np.ndarray:
        """bgv_debug_index_list_sums (test only): S[first .. first + n) as affine 96 B rows (zero: the identity)"""
        out = np.zeros((max(n, 1), 96), np.uint8)
        self._check(self.lib.bgv_debug_index_list_sums(self.h, list_id, first, n, out.ctypes.data))
        return out[:n]

    make_bits_batch = staticmethod(make_bits_batch)

    def verify_bits(self, arrays: dict, on_device: bool = False, want_set_codes: bool = True, sync_inputs: bool = True):
        """bgv_verify_bits: (job_result int32[n_jobs], set_code int32[n_sets] | None), as verify()"""
        b = make_bits_batch(arrays, on_device, sync_inputs)
        jr = np.zeros(max(b.n_jobs, 1), dtype=np.int32)
        sc = np.zeros(max(b.n_sets, 1), dtype=np.int32) if want_set_codes else None
        self._check(self.lib.bgv_verify_bits(self.h, ctypes.byref(b), jr.ctypes.data,
                                             sc.ctypes.data if sc is not None else None, ctypes.byref(self.last_stats)))
        return jr[: b.n_jobs], (sc[: b.n_sets] if sc is not None else None)

    def debug_bits_expand(self, arrays: dict, on_device: bool = False, cap: int | None = None):
        """bgv_debug_bits_expand (test only): (pk_offsets uint32[n_sets + 1], pk_indices uint32[total]).
        cap: room for the indices (default: found by a first call)"""
        b = make_bits_batch(arrays, on_device)
        po = np.zeros(b.n_sets + 1, np.uint32)
        total = ctypes.c_uint32()
        if cap is None:
            st = self.lib.bgv_debug_bits_expand(self.h, ctypes.byref(b), po.ctypes.data, None, 0, ctypes.byref(total))
            if st != BGV_OK and not (st == BGV_E_INVALID_ARG and total.value > 0):
                self._check(st)
            cap = total.value
        idx = np.zeros(max(cap, 1), np.uint32)
        self._check(self.lib.bgv_debug_bits_expand(self.h, ctypes.byref(b), po.ctypes.data, idx.ctypes.data, cap,
                                                   ctypes.byref(total)))
        return po, idx[: total.value]

    def bits_expand_ms(self) -> float:
        """device time of the last verify_bits' expansion kernels (timed contexts; else 0)"""
        ms = ctypes.c_float()
        self._check(self.lib.bgv_bits_expand_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def partial(self, arrays: dict, on_device: bool = False, sync_inputs: bool = True):
        """bgv_partial: (miller576 bytes, set codes, provisional job results
        (-code rejected / 1 pending the combined check), no-job-rejected)."""
        b = self.make_batch(arrays, on_device, sync_inputs)
        out = np.zeros(576, dtype=np.uint8)
        sc = np.zeros(max(b.n_sets, 1), dtype=np.int32)
        jr = np.zeros(max(b.n_jobs, 1), dtype=np.int32)
        ok = ctypes.c_int32()
        self._check(self.lib.bgv_partial(self.h, ctypes.byref(b), out.ctypes.data, sc.ctypes.data, jr.ctypes.data,
                                         ctypes.byref(ok)))
        self._partial_jobs = b.n_jobs
        self._check(self.lib.bgv_last_stats(self.h, ctypes.byref(self.last_stats)))
        return out.tobytes(), sc[: b.n_sets], jr[: b.n_jobs], bool(ok.value)

    def partial_finish(self) -> np.ndarray:
        """bgv_partial_finish: per-job verdicts of the shard left by partial()."""
        n = getattr(self, "_partial_jobs", 0)
        jr = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.lib.bgv_partial_finish(self.h, jr.ctypes.data, ctypes.byref(self.last_stats)))
        return jr[:n]

    def debug_stages(self, arrays: dict, on_device: bool = False) -> dict:
        """bgv_debug_stages (test only): per-stage canonical values as numpy arrays."""
        b = self.make_batch(arrays, on_device)
        n, J = b.n_sets, b.n_jobs
        bufs = {"sig_aff": np.zeros((max(n, 1), 192), np.uint8), "h_aff": np.zeros((max(n, 1), 192), np.uint8),
                "pk_agg": np.zeros((max(n, 1), 96), np.uint8), "rpk_aff": np.zeros((max(n, 1), 96), np.uint8),
                "s_aff": np.zeros((max(J, 1), 192), np.uint8), "pair_fe": np.zeros((max(n + J, 1), 576), np.uint8),
                "job_fe": np.zeros((max(J, 1), 576), np.uint8), "batch_fe": np.zeros(576, np.uint8)}
        dbg = BgvDebug(**{k: v.ctypes.data for k, v in bufs.items()})
        jr = np.zeros(max(J, 1), dtype=np.int32)
        sc = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.lib.bgv_debug_stages(self.h, ctypes.byref(b), jr.ctypes.data, sc.ctypes.data, ctypes.byref(dbg)))
        out = {k: (v[: n] if k in ("sig_aff", "h_aff", "pk_agg", "rpk_aff") else v[: J] if k in ("s_aff", "job_fe")
                   else v[: n + J] if k == "pair_fe" else v) for k, v in bufs.items()}
        out["job_result"] = jr[:J]
        out["set_code"] = sc[:n]
        return out

    def combine_final(self, partials: list[bytes]) -> bool:
        buf = np.frombuffer(b"".join(partials), dtype=np.uint8) if partials else np.zeros(1, np.uint8)
        r = ctypes.c_int32()
        self._check(self.lib.bgv_combine_final(self.h, buf.ctypes.data, len(partials), ctypes.byref(r)))
        return bool(r.value)

    def gen_sign(self, arrays: dict, out, on_device: bool = False):
        _sync_producers(out)
        b = self.make_batch(arrays, on_device)
        self._check(self.lib.bgv_gen_sign(self.h, ctypes.byref(b), _ptr(out)))

    def debug_fp_ops(self, ab: np.ndarray) -> np.ndarray:
        """Device modular add/sub primitives (test only): ab is (n, 2, 12) u32
        limbs; returns (n, FP_OPS_N, 12) u32 (include/bgv.h bgv_debug_fp_ops)."""
        ab = np.ascontiguousarray(ab, dtype=np.uint32)
        n = ab.shape[0]
        out = np.zeros((n, FP_OPS_N, 12), np.uint32)
        self._check(self.lib.bgv_debug_fp_ops(self.h, ab.ctypes.data, n, out.ctypes.data))
        return out

    def debug_g2_decode(self, sigs192: np.ndarray, sig_len: np.ndarray):
        """Signature decode without the subgroup check (test only): sigs192 is
        (n, 192) u8, sig_len (n,) u32; returns ((n, 192) u8 affine points as
        x.c0 || x.c1 || y.c0 || y.c1 big-endian, (n,) i32 set codes)
        (include/bgv.h bgv_debug_g2_decode)."""
        sigs192 = np.ascontiguousarray(sigs192, dtype=np.uint8)
        sig_len = np.ascontiguousarray(sig_len, dtype=np.uint32)
        n = sig_len.shape[0]
        assert sigs192.shape == (n, 192)
        out = np.zeros((n, 192), np.uint8)
        codes = np.zeros(n, np.int32)
        self._check(self.lib.bgv_debug_g2_decode(self.h, sigs192.ctypes.data, sig_len.ctypes.data, n, out.ctypes.data,
                                                 codes.ctypes.data))
        return out, codes

    # ---------------------------------------------------------- microbench
    def bench_fpmul(self, lanes: int, iters: int) -> float:
        ms = ctypes.c_float()
        self._check(self.lib.bgv_bench_fpmul(self.h, lanes, iters, ctypes.byref(ms)))
        return ms.value

    def bench_mad(self, lanes: int, iters: int) -> float:
        ms = ctypes.c_float()
        self._check(self.lib.bgv_bench_mad(self.h, lanes, iters, ctypes.byref(ms)))
        return ms.value
