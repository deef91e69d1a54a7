"""ctypes bindings for libdbeel_gpu.so — the product compaction engine.

The HIP library is the product path: if it is missing or no GPU is present,
every call raises loudly (no CPU fallback — the CPU restatement in oracle/
is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .format import INDEX_DTYPE

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "libdbeel_gpu.so")

ERROR_NAMES = {
    0: "OK",
    1: "INVALID_ARG",
    2: "CORRUPT",
    3: "ITEM_TOO_LARGE",
    4: "HIP",
    5: "NO_GPU",
    6: "OOM",
    7: "IO",
}


class DbeelGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dbeel_gpu error {ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


class RunView(ctypes.Structure):
    _fields_ = [
        ("data", ctypes.POINTER(ctypes.c_uint8)),
        ("data_len", ctypes.c_size_t),
        ("index", ctypes.POINTER(ctypes.c_uint8)),
        ("index_len", ctypes.c_size_t),
    ]


class CompactResult(ctypes.Structure):
    _fields_ = [
        ("data", ctypes.POINTER(ctypes.c_uint8)),
        ("data_len", ctypes.c_size_t),
        ("index", ctypes.POINTER(ctypes.c_uint8)),
        ("index_len", ctypes.c_size_t),
        ("entries_written", ctypes.c_uint64),
    ]


class CompactTimings(ctypes.Structure):
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("prep_ms", ctypes.c_double),
        ("rank_ms", ctypes.c_double),
        ("scan_ms", ctypes.c_double),
        ("emit_ms", ctypes.c_double),
        ("copy_ms", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _ptr_bytes(ptr, n: int) -> bytes:
    """Copy n bytes from a ctypes uint8 pointer. ctypes.string_at truncates
    its size argument to 32 bits on this interpreter (CPython 3.10), which
    silently corrupts >4 GB results — use a numpy view instead."""
    if not n:
        return b""
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).tobytes()


_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} not built — run __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950). The product path has no "
                "CPU fallback."
            )
        lib = ctypes.CDLL(LIB_PATH)
        lib.dbeel_gpu_compact_timed.restype = ctypes.c_int
        lib.dbeel_gpu_compact_timed.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t, ctypes.c_int,
            ctypes.c_int, ctypes.POINTER(CompactResult),
            ctypes.POINTER(CompactTimings),
        ]
        lib.dbeel_gpu_result_free.argtypes = [ctypes.POINTER(CompactResult)]
        lib.dbeel_gpu_last_error.restype = ctypes.c_char_p
        lib.dbeel_gpu_job_create.restype = ctypes.c_int
        lib.dbeel_gpu_job_create.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t, ctypes.c_int,
            ctypes.POINTER(ctypes.c_void_p),
        ]
        lib.dbeel_gpu_job_run.restype = ctypes.c_int
        lib.dbeel_gpu_job_run.argtypes = [
            ctypes.c_void_p, ctypes.c_int,
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(CompactTimings),
        ]
        lib.dbeel_gpu_job_fetch.restype = ctypes.c_int
        lib.dbeel_gpu_job_fetch.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(CompactResult)
        ]
        lib.dbeel_gpu_job_destroy.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_encode_run.restype = ctypes.c_int
        lib.dbeel_gpu_encode_run.argtypes = [
            ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_int,
            ctypes.POINTER(CompactResult),
        ]
        lib.dbeel_gpu_pin_host.restype = ctypes.c_int
        lib.dbeel_gpu_pin_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        lib.dbeel_gpu_unpin_host.restype = ctypes.c_int
        lib.dbeel_gpu_unpin_host.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_job_ingest.restype = ctypes.c_int
        lib.dbeel_gpu_job_ingest.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(RunView), ctypes.c_size_t,
            ctypes.POINTER(IngestStats),
        ]
        lib.dbeel_gpu_compact_sliced.restype = ctypes.c_int
        lib.dbeel_gpu_compact_sliced.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t, ctypes.c_int,
            ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(CompactResult),
        ]
        lib.dbeel_gpu_scan.restype = ctypes.c_int
        lib.dbeel_gpu_scan.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
            ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(CompactResult),
        ]
        lib.dbeel_gpu_grid_for.restype = ctypes.c_uint32
        lib.dbeel_gpu_grid_for.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
        _lib = lib
    return _lib


def grid_for(work_items: int, block: int = 256) -> int:
    """dbeel_gpu_grid_for: the blocks a launch over work_items items gets
    (capped; a grid-stride loop covers the rest). Host arithmetic only."""
    return int(load().dbeel_gpu_grid_for(int(work_items), int(block)))


def _as_u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, dtype=np.uint8)
    return np.frombuffer(buf, dtype=np.uint8)


def _views(runs):
    keep = []
    views = (RunView * len(runs))()
    for i, (d, x) in enumerate(runs):
        d = _as_u8(d)
        x = _as_u8(x)
        keep += [d, x]
        views[i].data = d.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        views[i].data_len = d.nbytes
        views[i].index = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        views[i].index_len = x.nbytes
    return views, keep


def compact(runs, keep_tombstones: bool, device: int = 0,
            want_timings: bool = False):
    """Compact runs [(data, index), ...] on `device`.

    Returns (data_bytes, index_bytes, entries_written[, timings_dict]).
    """
    lib = load()
    views, keepalive = _views(runs)
    res = CompactResult()
    tim = CompactTimings()
    rc = lib.dbeel_gpu_compact_timed(
        views, len(runs), int(keep_tombstones), device,
        ctypes.byref(res), ctypes.byref(tim),
    )
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    try:
        data = _ptr_bytes(res.data, res.data_len)
        index = _ptr_bytes(res.index, res.index_len)
        n = int(res.entries_written)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    del keepalive
    if want_timings:
        return data, index, n, tim.as_dict()
    return data, index, n


def scan(runs, start_key: bytes | None = None,
         end_key: bytes | None = None, hash_ranges=None, device: int = 0):
    """Migration/iteration scan (AsyncIter analogue, lsm_tree.rs:141-282 +
    tasks/migration.rs:62-131): yields every entry in the reference's
    order — runs ascending, entries in key order within each — with no
    dedup and no tombstone filter, restricted by an optional key range
    [start_key, end_key) and/or murmur3_32 hash ranges [(start, end), ...]
    (hash_bytes shards.rs:99-101, between_cmp migration.rs:54-60).
    Returns (data_bytes, index_bytes, n) shaped like a run file."""
    lib = load()
    views, keepalive = _views(runs)

    def _kb(b):
        if b is None:
            return None, 0, None
        a = np.frombuffer(b or b"\0", dtype=np.uint8)
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(b), a

    sp, sl, sa = _kb(start_key)
    ep, el, ea = _kb(end_key)
    n_ranges = len(hash_ranges) if hash_ranges else 0
    if n_ranges:
        rs = np.array([r[0] for r in hash_ranges], dtype=np.uint32)
        re_ = np.array([r[1] for r in hash_ranges], dtype=np.uint32)
        rsp = rs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        rep = re_.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    else:
        rsp = rep = None
    res = CompactResult()
    rc = lib.dbeel_gpu_scan(views, len(runs), sp, sl, ep, el, rsp, rep,
                            n_ranges, device, ctypes.byref(res))
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    try:
        data = _ptr_bytes(res.data, res.data_len)
        index = _ptr_bytes(res.index, res.index_len)
        n = int(res.entries_written)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    del keepalive
    return data, index, n


class IngestStats(ctypes.Structure):
    _fields_ = [
        ("ingest_ms", ctypes.c_double),
        ("copy_ms", ctypes.c_double),
        ("prep_ms", ctypes.c_double),
        ("bytes", ctypes.c_uint64),
        ("chunks", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def pin_host(arr: np.ndarray) -> None:
    """Page-lock a numpy buffer (hipHostRegister) so streamed ingest runs
    as true async DMA. Pin once, outside the hot loop."""
    lib = load()
    rc = lib.dbeel_gpu_pin_host(arr.ctypes.data, arr.nbytes)
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


def unpin_host(arr: np.ndarray) -> None:
    lib = load()
    rc = lib.dbeel_gpu_unpin_host(arr.ctypes.data)
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


def compact_sliced(runs, keep_tombstones: bool, device: int = 0,
                   max_resident_bytes: int = 0):
    """Sliced compaction for inputs larger than HBM: key space cut at
    pivots, each slice compacted on-device, outputs concatenated —
    byte-identical to one whole compaction (include/dbeel_gpu.h)."""
    lib = load()
    views, keepalive = _views(runs)
    res = CompactResult()
    rc = lib.dbeel_gpu_compact_sliced(
        views, len(runs), int(keep_tombstones), device,
        max_resident_bytes, ctypes.byref(res),
    )
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    try:
        data = _ptr_bytes(res.data, res.data_len)
        index = _ptr_bytes(res.index, res.index_len)
        n = int(res.entries_written)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    del keepalive
    return data, index, n


class CompactIntoResult(ctypes.Structure):
    """dbeel_compact_into_result."""
    _fields_ = [
        ("data_len", ctypes.c_uint64),
        ("index_len", ctypes.c_uint64),
        ("entries_written", ctypes.c_uint64),
    ]


class CompactIntoStats(ctypes.Structure):
    """dbeel_compact_into_stats."""
    _fields_ = [
        ("slices", ctypes.c_uint64),
        ("bytes_in", ctypes.c_uint64),
        ("bytes_out", ctypes.c_uint64),
        ("h2d_ms", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("wall_ms", ctypes.c_double),
        ("overlap_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _load_into(lib):
    if not hasattr(lib, "_into_ready"):
        u8p = ctypes.POINTER(ctypes.c_uint8)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        lib.dbeel_gpu_job_fetch_into.restype = ctypes.c_int
        lib.dbeel_gpu_job_fetch_into.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p,
            ctypes.POINTER(ctypes.c_double)]
        lib.dbeel_gpu_compact_into.restype = ctypes.c_int
        lib.dbeel_gpu_compact_into.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t, ctypes.c_int,
            ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
            ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(u8p), u64p,
            ctypes.POINTER(CompactIntoResult),
            ctypes.POINTER(CompactIntoStats)]
        lib.dbeel_gpu_bloom_free.restype = None
        lib.dbeel_gpu_bloom_free.argtypes = [u8p]
        lib._into_ready = True
    return lib


def compact_into(runs, keep_tombstones: bool, data_arr: np.ndarray,
                 index_arr: np.ndarray, device: int = 0,
                 max_resident_bytes: int = 0, n_slices: int = 0,
                 bloom: bool = False):
    """dbeel_gpu_compact_into: compact runs [(data, index), ...] into the
    caller's numpy u8 arrays (passed by pointer, so arrays registered with
    pin_host receive true async DMA), in n_slices pipelined key slices
    (0 = as many as max_resident_bytes / free device memory ask for). The
    bytes written equal compact()'s.

    Returns (data_len, index_len, entries_written, stats_dict, bloom_bytes);
    bloom_bytes is the "DBLM" filter over the surviving keys, None unless
    bloom. Arrays too small raise DbeelGpuError with code 3 and .needed =
    (data_len, index_len); nothing past the arrays' ends is written."""
    lib = _load_into(load())
    views, keepalive = _views(runs)
    res = CompactIntoResult()
    st = CompactIntoStats()
    bp = ctypes.POINTER(ctypes.c_uint8)()
    bn = ctypes.c_uint64()
    rc = lib.dbeel_gpu_compact_into(
        views, len(runs), int(keep_tombstones), device,
        int(max_resident_bytes), int(n_slices),
        data_arr.ctypes.data, data_arr.nbytes,
        index_arr.ctypes.data, index_arr.nbytes, int(bool(bloom)),
        ctypes.byref(bp) if bloom else None,
        ctypes.byref(bn) if bloom else None,
        ctypes.byref(res), ctypes.byref(st))
    del keepalive
    if rc != 0:
        err = DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
        err.needed = (int(res.data_len), int(res.index_len))
        err.stats = st.as_dict()
        raise err
    bloom_bytes = None
    if bloom:
        try:
            bloom_bytes = _ptr_bytes(bp, int(bn.value))
        finally:
            lib.dbeel_gpu_bloom_free(bp)
    return (int(res.data_len), int(res.index_len), int(res.entries_written),
            st.as_dict(), bloom_bytes)


class LookupHit(ctypes.Structure):
    _fields_ = [
        ("run", ctypes.c_int32),
        ("is_tombstone", ctypes.c_uint32),
        ("value_offset", ctypes.c_uint64),
        ("value_len", ctypes.c_uint64),
    ]


def lookup(runs, keys, device: int = 0):
    """Batched point lookup (LSMTree::get over sstables,
    lsm_tree.rs:605-723): for each key returns the value bytes of the
    first match scanning runs newest-index-first (the reference's
    `sstables.iter().rev()`, lsm_tree.rs:692-696 — highest run index
    wins), b"" for a deleted key (tombstone), or None if absent."""
    lib = load()
    if not hasattr(lib, "_lookup_ready"):
        lib.dbeel_gpu_lookup.restype = ctypes.c_int
        lib.dbeel_gpu_lookup.argtypes = [
            ctypes.POINTER(RunView), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64),
            ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(LookupHit),
        ]
        lib._lookup_ready = True
    views, keepalive = _views(runs)
    blob = b"".join(keys)
    koff = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keys], out=koff[1:])
    ka = np.frombuffer(blob or b"\0", dtype=np.uint8)
    hits = (LookupHit * len(keys))()
    rc = lib.dbeel_gpu_lookup(
        views, len(runs),
        ka.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        len(keys), device, hits,
    )
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    out = []
    datas = [bytes(_as_u8(d)) if not isinstance(d, bytes) else d
             for d, _ in runs]
    for h in hits:
        if h.run < 0:
            out.append(None)
        elif h.is_tombstone:
            out.append(b"")
        else:
            out.append(
                datas[h.run][h.value_offset : h.value_offset + h.value_len]
            )
    del keepalive
    return out


HIT_DTYPE = np.dtype(
    [("run", "<i4"), ("is_tombstone", "<u4"), ("value_offset", "<u8"),
     ("value_len", "<u8")]
)
assert HIT_DTYPE.itemsize == ctypes.sizeof(LookupHit)


def _key_blob(keys):
    """keys -> (u8 blob array, n+1 u64 offsets) in the C ABI's layout."""
    blob = b"".join(keys)
    koff = np.zeros(len(keys) + 1, dtype=np.uint64)
    lens = np.fromiter((len(k) for k in keys), dtype=np.uint64,
                       count=len(keys))
    np.cumsum(lens, out=koff[1:])
    return np.frombuffer(blob or b"\0", dtype=np.uint8), koff


def lookup_raw(runs, keys, device: int = 0) -> np.ndarray:
    """dbeel_gpu_lookup's hit records as a HIT_DTYPE array (run = -1
    absent, value_offset into runs[run].data) — the field-for-field
    comparison target of Reader.get_raw."""
    lib = load()
    lib.dbeel_gpu_lookup.restype = ctypes.c_int
    lib.dbeel_gpu_lookup.argtypes = [
        ctypes.POINTER(RunView), ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(LookupHit),
    ]
    views, keepalive = _views(runs)
    ka, koff = _key_blob(keys)
    hits = np.zeros(len(keys), dtype=HIT_DTYPE)
    rc = lib.dbeel_gpu_lookup(
        views, len(runs),
        ka.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        len(keys), device,
        hits.ctypes.data_as(ctypes.POINTER(LookupHit)),
    )
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    del keepalive
    return hits


class BloomView(ctypes.Structure):
    _fields_ = [
        ("bytes", ctypes.POINTER(ctypes.c_uint8)),
        ("len", ctypes.c_size_t),
    ]


class GetResult(ctypes.Structure):
    _fields_ = [
        ("hits", ctypes.POINTER(LookupHit)),
        ("value_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("values", ctypes.POINTER(ctypes.c_uint8)),
        ("values_len", ctypes.c_uint64),
        ("n_keys", ctypes.c_uint64),
    ]


class GetStats(ctypes.Structure):
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("search_ms", ctypes.c_double),
        ("gather_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("bloom_probes", ctypes.c_uint64),
        ("bloom_skips", ctypes.c_uint64),
        ("searches", ctypes.c_uint64),
        ("hits", ctypes.c_uint64),
        ("tombstones", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GetBuffers(ctypes.Structure):
    """dbeel_get_buffers: all caller-owned."""
    _fields_ = [
        ("hits", ctypes.POINTER(LookupHit)),
        ("record_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("records", ctypes.POINTER(ctypes.c_uint8)),
        ("records_cap", ctypes.c_uint64),
    ]


class GetPage(ctypes.Structure):
    """dbeel_get_page."""
    _fields_ = [
        ("n_done", ctypes.c_uint64),
        ("records_len", ctypes.c_uint64),
        ("records_total", ctypes.c_uint64),
        ("needed", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


MERGE_ANSWERS = 0   # DBEEL_MERGE_ANSWERS
MERGE_READER = 1    # DBEEL_MERGE_READER
MERGE_MAX_SOURCES = 15


class MergeSource(ctypes.Structure):
    """dbeel_merge_source."""
    _fields_ = [
        ("kind", ctypes.c_int),
        ("reader", ctypes.c_void_p),
        ("record_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("records", ctypes.POINTER(ctypes.c_uint8)),
    ]


class MergeHit(ctypes.Structure):
    """dbeel_merge_hit."""
    _fields_ = [
        ("source", ctypes.c_int32),
        ("is_tombstone", ctypes.c_uint32),
        ("value_len", ctypes.c_uint64),
        ("stale_mask", ctypes.c_uint64),
    ]


MERGE_HIT_DTYPE = np.dtype(
    [("source", "<i4"), ("is_tombstone", "<u4"), ("value_len", "<u8"),
     ("stale_mask", "<u8")]
)
assert MERGE_HIT_DTYPE.itemsize == ctypes.sizeof(MergeHit)


class MergeBuffers(ctypes.Structure):
    """dbeel_merge_buffers: all caller-owned."""
    _fields_ = [
        ("hits", ctypes.POINTER(MergeHit)),
        ("record_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("records", ctypes.POINTER(ctypes.c_uint8)),
        ("records_cap", ctypes.c_uint64),
    ]


class MergeStats(ctypes.Structure):
    """dbeel_merge_stats."""
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("search_ms", ctypes.c_double),
        ("pick_ms", ctypes.c_double),
        ("gather_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("winners", ctypes.c_uint64),
        ("tombstones", ctypes.c_uint64),
        ("from_local", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReaderCompactStats(ctypes.Structure):
    _fields_ = [
        ("pipeline", CompactTimings),
        ("adopt_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("d2h_bytes", ctypes.c_uint64),
        ("entries_in", ctypes.c_uint64),
        ("entries_out", ctypes.c_uint64),
        ("data_bytes_out", ctypes.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[1:]}
        d["pipeline"] = self.pipeline.as_dict()
        return d


class WriteBatchStats(ctypes.Structure):
    """dbeel_write_batch_stats."""
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("order_ms", ctypes.c_double),
        ("encode_ms", ctypes.c_double),
        ("adopt_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("writes_in", ctypes.c_uint64),
        ("entries_out", ctypes.c_uint64),
        ("data_bytes_out", ctypes.c_uint64),
        ("prefix_tied", ctypes.c_uint64),
        ("d2h_bytes", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MemtablePutStats(ctypes.Structure):
    """dbeel_memtable_put_stats."""
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("order_ms", ctypes.c_double),
        ("merge_ms", ctypes.c_double),
        ("writes_in", ctypes.c_uint64),
        ("batch_entries", ctypes.c_uint64),
        ("replaced", ctypes.c_uint64),
        ("entries", ctypes.c_uint64),
        ("data_bytes", ctypes.c_uint64),
        ("prefix_tied", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MemtableInfo(ctypes.Structure):
    """dbeel_memtable_info."""
    _fields_ = [
        ("entries", ctypes.c_uint64),
        ("data_bytes", ctypes.c_uint64),
        ("reserved_bytes", ctypes.c_uint64),
        ("puts", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PutEntriesStats(ctypes.Structure):
    """dbeel_put_entries_stats."""
    _fields_ = [
        ("h2d_ms", ctypes.c_double),
        ("order_ms", ctypes.c_double),
        ("merge_ms", ctypes.c_double),
        ("entries_in", ctypes.c_uint64),
        ("selected", ctypes.c_uint64),
        ("batch_entries", ctypes.c_uint64),
        ("replaced", ctypes.c_uint64),
        ("entries", ctypes.c_uint64),
        ("data_bytes", ctypes.c_uint64),
        ("prefix_tied", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ApplyAction(ctypes.Structure):
    """dbeel_apply_action."""
    _fields_ = [
        ("kind", ctypes.c_int),
        ("dst", ctypes.c_void_p),
    ]


class ScanApplyStats(ctypes.Structure):
    """dbeel_scan_apply_stats."""
    _fields_ = [
        ("apply_ms", ctypes.c_double),
        ("put_entries", ctypes.c_uint64),
        ("delete_entries", ctypes.c_uint64),
        ("skipped", ctypes.c_uint64),
        ("groups", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


APPLY_SKIP = 0     # DBEEL_APPLY_SKIP
APPLY_PUT = 1      # DBEEL_APPLY_PUT
APPLY_DELETE = 2   # DBEEL_APPLY_DELETE
_APPLY_KINDS = {"skip": APPLY_SKIP, "put": APPLY_PUT, "delete": APPLY_DELETE}


def _ts16(ts):
    """A timestamp (int, or 16 raw bytes) as a u8[16] array, i128 LE."""
    if ts is None:
        return None
    raw = (bytes(ts) if isinstance(ts, (bytes, bytearray))
           else int(ts).to_bytes(16, "little", signed=True))
    if len(raw) != 16:
        raise ValueError("a timestamp is 16 bytes")
    return np.frombuffer(raw, dtype=np.uint8)


_U8P = ctypes.POINTER(ctypes.c_uint8)
_U64P = ctypes.POINTER(ctypes.c_uint64)
_BATCH_ARGTYPES = [ctypes.c_uint64, _U8P, _U64P, _U8P, _U64P, _U8P]


def _write_arrays(writes):
    """A write batch — an iterable of (key, value, timestamp) in arrival
    order, unsorted, keys may repeat, b"" = tombstone — as the C ABI's
    arrays: (n, [five ctypes pointers], keepalive)."""
    writes = list(writes)
    n = len(writes)
    ka = np.frombuffer(b"".join(w[0] for w in writes) or b"\0", dtype=np.uint8)
    va = np.frombuffer(b"".join(w[1] for w in writes) or b"\0", dtype=np.uint8)
    koff = np.zeros(n + 1, dtype=np.uint64)
    voff = np.zeros(n + 1, dtype=np.uint64)
    koff[1:] = np.cumsum(np.array([len(w[0]) for w in writes], dtype=np.uint64))
    voff[1:] = np.cumsum(np.array([len(w[1]) for w in writes], dtype=np.uint64))
    ts = np.frombuffer(
        b"".join(int(w[2]).to_bytes(16, "little", signed=True)
                 for w in writes) or b"\0", dtype=np.uint8)
    ptrs = [ka.ctypes.data_as(_U8P), koff.ctypes.data_as(_U64P),
            va.ctypes.data_as(_U8P), voff.ctypes.data_as(_U64P),
            ts.ctypes.data_as(_U8P)]
    return n, ptrs, (ka, va, koff, voff, ts)


def _load_reader() -> ctypes.CDLL:
    lib = load()
    if not hasattr(lib, "_reader_ready"):
        lib.dbeel_gpu_reader_open.restype = ctypes.c_int
        lib.dbeel_gpu_reader_open.argtypes = [
            ctypes.POINTER(RunView), ctypes.POINTER(BloomView),
            ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ]
        lib.dbeel_gpu_reader_table_bytes.restype = ctypes.c_uint64
        lib.dbeel_gpu_reader_table_bytes.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_get.restype = ctypes.c_int
        lib.dbeel_gpu_reader_get.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8),
            ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64,
            ctypes.POINTER(GetResult), ctypes.POINTER(GetStats),
        ]
        lib.dbeel_gpu_get_result_free.restype = None
        lib.dbeel_gpu_get_result_free.argtypes = [ctypes.POINTER(GetResult)]
        lib.dbeel_gpu_reader_close.restype = None
        lib.dbeel_gpu_reader_close.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_run_count.restype = ctypes.c_size_t
        lib.dbeel_gpu_reader_run_count.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_insert_run.restype = ctypes.c_int
        lib.dbeel_gpu_reader_insert_run.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(RunView),
            ctypes.POINTER(BloomView),
        ]
        lib.dbeel_gpu_reader_compact_begin.restype = ctypes.c_int
        lib.dbeel_gpu_reader_compact_begin.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
            ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(CompactResult),
            ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
            ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ReaderCompactStats),
        ]
        lib.dbeel_gpu_reader_compact_commit.restype = ctypes.c_int
        lib.dbeel_gpu_reader_compact_commit.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t]
        lib.dbeel_gpu_reader_compact_abort.restype = None
        lib.dbeel_gpu_reader_compact_abort.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_bloom_free.restype = None
        lib.dbeel_gpu_bloom_free.argtypes = [ctypes.POINTER(ctypes.c_uint8)]
        lib.dbeel_gpu_reader_scan_begin.restype = ctypes.c_int
        lib.dbeel_gpu_reader_scan_begin.argtypes = [
            ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
            ctypes.c_size_t, ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_void_p),
        ]
        lib.dbeel_gpu_reader_scan_next.restype = ctypes.c_int
        lib.dbeel_gpu_reader_scan_next.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
            ctypes.POINTER(ScanPage),
        ]
        lib.dbeel_gpu_reader_scan_end.restype = None
        lib.dbeel_gpu_reader_scan_end.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_scan_snapshot.restype = ctypes.c_int
        lib.dbeel_gpu_reader_scan_snapshot.argtypes = (
            lib.dbeel_gpu_reader_scan_begin.argtypes[:-1]
            + [ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)])
        lib.dbeel_gpu_reader_scan_info.restype = ctypes.c_int
        lib.dbeel_gpu_reader_scan_info.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ScanSnapshotInfo)]
        lib.dbeel_gpu_reader_held_bytes.restype = ctypes.c_uint64
        lib.dbeel_gpu_reader_held_bytes.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_write_batch.restype = ctypes.c_int
        lib.dbeel_gpu_reader_write_batch.argtypes = (
            [ctypes.c_void_p, ctypes.c_size_t] + _BATCH_ARGTYPES + [
                ctypes.c_int, ctypes.POINTER(CompactResult),
                ctypes.POINTER(_U8P), _U64P,
                ctypes.POINTER(WriteBatchStats)])
        lib.dbeel_gpu_flush_batch.restype = ctypes.c_int
        lib.dbeel_gpu_flush_batch.argtypes = _BATCH_ARGTYPES + [
            ctypes.c_int, ctypes.POINTER(CompactResult)]
        lib.dbeel_gpu_reader_put.restype = ctypes.c_int
        lib.dbeel_gpu_reader_put.argtypes = (
            [ctypes.c_void_p] + _BATCH_ARGTYPES
            + [ctypes.POINTER(MemtablePutStats)])
        lib.dbeel_gpu_reader_memtable_info.restype = ctypes.c_int
        lib.dbeel_gpu_reader_memtable_info.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(MemtableInfo)]
        lib.dbeel_gpu_reader_memtable_fetch.restype = ctypes.c_int
        lib.dbeel_gpu_reader_memtable_fetch.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(CompactResult)]
        lib.dbeel_gpu_reader_memtable_flush.restype = ctypes.c_int
        lib.dbeel_gpu_reader_memtable_flush.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(CompactResult),
            ctypes.POINTER(_U8P), _U64P]
        lib.dbeel_gpu_reader_memtable_clear.restype = None
        lib.dbeel_gpu_reader_memtable_clear.argtypes = [ctypes.c_void_p]
        lib.dbeel_gpu_reader_get_entries.restype = ctypes.c_int
        lib.dbeel_gpu_reader_get_entries.argtypes = [
            ctypes.c_void_p, _U8P, _U64P, ctypes.c_uint64,
            ctypes.POINTER(GetBuffers), ctypes.POINTER(GetPage),
            ctypes.POINTER(GetStats)]
        lib.dbeel_gpu_reader_get_merged.restype = ctypes.c_int
        lib.dbeel_gpu_reader_get_merged.argtypes = [
            ctypes.c_void_p, _U8P, _U64P, ctypes.c_uint64,
            ctypes.POINTER(MergeSource), ctypes.c_size_t,
            ctypes.POINTER(MergeBuffers), ctypes.POINTER(GetPage),
            ctypes.POINTER(MergeStats)]
        lib.dbeel_gpu_reader_put_entries.restype = ctypes.c_int
        lib.dbeel_gpu_reader_put_entries.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
            ctypes.POINTER(PutEntriesStats)]
        lib.dbeel_gpu_reader_scan_apply.restype = ctypes.c_int
        lib.dbeel_gpu_reader_scan_apply.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ApplyAction), ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
            ctypes.POINTER(ScanPage), ctypes.POINTER(ScanApplyStats)]
        lib.dbeel_gpu_reader_compact_fetch.restype = ctypes.c_int
        lib.dbeel_gpu_reader_compact_fetch.argtypes = [
            ctypes.c_void_p, _U8P, ctypes.c_uint64, _U8P, ctypes.c_uint64,
            _U64P, _U64P, ctypes.POINTER(ctypes.c_double)]
        lib._reader_ready = True
    return lib


class ScanPage(ctypes.Structure):
    """dbeel_scan_page."""
    _fields_ = [
        ("data_len", ctypes.c_uint64),
        ("n_entries", ctypes.c_uint64),
        ("candidates", ctypes.c_uint64),
        ("needed", ctypes.c_uint64),
        ("done", ctypes.c_int),
        ("flag_ms", ctypes.c_double),
        ("emit_ms", ctypes.c_double),
        ("copy_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SCAN_MEMTABLE = 1      # DBEEL_SCAN_MEMTABLE
SCAN_NEWEST_ONLY = 2   # DBEEL_SCAN_NEWEST_ONLY


class ScanSnapshotInfo(ctypes.Structure):
    """dbeel_scan_snapshot_info."""
    _fields_ = [
        ("n_tables", ctypes.c_uint32),
        ("has_memtable", ctypes.c_uint32),
        ("table_candidates", ctypes.c_uint64),
        ("memtable_candidates", ctypes.c_uint64),
        ("shadowed", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReaderScan:
    """One open paged scan of a Reader (dbeel_gpu_reader_scan_*): next()
    fills caller-owned numpy buffers with the next page. Made by
    Reader.scan_open() or, with snapshot_flags (an int, 0 included), by
    Reader.snapshot_open(); ended by close(), or by closing the reader."""

    def __init__(self, reader: "Reader", start_key, end_key, hash_ranges,
                 max_candidates: int, snapshot_flags: int | None = None):
        if not reader._h:
            raise ValueError("reader is closed")
        self._reader = reader
        self._lib = reader._lib
        self._h = None

        def _kb(b):
            if b is None:
                return None, 0, None
            a = np.frombuffer(bytes(b) or b"\0", dtype=np.uint8)
            return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(b), a

        sp, sl, sa = _kb(start_key)
        ep, el, ea = _kb(end_key)
        self.n_ranges = len(hash_ranges) if hash_ranges else 0
        rsp = rep = None
        if self.n_ranges:
            rs = np.array([r[0] for r in hash_ranges], dtype=np.uint32)
            re_ = np.array([r[1] for r in hash_ranges], dtype=np.uint32)
            rsp = rs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
            rep = re_.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        h = ctypes.c_void_p()
        if snapshot_flags is None:
            rc = self._lib.dbeel_gpu_reader_scan_begin(
                reader._h, sp, sl, ep, el, rsp, rep, self.n_ranges,
                int(max_candidates), ctypes.byref(h))
        else:
            rc = self._lib.dbeel_gpu_reader_scan_snapshot(
                reader._h, sp, sl, ep, el, rsp, rep, self.n_ranges,
                int(max_candidates), int(snapshot_flags), ctypes.byref(h))
        del sa, ea  # begin has copied the bounds and ranges to the device
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        self._h = h
        reader._scans.append(self)

    def next(self, data: np.ndarray, index: np.ndarray, range_ids=None):
        """Fill data (u8) / index (u8, 16 B per record) / range_ids (u32,
        one slot per index record, or None) with the next page. Returns the
        dbeel_scan_page as a dict. A first entry larger than data raises
        DbeelGpuError with code 3 and .page["needed"] set; the scan stays
        where it was, so next() may be called again with a larger buffer."""
        if not self._h:
            raise ValueError("scan is closed")
        if range_ids is not None and range_ids.nbytes // 4 < index.nbytes // 16:
            raise ValueError("range_ids needs one slot per index record")
        pg = ScanPage()
        rc = self._lib.dbeel_gpu_reader_scan_next(
            self._h, data.ctypes.data, data.nbytes, index.ctypes.data,
            index.nbytes,
            None if range_ids is None else range_ids.ctypes.data,
            ctypes.byref(pg))
        if rc != 0:
            err = DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
            err.page = pg.as_dict()
            raise err
        return pg.as_dict()

    def apply(self, actions, page_bytes: int, page_entries=None,
              delete_ts=None):
        """Draws the next page as next() would into buffers of page_bytes
        and page_entries records (default: one per 32 page bytes, the
        smallest entry) and applies it on the device
        (dbeel_gpu_reader_scan_apply): actions[id] is ("skip",),
        ("put", reader) or ("delete", reader) for the entries whose first
        matching hash range is id — one action for a scan without ranges.
        delete_ts (int or 16 bytes) is the tombstones' timestamp. Returns
        (page dict, stats dict); errors as next(), with the cursor where it
        was."""
        if not self._h:
            raise ValueError("scan is closed")
        acts = (ApplyAction * max(len(actions), 1))()
        for i, a in enumerate(actions):
            acts[i].kind = _APPLY_KINDS.get(a[0], a[0])
            dst = a[1] if len(a) > 1 else None
            if dst is not None and not dst._h:
                raise ValueError("destination reader is closed")
            acts[i].dst = None if dst is None else dst._h
        if page_entries is None:
            page_entries = max(1, int(page_bytes) // 32)
        ts = _ts16(delete_ts)
        pg = ScanPage()
        st = ScanApplyStats()
        rc = self._lib.dbeel_gpu_reader_scan_apply(
            self._h, acts, len(actions),
            None if ts is None else ts.ctypes.data, int(page_bytes),
            int(page_entries), ctypes.byref(pg), ctypes.byref(st))
        if rc != 0:
            err = DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
            err.page = pg.as_dict()
            raise err
        return pg.as_dict(), st.as_dict()

    def info(self) -> dict:
        """dbeel_scan_snapshot_info as a dict: the snapshot's segments and
        candidates, and the entries NEWEST_ONLY has dropped so far."""
        if not self._h:
            raise ValueError("scan is closed")
        si = ScanSnapshotInfo()
        rc = self._lib.dbeel_gpu_reader_scan_info(self._h, ctypes.byref(si))
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        return si.as_dict()

    def close(self):
        if self._h:
            self._lib.dbeel_gpu_reader_scan_end(self._h)
            self._h = None
            self._reader._scans.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Reader:
    """Resident table reader (LSMTree::get over the sstables,
    lsm_tree.rs:674-723): runs [(data, index), ...] and their optional
    "DBLM" filters (blooms[r] = the .bloom file's bytes, or None) are
    uploaded once; every get() after that moves only keys in and hits +
    packed values out. No host copy of the runs is needed afterwards.

    The reader is live: insert_run() takes a flushed run, compact_begin()
    / compact_commit() compact runs it already holds in HBM and swap the
    list in one step (the reference's shared sstable list,
    lsm_tree.rs:901-915 and 1113-1145). Runs are named by position in the
    list, which is what hit["run"] reports."""

    def __init__(self, runs, blooms=None, device: int = 0):
        self._lib = _load_reader()
        self._h = None
        self._scans = []  # open ReaderScans; close() ends them
        views, keepalive = _views(runs)
        bviews = None
        if blooms is not None:
            if len(blooms) != len(runs):
                raise ValueError("blooms must be None or one per run")
            bviews = (BloomView * len(runs))()
            for i, b in enumerate(blooms):
                if b is None:
                    continue
                a = np.frombuffer(bytes(b) or b"\0", dtype=np.uint8)
                keepalive.append(a)
                bviews[i].bytes = a.ctypes.data_as(
                    ctypes.POINTER(ctypes.c_uint8))
                bviews[i].len = len(b)
        h = ctypes.c_void_p()
        rc = self._lib.dbeel_gpu_reader_open(
            views, bviews, len(runs), device, ctypes.byref(h)
        )
        del keepalive  # open has copied everything to the device
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        self._h = h

    @classmethod
    def _from_handle(cls, handle) -> "Reader":
        self = cls.__new__(cls)
        self._lib = _load_reader()
        self._h = handle
        self._scans = []
        return self

    @property
    def table_bytes(self) -> int:
        """Device bytes held between calls, summed over the tables: run
        bytes + prefixes + bitmaps."""
        return int(self._lib.dbeel_gpu_reader_table_bytes(self._h))

    @property
    def held_bytes(self) -> int:
        """Device bytes that left the list or the memtable's pair and live
        only because a snapshot scan still reads them, each buffer once."""
        return int(self._lib.dbeel_gpu_reader_held_bytes(self._h))

    @property
    def n_runs(self) -> int:
        return int(self._lib.dbeel_gpu_reader_run_count(self._h))

    def _check(self, rc):
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())

    def insert_run(self, pos: int, run, bloom=None):
        """Flush: upload one run (data, index) and its optional "DBLM"
        filter bytes, inserted at position pos in [0, n_runs]; runs at
        >= pos move up by one. On failure the reader is unchanged."""
        if not self._h:
            raise ValueError("reader is closed")
        views, keepalive = _views([run])
        bview = None
        if bloom is not None:
            a = np.frombuffer(bytes(bloom) or b"\0", dtype=np.uint8)
            keepalive.append(a)
            bview = BloomView(
                a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(bloom))
        self._check(self._lib.dbeel_gpu_reader_insert_run(
            self._h, pos, views, None if bview is None else ctypes.byref(bview)))
        del keepalive

    def write_batch(self, writes, pos: int | None = None,
                    build_bloom: bool = False, fetch: bool = True):
        """The memtable and its flush in one call: `writes` is an iterable
        of (key, value, timestamp) in ARRIVAL order — unsorted, keys may
        repeat, b"" is a tombstone. The batch is sorted, the last write of
        every key kept (whatever the timestamps), and the run encoded on
        the device straight into a new table at position pos (None = the
        end: gets see it first). Returns (data, index, bloom_bytes, stats):
        the run's file bytes (None, None when fetch=False), its "DBLM"
        filter bytes (None unless build_bloom and fetch) and the stats
        dict. An empty batch changes nothing. On failure the reader is
        unchanged."""
        if not self._h:
            raise ValueError("reader is closed")
        n, ptrs, keepalive = _write_arrays(writes)
        res = CompactResult()
        st = WriteBatchStats()
        bp = _U8P()
        bn = ctypes.c_uint64()
        want_bloom = bool(build_bloom) and fetch
        rc = self._lib.dbeel_gpu_reader_write_batch(
            self._h, self.n_runs if pos is None else pos, n, *ptrs,
            int(build_bloom), ctypes.byref(res) if fetch else None,
            ctypes.byref(bp) if want_bloom else None,
            ctypes.byref(bn) if want_bloom else None, ctypes.byref(st))
        del keepalive
        self._check(rc)
        data = index = bloom_bytes = None
        try:
            if fetch:
                data = _ptr_bytes(res.data, res.data_len)
                index = _ptr_bytes(res.index, res.index_len)
            if want_bloom and bp:
                bloom_bytes = _ptr_bytes(bp, int(bn.value))
        finally:
            if fetch:
                self._lib.dbeel_gpu_result_free(ctypes.byref(res))
            if want_bloom:
                self._lib.dbeel_gpu_bloom_free(bp)
        return data, index, bloom_bytes, st.as_dict()

    def put(self, writes):
        """Puts `writes` — (key, value, timestamp) in ARRIVAL order,
        unsorted, keys may repeat, b"" is a tombstone — into the reader's
        resident memtable: the last arrival of a key wins, across puts too,
        whatever the timestamps. Gets see the memtable before every table
        (hit["run"] == n_runs); scans do not. Returns the stats dict. An
        empty batch changes nothing; on failure the memtable is
        unchanged."""
        if not self._h:
            raise ValueError("reader is closed")
        n, ptrs, keepalive = _write_arrays(writes)
        st = MemtablePutStats()
        rc = self._lib.dbeel_gpu_reader_put(self._h, n, *ptrs,
                                            ctypes.byref(st))
        del keepalive
        self._check(rc)
        return st.as_dict()

    def put_entries(self, data, index, range_ids=None, take=None,
                    delete_ts=None):
        """Puts a page exactly as a paged scan yields it — numpy arrays
        data (u8), index (u8, 16 B per record) and optionally range_ids
        (u32, one per record) with take (u8, take[id] != 0 selects), passed
        through by pointer so pinned arrays work — into the memtable, in
        page order, under put()'s contract. With delete_ts (int or 16 bytes)
        every selected entry becomes a tombstone with that timestamp
        instead (dbeel_gpu_reader_put_entries). Returns the stats dict; on
        failure the memtable is unchanged."""
        if not self._h:
            raise ValueError("reader is closed")
        n = index.nbytes // 16
        if range_ids is not None and range_ids.nbytes // 4 < n:
            raise ValueError("range_ids needs one slot per index record")
        if take is not None:
            take = np.ascontiguousarray(take, dtype=np.uint8)
        ts = _ts16(delete_ts)
        st = PutEntriesStats()
        rc = self._lib.dbeel_gpu_reader_put_entries(
            self._h, data.ctypes.data, data.nbytes, index.ctypes.data, n,
            None if range_ids is None else range_ids.ctypes.data,
            None if take is None else take.ctypes.data,
            0 if take is None else take.size,
            APPLY_PUT if ts is None else APPLY_DELETE,
            None if ts is None else ts.ctypes.data, ctypes.byref(st))
        self._check(rc)
        return st.as_dict()

    def migrate(self, actions, start_key=None, end_key=None,
                hash_ranges=None, flags: int = SCAN_MEMTABLE,
                page_bytes: int = 64 << 20, delete_ts=None,
                max_candidates: int = 0):
        """The migration loop inside HBM: opens a snapshot scan with
        `flags` (SCAN_MEMTABLE | SCAN_NEWEST_ONLY), applies page after page
        with ReaderScan.apply(actions, ...) until done, and returns the
        summed stats: pages, entries, put_entries, delete_entries, skipped,
        groups, apply_ms and the pages' flag / emit / copy ms."""
        total = {"pages": 0, "entries": 0, "put_entries": 0,
                 "delete_entries": 0, "skipped": 0, "groups": 0,
                 "apply_ms": 0.0, "flag_ms": 0.0, "emit_ms": 0.0,
                 "copy_ms": 0.0}
        sc = ReaderScan(self, start_key, end_key, hash_ranges,
                        max_candidates, snapshot_flags=int(flags))
        try:
            while True:
                pg, st = sc.apply(actions, page_bytes, delete_ts=delete_ts)
                total["pages"] += 1
                total["entries"] += pg["n_entries"]
                for k in ("put_entries", "delete_entries", "skipped",
                          "groups", "apply_ms"):
                    total[k] += st[k]
                for k in ("flag_ms", "emit_ms", "copy_ms"):
                    total[k] += pg[k]
                if pg["done"]:
                    break
        finally:
            sc.close()
        return total

    @property
    def memtable_info(self) -> dict:
        """entries / data_bytes held, reserved_bytes of device storage (not
        part of table_bytes), puts since the last flush or clear."""
        if not self._h:
            raise ValueError("reader is closed")
        info = MemtableInfo()
        self._check(self._lib.dbeel_gpu_reader_memtable_info(
            self._h, ctypes.byref(info)))
        return info.as_dict()

    def memtable_fetch(self):
        """-> (data, index): the memtable's run bytes, what a flush would
        write; (b"", b"") when it is empty. Changes nothing."""
        if not self._h:
            raise ValueError("reader is closed")
        res = CompactResult()
        self._check(self._lib.dbeel_gpu_reader_memtable_fetch(
            self._h, ctypes.byref(res)))
        try:
            return (_ptr_bytes(res.data, res.data_len),
                    _ptr_bytes(res.index, res.index_len))
        finally:
            self._lib.dbeel_gpu_result_free(ctypes.byref(res))

    def memtable_flush(self, build_bloom: bool = False, fetch: bool = True):
        """The memtable becomes the newest table (position n_runs) and is
        empty afterwards. Returns (data, index, bloom_bytes): the run's file
        bytes (None, None when fetch=False) and its "DBLM" filter bytes
        (None unless build_bloom and fetch). An empty memtable flushes
        nothing: (b"", b"", None)."""
        if not self._h:
            raise ValueError("reader is closed")
        res = CompactResult()
        bp = _U8P()
        bn = ctypes.c_uint64()
        want_bloom = bool(build_bloom) and fetch
        rc = self._lib.dbeel_gpu_reader_memtable_flush(
            self._h, int(build_bloom), ctypes.byref(res) if fetch else None,
            ctypes.byref(bp) if want_bloom else None,
            ctypes.byref(bn) if want_bloom else None)
        self._check(rc)
        data = index = bloom_bytes = None
        try:
            if fetch:
                data = _ptr_bytes(res.data, res.data_len)
                index = _ptr_bytes(res.index, res.index_len)
            if want_bloom and bp:
                bloom_bytes = _ptr_bytes(bp, int(bn.value))
        finally:
            if fetch:
                self._lib.dbeel_gpu_result_free(ctypes.byref(res))
            if want_bloom:
                self._lib.dbeel_gpu_bloom_free(bp)
        return data, index, bloom_bytes

    def memtable_clear(self):
        """Drop the memtable's contents; its device storage is kept."""
        if self._h:
            self._lib.dbeel_gpu_reader_memtable_clear(self._h)

    def compact_begin(self, positions, keep_tombstones: bool,
                      bloom: bool = False, fetch: bool = True):
        """Compact the runs at `positions` (strictly ascending) where they
        lie in HBM. The output becomes a pending table: gets keep seeing
        the old list until compact_commit(). Returns (data, index,
        bloom_bytes, stats): the output run's file bytes (None, None when
        fetch=False), its "DBLM" filter bytes (None unless bloom) and the
        stats dict."""
        if not self._h:
            raise ValueError("reader is closed")
        positions = list(positions)
        pos = (ctypes.c_uint32 * max(1, len(positions)))(*positions)
        res = CompactResult()
        st = ReaderCompactStats()
        bp = ctypes.POINTER(ctypes.c_uint8)()
        bn = ctypes.c_uint64()
        want_bloom = bool(bloom) and fetch
        rc = self._lib.dbeel_gpu_reader_compact_begin(
            self._h, pos, len(positions), int(keep_tombstones), int(bloom),
            ctypes.byref(res) if fetch else None,
            ctypes.byref(bp) if want_bloom else None,
            ctypes.byref(bn) if want_bloom else None, ctypes.byref(st))
        self._check(rc)
        data = index = bloom_bytes = None
        try:
            if fetch:
                data = _ptr_bytes(res.data, res.data_len)
                index = _ptr_bytes(res.index, res.index_len)
            if want_bloom:
                bloom_bytes = _ptr_bytes(bp, int(bn.value))
        finally:
            if fetch:
                self._lib.dbeel_gpu_result_free(ctypes.byref(res))
            if want_bloom:
                self._lib.dbeel_gpu_bloom_free(bp)
        return data, index, bloom_bytes, st.as_dict()

    def compact_commit(self, out_pos: int):
        """Swap: remove the compacted runs, insert the pending output at
        out_pos in [0, n_runs - len(positions)]."""
        self._check(self._lib.dbeel_gpu_reader_compact_commit(self._h,
                                                              out_pos))

    def compact_abort(self):
        """Drop the pending output; the list is unchanged."""
        if self._h:
            self._lib.dbeel_gpu_reader_compact_abort(self._h)

    def compact(self, positions, out_pos: int, keep_tombstones: bool,
                bloom: bool = False, fetch: bool = True):
        """compact_begin followed by compact_commit."""
        out = self.compact_begin(positions, keep_tombstones, bloom=bloom,
                                 fetch=fetch)
        try:
            self.compact_commit(out_pos)
        except DbeelGpuError:
            self.compact_abort()
            raise
        return out

    def get_raw(self, keys):
        """-> (hits HIT_DTYPE array, value_offsets u64[n+1], values u8
        array packed in query order, stats dict)."""
        if not self._h:
            raise ValueError("reader is closed")
        ka, koff = _key_blob(keys)
        res = GetResult()
        st = GetStats()
        rc = self._lib.dbeel_gpu_reader_get(
            self._h,
            ka.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            len(keys), ctypes.byref(res), ctypes.byref(st),
        )
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        try:
            n = int(res.n_keys)
            hits = np.empty(n, dtype=HIT_DTYPE)
            if n:
                ctypes.memmove(hits.ctypes.data, res.hits,
                               n * HIT_DTYPE.itemsize)
            voff = np.ctypeslib.as_array(res.value_offsets,
                                         shape=(n + 1,)).copy()
            nv = int(res.values_len)
            values = (np.ctypeslib.as_array(res.values, shape=(nv,)).copy()
                      if nv else np.zeros(0, dtype=np.uint8))
        finally:
            self._lib.dbeel_gpu_get_result_free(ctypes.byref(res))
        return hits, voff, values, st.as_dict()

    def get(self, keys):
        """lookup()'s convention: value bytes, b"" for a deleted key
        (tombstone), None if absent."""
        hits, voff, values, _ = self.get_raw(keys)
        blob = values.tobytes()
        off = voff.tolist()
        return [None if r < 0 else blob[off[q] : off[q + 1]]
                for q, r in enumerate(hits["run"].tolist())]

    def _get_entries_into(self, ka, koff, hits, roff, records, cap):
        """dbeel_gpu_reader_get_entries over the key blob ka / offsets koff
        (len(koff) - 1 keys) into the caller's arrays: hits (HIT_DTYPE, n),
        roff (u64, n + 1), records (u8, at least cap bytes, or None with
        cap 0). -> (rc, GetPage, GetStats); nothing is raised."""
        if not self._h:
            raise ValueError("reader is closed")
        n = len(koff) - 1
        buf = GetBuffers(
            hits.ctypes.data_as(ctypes.POINTER(LookupHit)),
            roff.ctypes.data_as(_U64P),
            None if records is None else records.ctypes.data_as(_U8P),
            cap)
        page = GetPage()
        st = GetStats()
        rc = self._lib.dbeel_gpu_reader_get_entries(
            self._h, ka.ctypes.data_as(_U8P), koff.ctypes.data_as(_U64P), n,
            ctypes.byref(buf), ctypes.byref(page), ctypes.byref(st))
        return rc, page, st

    @staticmethod
    def _records_arg(records, records_cap):
        """The records / records_cap arguments of get_entries_raw and
        get_merged_raw -> (u8 array, cap)."""
        if records is None:
            cap = (64 << 20) if records_cap is None else int(records_cap)
            return np.empty(max(cap, 1), dtype=np.uint8), cap
        if (records.dtype != np.uint8 or records.ndim != 1
                or not records.flags.c_contiguous):
            raise ValueError("records must be a contiguous 1-D uint8 array")
        cap = records.size if records_cap is None else int(records_cap)
        if cap > records.size:
            raise ValueError("records_cap exceeds the records array")
        return records, cap

    def get_entries_raw(self, keys, records=None, records_cap=None):
        """get_entry for a batch, with timestamps: -> (hits HIT_DTYPE array,
        record_offsets u64[n+1], records view, page dict, stats dict). The
        record of a found key — a tombstone included — is the stored
        `data_len:u64 | data | timestamp:i128`, 24 + value_len bytes, the
        bincode form of EntryValue; an absent key has an empty range.
        record_offsets covers ALL keys; the records of the first
        page["n_done"] keys are in the view (records[:page["records_len"]]);
        call again with keys[n_done:] for the rest.

        records is a caller np.uint8 array (pin_host it for true async DMA),
        of which records_cap bytes (default: all) may be written; when it is
        omitted one of records_cap bytes (default 64 MiB) is allocated. If
        the first record alone is over the cap, DbeelGpuError
        (ITEM_TOO_LARGE) is raised carrying .page (needed = its size), .hits
        and .record_offsets, which are complete."""
        ka, koff = _key_blob(keys)
        n = len(keys)
        records, cap = self._records_arg(records, records_cap)
        hits = np.empty(n, dtype=HIT_DTYPE)
        roff = np.zeros(n + 1, dtype=np.uint64)
        rc, page, st = self._get_entries_into(ka, koff, hits, roff, records,
                                              cap)
        if rc != 0:
            err = DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
            err.page, err.hits, err.record_offsets = page.as_dict(), hits, roff
            raise err
        return (hits, roff, records[:int(page.records_len)], page.as_dict(),
                st.as_dict())

    def get_entries(self, keys, page_bytes: int = 64 << 20):
        """LSMTree::get_entry for a batch: a list of None (absent) or
        (data: bytes, timestamp: int), a deleted key being (b"", ts) — what
        a replicated read compares timestamps on before it tests for the
        tombstone. Pages of page_bytes are drawn until every key is
        answered; a record larger than the page grows the buffer to its
        size, once."""
        keys = list(keys)
        records = np.empty(max(int(page_bytes), 1), dtype=np.uint8)
        cap = int(page_bytes)
        out = []
        grown = False
        while len(out) < len(keys):
            try:
                hits, roff, view, page, _ = self.get_entries_raw(
                    keys[len(out):], records=records, records_cap=cap)
            except DbeelGpuError as e:
                if e.code != 3 or grown:
                    raise
                cap = int(e.page["needed"])
                records = np.empty(cap, dtype=np.uint8)
                grown = True
                continue
            grown = False
            blob = view.tobytes()
            off = roff.tolist()
            for q, r in enumerate(hits["run"][:page["n_done"]].tolist()):
                if r < 0:
                    out.append(None)
                    continue
                rec = blob[off[q]:off[q + 1]]
                out.append((rec[8:-16],
                            int.from_bytes(rec[-16:], "little", signed=True)))
        return out

    @staticmethod
    def _merge_sources(sources):
        """sources — each a Reader or a (record_offsets, records) pair as
        get_entries_raw returns them — as a dbeel_merge_source array:
        -> (array or None, keepalive)."""
        sources = list(sources)
        if not sources:
            return None, []
        arr = (MergeSource * len(sources))()
        keep = []
        for i, s in enumerate(sources):
            if isinstance(s, Reader):
                if not s._h:
                    raise ValueError("source reader is closed")
                arr[i].kind = MERGE_READER
                arr[i].reader = s._h
                keep.append(s)
                continue
            off, rec = s
            off = np.ascontiguousarray(off, dtype=np.uint64)
            if rec is None:  # legal when the answer holds no record bytes
                rec = np.zeros(0, dtype=np.uint8)
            rec = (np.frombuffer(rec, dtype=np.uint8)
                   if isinstance(rec, (bytes, bytearray))
                   else np.ascontiguousarray(rec, dtype=np.uint8))
            arr[i].kind = MERGE_ANSWERS
            arr[i].record_offsets = off.ctypes.data_as(_U64P)
            if rec.size:
                arr[i].records = rec.ctypes.data_as(_U8P)
            keep += [off, rec]
        return arr, keep

    def _get_merged_into(self, ka, koff, srcs, n_sources, hits, roff,
                         records, cap):
        """dbeel_gpu_reader_get_merged over the key blob ka / offsets koff
        and the dbeel_merge_source array srcs into the caller's arrays: hits
        (MERGE_HIT_DTYPE, n), roff (u64, n + 1), records (u8, at least cap
        bytes, or None with cap 0). -> (rc, GetPage, MergeStats); nothing is
        raised."""
        if not self._h:
            raise ValueError("reader is closed")
        n = len(koff) - 1
        buf = MergeBuffers(
            hits.ctypes.data_as(ctypes.POINTER(MergeHit)),
            roff.ctypes.data_as(_U64P),
            None if records is None else records.ctypes.data_as(_U8P),
            cap)
        page = GetPage()
        st = MergeStats()
        rc = self._lib.dbeel_gpu_reader_get_merged(
            self._h, ka.ctypes.data_as(_U8P), koff.ctypes.data_as(_U64P), n,
            srcs, n_sources, ctypes.byref(buf), ctypes.byref(page),
            ctypes.byref(st))
        return rc, page, st

    def get_merged_raw(self, keys, sources, records=None, records_cap=None):
        """The replicated read's pick for a batch (tasks/db_server.rs:
        338-363): -> (hits MERGE_HIT_DTYPE array, record_offsets u64[n+1],
        records view, page dict, stats dict). The candidates of a key are
        the sources' answers in order and this reader's own LAST; the winner
        has the greatest timestamp, the highest index among equals. A source
        is a Reader on the same device or a (record_offsets, records) pair
        as get_entries_raw returns them for the same keys. hits["source"]
        names the winner (len(sources) = this reader, -1 = nobody holds the
        key), hits["stale_mask"] the candidates that are absent or older.
        Records, buffers, paging and the error protocol are
        get_entries_raw's; for the next page the caller advances the keys
        and every pair (offsets rebased to 0)."""
        ka, koff = _key_blob(keys)
        n = len(keys)
        records, cap = self._records_arg(records, records_cap)
        srcs, keep = self._merge_sources(sources)
        hits = np.empty(n, dtype=MERGE_HIT_DTYPE)
        roff = np.zeros(n + 1, dtype=np.uint64)
        rc, page, st = self._get_merged_into(
            ka, koff, srcs, len(srcs) if srcs is not None else 0, hits, roff,
            records, cap)
        del keep
        if rc != 0:
            err = DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
            err.page, err.hits, err.record_offsets = page.as_dict(), hits, roff
            raise err
        return (hits, roff, records[:int(page.records_len)], page.as_dict(),
                st.as_dict())

    def get_merged(self, keys, sources, page_bytes: int = 64 << 20):
        """The newest answer across replicas for a batch: a list of None
        (no candidate holds the key) or (data: bytes, timestamp: int,
        source: int), a winning tombstone being (b"", ts, source). Pages
        like get_entries; the (record_offsets, records) sources are sliced
        per page."""
        keys = list(keys)
        sources = [s if isinstance(s, Reader)
                   else (np.ascontiguousarray(s[0], dtype=np.uint64),
                         np.frombuffer(s[1], dtype=np.uint8)
                         if isinstance(s[1], (bytes, bytearray))
                         else np.ascontiguousarray(s[1], dtype=np.uint8))
                   for s in sources]
        records = np.empty(max(int(page_bytes), 1), dtype=np.uint8)
        cap = int(page_bytes)
        out = []
        grown = False
        while len(out) < len(keys):
            p = len(out)
            page_src = [s if isinstance(s, Reader)
                        else (s[0][p:] - s[0][p],
                              s[1][int(s[0][p]):int(s[0][-1])])
                        for s in sources]
            try:
                hits, roff, view, page, _ = self.get_merged_raw(
                    keys[p:], page_src, records=records, records_cap=cap)
            except DbeelGpuError as e:
                if e.code != 3 or grown:
                    raise
                cap = int(e.page["needed"])
                records = np.empty(cap, dtype=np.uint8)
                grown = True
                continue
            grown = False
            blob = view.tobytes()
            off = roff.tolist()
            for q, s in enumerate(hits["source"][:page["n_done"]].tolist()):
                if s < 0:
                    out.append(None)
                    continue
                rec = blob[off[q]:off[q + 1]]
                out.append((rec[8:-16],
                            int.from_bytes(rec[-16:], "little", signed=True),
                            s))
        return out

    def get_replicated(self, keys, sources, page_bytes: int = 64 << 20):
        """The client-facing answer of a replicated get (db_server.rs:
        355-363): the newest candidate's data, or None when nobody holds the
        key or the newest answer is a tombstone."""
        return [None if m is None or not m[0] else m[0]
                for m in self.get_merged(keys, sources, page_bytes)]

    def compact_fetch_into(self, data_arr, index_arr):
        """Copy the PENDING compaction output's .data / .index bytes — what
        compact_begin(fetch=True) returns — into the caller's np.uint8
        arrays (pin_host them for true async DMA): -> (data_len, index_len,
        d2h_ms). Use after compact_begin(fetch=False); callable any number
        of times until commit / abort. An array too small raises
        DbeelGpuError (ITEM_TOO_LARGE) carrying .data_len / .index_len, the
        sizes needed; nothing is written and the pending table is kept."""
        if not self._h:
            raise ValueError("reader is closed")
        for a in (data_arr, index_arr):
            if (a.dtype != np.uint8 or a.ndim != 1
                    or not a.flags.c_contiguous):
                raise ValueError("buffers must be contiguous 1-D uint8 "
                                 "arrays")
        dl, il = ctypes.c_uint64(), ctypes.c_uint64()
        ms = ctypes.c_double()
        rc = self._lib.dbeel_gpu_reader_compact_fetch(
            self._h, data_arr.ctypes.data_as(_U8P), data_arr.size,
            index_arr.ctypes.data_as(_U8P), index_arr.size,
            ctypes.byref(dl), ctypes.byref(il), ctypes.byref(ms))
        if rc != 0:
            err = DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
            err.data_len, err.index_len = int(dl.value), int(il.value)
            raise err
        return int(dl.value), int(il.value), float(ms.value)

    def scan_open(self, start_key=None, end_key=None, hash_ranges=None,
                  max_candidates: int = 0) -> ReaderScan:
        """Begin a paged scan (engine.scan's filters) over the runs held;
        see ReaderScan.next."""
        return ReaderScan(self, start_key, end_key, hash_ranges,
                          max_candidates)

    def snapshot_open(self, start_key=None, end_key=None, hash_ranges=None,
                      max_candidates: int = 0, memtable: bool = False,
                      newest_only: bool = False) -> ReaderScan:
        """Begin a snapshot scan (dbeel_gpu_reader_scan_snapshot): nothing
        done to the reader afterwards changes what it yields or makes it
        stale. memtable=True appends the memtable of this moment as the last
        segment; newest_only=True drops every entry whose key a later
        segment of the snapshot holds. .info() reports its segments."""
        flags = ((SCAN_MEMTABLE if memtable else 0)
                 | (SCAN_NEWEST_ONLY if newest_only else 0))
        return ReaderScan(self, start_key, end_key, hash_ranges,
                          max_candidates, snapshot_flags=flags)

    def snapshot_pages(self, start_key=None, end_key=None, hash_ranges=None,
                       page_bytes: int = 64 << 20,
                       page_entries: int = 1 << 20, max_candidates: int = 0,
                       pinned: bool = False, memtable: bool = False,
                       newest_only: bool = False):
        """scan_pages over a snapshot scan (see snapshot_open)."""
        return self._pages(
            lambda: self.snapshot_open(start_key, end_key, hash_ranges,
                                       max_candidates, memtable, newest_only),
            bool(hash_ranges), page_bytes, page_entries, pinned)

    def snapshot(self, start_key=None, end_key=None, hash_ranges=None,
                 page_bytes: int = 64 << 20, page_entries: int = 1 << 20,
                 max_candidates: int = 0, pinned: bool = False,
                 return_range_ids: bool = False, memtable: bool = False,
                 newest_only: bool = False):
        """scan over a snapshot scan (see snapshot_open)."""
        return self._joined(
            self.snapshot_pages(start_key, end_key, hash_ranges, page_bytes,
                                page_entries, max_candidates, pinned,
                                memtable, newest_only), return_range_ids)

    def scan_pages(self, start_key=None, end_key=None, hash_ranges=None,
                   page_bytes: int = 64 << 20, page_entries: int = 1 << 20,
                   max_candidates: int = 0, pinned: bool = False):
        """Paged migration scan over the resident runs: a generator of
        (data, index, n, range_ids) numpy VIEWS of one reused pair of
        buffers (copy what must outlive the next page). Every page is
        shaped like a run file — index offsets start at 0 — and holds at
        most page_bytes of entries and page_entries records; pages may be
        short or empty. range_ids[p] is the first hash range matching entry
        p (None without hash_ranges). Filters and yield order are
        engine.scan's; the pages concatenated are its result. pinned=True
        page-locks the buffers for the scan's lifetime. An entry larger
        than page_bytes raises DbeelGpuError (code 3, .page["needed"])."""
        return self._pages(
            lambda: self.scan_open(start_key, end_key, hash_ranges,
                                   max_candidates),
            bool(hash_ranges), page_bytes, page_entries, pinned)

    def _pages(self, opener, ranged: bool, page_bytes: int,
               page_entries: int, pinned: bool):
        """The page loop of scan_pages / snapshot_pages over opener()'s
        scan."""
        data = np.empty(page_bytes, dtype=np.uint8)
        index = np.empty(page_entries * 16, dtype=np.uint8)
        rid = np.empty(page_entries, dtype=np.uint32) if ranged else None
        bufs = [b for b in (data, index, rid) if b is not None]
        done_pin = []
        sc = None
        try:
            if pinned:
                for b in bufs:
                    pin_host(b)
                    done_pin.append(b)
            sc = opener()
            while True:
                pg = sc.next(data, index, rid)
                n = pg["n_entries"]
                yield (data[:pg["data_len"]], index[:n * 16], n,
                       None if rid is None else rid[:n])
                if pg["done"]:
                    break
        finally:
            if sc is not None:
                sc.close()
            for b in done_pin:
                unpin_host(b)

    def scan(self, start_key=None, end_key=None, hash_ranges=None,
             page_bytes: int = 64 << 20, page_entries: int = 1 << 20,
             max_candidates: int = 0, pinned: bool = False,
             return_range_ids: bool = False):
        """engine.scan over the resident runs: (data_bytes, index_bytes, n)
        with the pages' index offsets rebased into one run file; with
        return_range_ids also the u32 array of first matching ranges."""
        return self._joined(
            self.scan_pages(start_key, end_key, hash_ranges, page_bytes,
                            page_entries, max_candidates, pinned),
            return_range_ids)

    @staticmethod
    def _joined(pages, return_range_ids: bool):
        """Concatenates pages into one run file (offsets rebased)."""
        datas, indexes, rids = [], [], []
        off = 0
        total = 0
        for d, x, n, rid in pages:
            if not n:
                continue
            rec = x.view(INDEX_DTYPE).copy()
            rec["offset"] += off
            indexes.append(rec.tobytes())
            datas.append(d.tobytes())
            if rid is not None:
                rids.append(rid.copy())
            off += len(d)
            total += n
        out = (b"".join(datas), b"".join(indexes), total)
        if return_range_ids:
            ids = (np.concatenate(rids) if rids
                   else np.zeros(0, dtype=np.uint32))
            return out + (ids,)
        return out

    def close(self):
        if getattr(self, "_h", None):
            # reader_close ends the scans still open: drop their handles
            for sc in self._scans:
                sc._h = None
            self._scans = []
            self._lib.dbeel_gpu_reader_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_run(entries, device: int = 0):
    """GPU run encoder (the memtable-flush path, lsm_tree.rs:925-946):
    entries = iterable of (key: bytes, data: bytes, timestamp: int),
    ALREADY sorted ascending by key (memtable order). Returns
    (data_bytes, index_bytes, n)."""
    lib = load()
    keys = b"".join(e[0] for e in entries)
    vals = b"".join(e[1] for e in entries)
    n = len(entries)
    koff = np.zeros(n + 1, dtype=np.uint64)
    voff = np.zeros(n + 1, dtype=np.uint64)
    ts = np.zeros(16 * n, dtype=np.uint8)
    for i, (k, v, t) in enumerate(entries):
        koff[i + 1] = koff[i] + len(k)
        voff[i + 1] = voff[i] + len(v)
        ts[16 * i : 16 * (i + 1)] = np.frombuffer(
            int(t).to_bytes(16, "little", signed=True), dtype=np.uint8
        )
    ka = np.frombuffer(keys or b"\0", dtype=np.uint8)
    va = np.frombuffer(vals or b"\0", dtype=np.uint8)
    res = CompactResult()
    rc = lib.dbeel_gpu_encode_run(
        n,
        ka.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        va.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        voff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        ts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        device, ctypes.byref(res),
    )
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    try:
        data = _ptr_bytes(res.data, res.data_len)
        index = _ptr_bytes(res.index, res.index_len)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    return data, index, n


def flush_batch(writes, device: int = 0):
    """Reader.write_batch's run with no reader: writes = iterable of (key,
    value, timestamp) in arrival order, unsorted, keys may repeat. Returns
    (data_bytes, index_bytes, n) — what encode_run gives for the batch
    sorted by key with the last write of every key kept."""
    lib = _load_reader()
    n, ptrs, keepalive = _write_arrays(writes)
    res = CompactResult()
    rc = lib.dbeel_gpu_flush_batch(n, *ptrs, device, ctypes.byref(res))
    del keepalive
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    try:
        data = _ptr_bytes(res.data, res.data_len)
        index = _ptr_bytes(res.index, res.index_len)
        n_out = int(res.entries_written)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    return data, index, n_out


class Job:
    """Resident compaction job: inputs uploaded once, repeated runs timed
    with inputs already in HBM (the BASELINE measurement mode)."""

    def __init__(self, runs, device: int = 0):
        self._lib = load()
        views, self._keepalive = _views(runs)
        h = ctypes.c_void_p()
        rc = self._lib.dbeel_gpu_job_create(
            views, len(runs), device, ctypes.byref(h)
        )
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        self._h = h
        self.input_bytes = sum(v.data_len + v.index_len for v in views)

    def run(self, keep_tombstones: bool):
        dl = ctypes.c_uint64()
        ne = ctypes.c_uint64()
        tim = CompactTimings()
        rc = self._lib.dbeel_gpu_job_run(
            self._h, int(keep_tombstones), ctypes.byref(dl), ctypes.byref(ne),
            ctypes.byref(tim),
        )
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        return int(dl.value), int(ne.value), tim.as_dict()

    def ingest(self, runs):
        """Streamed pinned ingest (north_star): re-upload fresh run
        contents into this job's resident slab, chunked hipMemcpyAsync on
        a copy stream overlapped with the prepare kernel on the compute
        stream. Shapes must match the job's. The next run() skips the
        prepare stage (already done, hidden behind the transfer).
        Returns the ingest stats dict."""
        views, keepalive = _views(runs)
        st = IngestStats()
        rc = self._lib.dbeel_gpu_job_ingest(
            self._h, views, len(views), ctypes.byref(st)
        )
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        del keepalive
        return st.as_dict()

    def fetch(self):
        res = CompactResult()
        rc = self._lib.dbeel_gpu_job_fetch(self._h, ctypes.byref(res))
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        try:
            data = _ptr_bytes(res.data, res.data_len)
            index = _ptr_bytes(res.index, res.index_len)
            n = int(res.entries_written)
        finally:
            self._lib.dbeel_gpu_result_free(ctypes.byref(res))
        return data, index, n

    def fetch_into(self, data_arr: np.ndarray, index_arr: np.ndarray,
                   index_base: int = 0):
        """fetch() into the caller's numpy u8 arrays (by pointer: pinned
        arrays receive true async DMA), every index record's offset leaving
        with index_base added on the device; the job's own result is not
        changed by it. Returns (data_len, index_len, d2h_ms). Arrays too
        small raise DbeelGpuError with code 3 and .needed = (data_len,
        index_len), and nothing is written."""
        lib = _load_into(self._lib)
        dl = ctypes.c_uint64()
        il = ctypes.c_uint64()
        ms = ctypes.c_double()
        rc = lib.dbeel_gpu_job_fetch_into(
            self._h, data_arr.ctypes.data, data_arr.nbytes,
            index_arr.ctypes.data, index_arr.nbytes, int(index_base),
            ctypes.byref(dl), ctypes.byref(il), ctypes.byref(ms))
        if rc != 0:
            err = DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
            err.needed = (int(dl.value), int(il.value))
            raise err
        return int(dl.value), int(il.value), float(ms.value)

    def bloom(self) -> bytes:
        """The "DBLM" filter over the last run()'s surviving keys, built
        on the device (the .bloom file's bytes, include/dbeel_lsm.h)."""
        lib = self._lib
        if not hasattr(lib, "_bloom_ready"):
            lib.dbeel_gpu_job_bloom.restype = ctypes.c_int
            lib.dbeel_gpu_job_bloom.argtypes = [
                ctypes.c_void_p,
                ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                ctypes.POINTER(ctypes.c_uint64),
            ]
            lib.dbeel_gpu_bloom_free.restype = None
            lib.dbeel_gpu_bloom_free.argtypes = [
                ctypes.POINTER(ctypes.c_uint8)]
            lib._bloom_ready = True
        p = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        rc = lib.dbeel_gpu_job_bloom(self._h, ctypes.byref(p),
                                     ctypes.byref(n))
        if rc != 0:
            raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
        try:
            return _ptr_bytes(p, int(n.value))
        finally:
            lib.dbeel_gpu_bloom_free(p)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dbeel_gpu_job_destroy(self._h)
            self._h = None
            self._keepalive = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchJob(Job):
    """Batched INDEPENDENT jobs in one launch set (one dbeel shard each,
    BASELINE configs[3]): jobs = [runs, runs, ...]. run() executes every
    job's merge in one kernel pipeline; fetch_job(j) returns job j's
    (data, index, n) with offsets rebased to its own run file."""

    def __init__(self, jobs, device: int = 0):
        self._lib = load()
        if not hasattr(self._lib, "_batch_ready"):
            self._lib.dbeel_gpu_job_create_batched.restype = ctypes.c_int
            self._lib.dbeel_gpu_job_create_batched.argtypes = [
                ctypes.POINTER(RunView), ctypes.c_size_t,
                ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
            ]
            self._lib.dbeel_gpu_job_fetch_job.restype = ctypes.c_int
            self._lib.dbeel_gpu_job_fetch_job.argtypes = [
                ctypes.c_void_p, ctypes.c_size_t,
                ctypes.POINTER(CompactResult),
            ]
            self._lib._batch_ready = True
        flat = [rv for runs in jobs for rv in runs]
        views, self._keepalive = _views(flat)
        rpj = (ctypes.c_uint32 * len(jobs))(*[len(r) for r in jobs])
        h = ctypes.c_void_p()
        rc = self._lib.dbeel_gpu_job_create_batched(
            views, len(flat), rpj, len(jobs), device, ctypes.byref(h)
        )
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        self._h = h
        self.n_jobs = len(jobs)
        self.input_bytes = sum(v.data_len + v.index_len for v in views)

    def fetch_job(self, j: int):
        res = CompactResult()
        rc = self._lib.dbeel_gpu_job_fetch_job(self._h, j,
                                               ctypes.byref(res))
        if rc != 0:
            raise DbeelGpuError(rc, self._lib.dbeel_gpu_last_error().decode())
        try:
            data = _ptr_bytes(res.data, res.data_len)
            index = _ptr_bytes(res.index, res.index_len)
            n = int(res.entries_written)
        finally:
            self._lib.dbeel_gpu_result_free(ctypes.byref(res))
        return data, index, n

