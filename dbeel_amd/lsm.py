"""ctypes bindings for the file-level host layer (include/dbeel_lsm.h):
compact-with-journal, crash-recovery replay, the compaction trigger
policy, and the behavioral bloom check."""
from __future__ import annotations

import ctypes
import os

from .engine import DbeelGpuError, load as _load_gpu

_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        lib = _load_gpu()  # same .so
        lib.dbeel_lsm_compact.restype = ctypes.c_int
        lib.dbeel_lsm_compact.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
            ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_uint64),
        ]
        lib.dbeel_lsm_replay.restype = ctypes.c_int
        lib.dbeel_lsm_replay.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.dbeel_lsm_compact_tree.restype = ctypes.c_int
        lib.dbeel_lsm_compact_tree.argtypes = [
            ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_uint32),
        ]
        lib.dbeel_bloom_contains.restype = ctypes.c_int
        lib.dbeel_bloom_contains.argtypes = [
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_int),
        ]
        _lib = lib
    return _lib


def _check(rc, lib):
    if rc != 0:
        raise DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


DEFAULT_BLOOM_MIN_SIZE = 1_048_576  # mod.rs:19


def compact(dir: str, indices, output_index: int, keep_tombstones: bool,
            device: int = 0,
            bloom_min_size: int = DEFAULT_BLOOM_MIN_SIZE) -> int:
    lib = load()
    arr = (ctypes.c_uint64 * len(indices))(*indices)
    out = ctypes.c_uint64()
    rc = lib.dbeel_lsm_compact(
        dir.encode(), arr, len(indices), output_index,
        int(keep_tombstones), device, bloom_min_size, ctypes.byref(out),
    )
    _check(rc, lib)
    return int(out.value)


def compact_stream(dir: str, indices, output_index: int,
                   keep_tombstones: bool, device: int = 0,
                   max_resident_bytes: int = 0,
                   bloom_min_size: int = DEFAULT_BLOOM_MIN_SIZE) -> int:
    """compact() for inputs of any size (dbeel_lsm_compact_stream): pinned
    buffers, pipelined key slices of at most max_resident_bytes of input
    (0 = from free device memory), the filter built across slices. Leaves
    the directory byte-identical to compact()'s."""
    lib = load()
    if not hasattr(lib, "_lsm_stream_ready"):
        lib.dbeel_lsm_compact_stream.restype = ctypes.c_int
        lib.dbeel_lsm_compact_stream.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
            ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
            ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
        ]
        lib._lsm_stream_ready = True
    arr = (ctypes.c_uint64 * len(indices))(*indices)
    out = ctypes.c_uint64()
    rc = lib.dbeel_lsm_compact_stream(
        dir.encode(), arr, len(indices), output_index, int(keep_tombstones),
        device, int(max_resident_bytes), bloom_min_size, ctypes.byref(out),
    )
    _check(rc, lib)
    return int(out.value)


def replay(dir: str) -> int:
    lib = load()
    n = ctypes.c_uint32()
    rc = lib.dbeel_lsm_replay(dir.encode(), ctypes.byref(n))
    _check(rc, lib)
    return int(n.value)


def compact_tree(dir: str, compaction_factor: int = 2, device: int = 0,
                 bloom_min_size: int = DEFAULT_BLOOM_MIN_SIZE) -> int:
    lib = load()
    n = ctypes.c_uint32()
    rc = lib.dbeel_lsm_compact_tree(
        dir.encode(), compaction_factor, device, bloom_min_size,
        ctypes.byref(n),
    )
    _check(rc, lib)
    return int(n.value)


def major_compact(dir: str, device: int = 0,
                  bloom_min_size: int = DEFAULT_BLOOM_MIN_SIZE) -> int:
    """Merge EVERY live sstable into one run, dropping tombstones (safe:
    the group covers everything). Bounds tombstone buildup under the
    conservative full-coverage rule (include/dbeel_lsm.h)."""
    lib = load()
    if not hasattr(lib, "_major_ready"):
        lib.dbeel_lsm_major_compact.restype = ctypes.c_int
        lib.dbeel_lsm_major_compact.argtypes = [
            ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_uint64),
        ]
        lib._major_ready = True
    n = ctypes.c_uint64()
    rc = lib.dbeel_lsm_major_compact(dir.encode(), device, bloom_min_size,
                                     ctypes.byref(n))
    _check(rc, lib)
    return int(n.value)


def bloom_contains(bloom_bytes: bytes, key: bytes) -> bool:
    lib = load()
    bb = (ctypes.c_uint8 * len(bloom_bytes)).from_buffer_copy(bloom_bytes)
    kb = (ctypes.c_uint8 * max(len(key), 1)).from_buffer_copy(key or b"\0")
    out = ctypes.c_int()
    rc = lib.dbeel_bloom_contains(bb, len(bloom_bytes), kb, len(key),
                                  ctypes.byref(out))
    _check(rc, lib)
    return bool(out.value)


def open_reader(dir: str, device: int = 0):
    """Open a resident engine.Reader over every live sstable in dir (with
    its .bloom where one exists). Returns (reader, indices): indices[r] is
    the sstable index behind hit run r, ascending. Refuses a directory
    with a pending .compact_action journal (IO: replay first) or more
    than 64 sstables (INVALID_ARG: compact first); never mutates it."""
    from .engine import Reader

    lib = load()
    if not hasattr(lib, "_lsm_reader_ready"):
        lib.dbeel_lsm_reader_open.restype = ctypes.c_int
        lib.dbeel_lsm_reader_open.argtypes = [
            ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t),
        ]
        lib._lsm_reader_ready = True
    h = ctypes.c_void_p()
    idx = (ctypes.c_uint64 * 64)()
    n = ctypes.c_size_t()
    rc = lib.dbeel_lsm_reader_open(dir.encode(), device, ctypes.byref(h),
                                   idx, ctypes.byref(n))
    _check(rc, lib)
    return Reader._from_handle(h), [int(idx[i]) for i in range(n.value)]


def _load_live(lib):
    if not hasattr(lib, "_lsm_live_ready"):
        lib.dbeel_lsm_reader_add.restype = ctypes.c_int
        lib.dbeel_lsm_reader_add.argtypes = [
            ctypes.c_char_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t),
            ctypes.c_uint64,
        ]
        lib.dbeel_lsm_reader_compact.restype = ctypes.c_int
        lib.dbeel_lsm_reader_compact.argtypes = [
            ctypes.c_char_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t),
            ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
            ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_uint64),
        ]
        lib._lsm_live_ready = True
    return lib


def _indices_array(indices):
    if len(indices) > 64:
        raise ValueError("a reader holds at most 64 sstables")
    return ((ctypes.c_uint64 * 64)(*indices),
            ctypes.c_size_t(len(indices)))


def reader_add(dir: str, reader, indices, sstable_index: int):
    """A flush wrote sstable_index: read its files and insert the run into
    the open reader at its ascending-index position. Returns the new
    indices list; the reader then answers as a fresh open_reader(dir)
    would."""
    lib = _load_live(load())
    idx, n = _indices_array(indices)
    rc = lib.dbeel_lsm_reader_add(dir.encode(), reader._h, idx,
                                  ctypes.byref(n), sstable_index)
    _check(rc, lib)
    return [int(idx[i]) for i in range(n.value)]


def reader_flush(dir: str, reader, indices, sstable_index: int, writes):
    """The flush itself: `writes` — an iterable of (key, value, timestamp)
    in arrival order, unsorted, keys may repeat — is sorted, deduplicated
    (last write wins) and encoded on the device into a new table of the
    open reader at sstable_index's ascending-index position, and written
    as {sstable_index:020}.data/.index (no .bloom). Returns the new
    indices list; the reader then answers as a fresh open_reader(dir)
    would. An empty batch writes nothing."""
    from .engine import _BATCH_ARGTYPES, _write_arrays

    lib = load()
    if not hasattr(lib, "_lsm_flush_ready"):
        lib.dbeel_lsm_reader_flush.restype = ctypes.c_int
        lib.dbeel_lsm_reader_flush.argtypes = [
            ctypes.c_char_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t),
            ctypes.c_uint64] + _BATCH_ARGTYPES
        lib._lsm_flush_ready = True
    idx, n = _indices_array(indices)
    nw, ptrs, keepalive = _write_arrays(writes)
    rc = lib.dbeel_lsm_reader_flush(dir.encode(), reader._h, idx,
                                    ctypes.byref(n), sstable_index, nw, *ptrs)
    del keepalive
    _check(rc, lib)
    return [int(idx[i]) for i in range(n.value)]


def reader_memtable_flush(dir: str, reader, indices, sstable_index: int):
    """The flush of the reader's resident memtable (Reader.put): its run is
    fetched, written as {sstable_index:020}.data/.index (no .bloom) and
    only then linked in as the newest table. sstable_index must exceed every
    index held. Returns the new indices list; the reader then answers as a
    fresh open_reader(dir) would. An empty memtable writes nothing; a file
    that cannot be written leaves reader and memtable untouched."""
    lib = load()
    if not hasattr(lib, "_lsm_mem_flush_ready"):
        lib.dbeel_lsm_reader_memtable_flush.restype = ctypes.c_int
        lib.dbeel_lsm_reader_memtable_flush.argtypes = [
            ctypes.c_char_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t),
            ctypes.c_uint64]
        lib._lsm_mem_flush_ready = True
    idx, n = _indices_array(indices)
    rc = lib.dbeel_lsm_reader_memtable_flush(dir.encode(), reader._h, idx,
                                             ctypes.byref(n), sstable_index)
    _check(rc, lib)
    return [int(idx[i]) for i in range(n.value)]


def reader_compact(dir: str, reader, indices, compact_indices,
                   output_index: int, keep_tombstones: bool,
                   device_unused=None,
                   bloom_min_size: int = DEFAULT_BLOOM_MIN_SIZE):
    """compact() for a directory an open reader covers: the runs are
    compacted where they lie in the reader's device memory (no file reads,
    no upload), the directory goes through the same staging / journal /
    rename / delete sequence, and the reader's list is swapped between the
    renames and the deletes. Returns the new indices list. The device is
    the reader's; device_unused keeps compact()'s argument order."""
    lib = _load_live(load())
    idx, n = _indices_array(indices)
    arr = (ctypes.c_uint64 * max(1, len(compact_indices)))(*compact_indices)
    out = ctypes.c_uint64()
    rc = lib.dbeel_lsm_reader_compact(
        dir.encode(), reader._h, idx, ctypes.byref(n), arr,
        len(compact_indices), output_index, int(keep_tombstones),
        bloom_min_size, ctypes.byref(out))
    _check(rc, lib)
    return [int(idx[i]) for i in range(n.value)]


def write_run_files(dir: str, index: int, data: bytes, idx: bytes) -> None:
    """Write {index:020}.data/.index (test/bench helper)."""
    os.makedirs(dir, exist_ok=True)
    with open(os.path.join(dir, f"{index:020d}.data"), "wb") as f:
        f.write(data)
    with open(os.path.join(dir, f"{index:020d}.index"), "wb") as f:
        f.write(idx)


def read_run_files(dir: str, index: int) -> tuple[bytes, bytes]:
    with open(os.path.join(dir, f"{index:020d}.data"), "rb") as f:
        data = f.read()
    with open(os.path.join(dir, f"{index:020d}.index"), "rb") as f:
        idx = f.read()
    return data, idx
