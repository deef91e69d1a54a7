"""CPU-side checks of the write-batch ABI (sort + deduplicate + encode an
unsorted write batch into a resident table): the symbols are declared and
exported, the stats mirror matches the header, and bad arguments are refused
before any device access (so these run without a GPU)."""
import ctypes
import os

import pytest

import batch_model
from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG, ITEM_TOO_LARGE = 1, 3


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def test_write_batch_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in ("dbeel_gpu_reader_write_batch", "dbeel_gpu_flush_batch",
                "dbeel_write_batch_stats"):
        assert sym in hdr, sym
    for sym in ("dbeel_gpu_reader_write_batch", "dbeel_gpu_flush_batch",
                "dbeel_lsm_reader_flush"):
        assert getattr(lib, sym, None) is not None, sym
    lsm_hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_lsm.h")).read()
    assert "dbeel_lsm_reader_flush" in lsm_hdr
    # library-internal helpers stay internal
    assert getattr(lib, "dbeel_reader_drop_run", None) is None


def test_stats_struct_matches_header_layout():
    _built()
    from dbeel_amd.engine import WriteBatchStats

    # 5 doubles then 5 u64 — no padding anywhere
    assert ctypes.sizeof(WriteBatchStats) == 5 * 8 + 5 * 8
    assert WriteBatchStats.writes_in.offset == 5 * 8
    assert [f for f, _ in WriteBatchStats._fields_] == [
        "h2d_ms", "order_ms", "encode_ms", "adopt_ms", "d2h_ms",
        "writes_in", "entries_out", "data_bytes_out", "prefix_tied",
        "d2h_bytes"]


def test_null_reader_and_null_out():
    _built()
    from dbeel_amd.engine import (CompactResult, WriteBatchStats,
                                  _load_reader, _write_arrays)

    lib = _load_reader()
    n, ptrs, keep = _write_arrays([(b"k", b"v", 1), (b"a", b"", -1)])
    res = CompactResult()
    st = WriteBatchStats()
    bp = ctypes.POINTER(ctypes.c_uint8)()
    bn = ctypes.c_uint64(123)
    rc = lib.dbeel_gpu_reader_write_batch(
        None, 0, n, *ptrs, 1, ctypes.byref(res), ctypes.byref(bp),
        ctypes.byref(bn), ctypes.byref(st))
    assert rc == INVALID_ARG
    assert lib.dbeel_gpu_last_error()
    # outputs are left in a freeable state
    assert not res.data and not res.index and not bp and bn.value == 0
    assert lib.dbeel_gpu_reader_write_batch(
        None, 0, 0, None, None, None, None, None, 0, None, None, None,
        None) == INVALID_ARG

    assert lib.dbeel_gpu_flush_batch(n, *ptrs, 0, None) == INVALID_ARG
    assert lib.dbeel_gpu_last_error()
    del keep


def test_flush_batch_host_validation():
    """Everything flush_batch refuses on the host, in a process with no
    device: NULL arrays, a negative device, a descending offset, an
    oversized write; an empty batch succeeds with zeroed outputs."""
    _built()
    import numpy as np

    from dbeel_amd.engine import CompactResult, _load_reader, _write_arrays

    lib = _load_reader()
    n, ptrs, keep = _write_arrays([(b"k", b"v", 1), (b"a", b"", -1)])
    res = CompactResult()
    assert lib.dbeel_gpu_flush_batch(
        n, None, ptrs[1], ptrs[2], ptrs[3], ptrs[4], 0,
        ctypes.byref(res)) == INVALID_ARG
    assert lib.dbeel_gpu_flush_batch(n, *ptrs, -1,
                                     ctypes.byref(res)) == INVALID_ARG
    u64p = ctypes.POINTER(ctypes.c_uint64)
    desc = np.array([1, 0, 0], dtype=np.uint64)
    assert lib.dbeel_gpu_flush_batch(
        n, ptrs[0], desc.ctypes.data_as(u64p), ptrs[2], ptrs[3], ptrs[4], 0,
        ctypes.byref(res)) == INVALID_ARG
    assert b"descend" in lib.dbeel_gpu_last_error()
    # offsets only: the blob is never read on the host
    huge = np.array([0, 1, 1 + 0xFFFFFFFF - 32], dtype=np.uint64)
    assert lib.dbeel_gpu_flush_batch(
        n, ptrs[0], ptrs[1], ptrs[2], huge.ctypes.data_as(u64p), ptrs[4], 0,
        ctypes.byref(res)) == ITEM_TOO_LARGE
    assert lib.dbeel_gpu_flush_batch(
        1 << 31, *ptrs, 0, ctypes.byref(res)) == INVALID_ARG
    assert not res.data and not res.index

    res.entries_written = 7
    assert lib.dbeel_gpu_flush_batch(0, None, None, None, None, None, 0,
                                     ctypes.byref(res)) == 0
    assert not res.data and not res.index and res.entries_written == 0
    del keep


def test_null_reader_lsm_flush(tmp_path):
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    class _Null:
        _h = None

    with pytest.raises(DbeelGpuError) as ei:
        lsm.reader_flush(str(tmp_path), _Null(), [], 0, [(b"k", b"v", 1)])
    assert ei.value.code == INVALID_ARG
    assert os.listdir(tmp_path) == []


def test_model_self_check():
    batch_model.self_check()
