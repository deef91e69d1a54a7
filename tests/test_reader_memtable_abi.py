"""CPU-side checks of the resident-memtable ABI (put / memtable_info /
memtable_fetch / memtable_flush / memtable_clear and the file layer's
reader_memtable_flush): the symbols are declared and exported, the ctypes
mirrors match the header, and what can be refused without a reader is
refused before any device access (so these run without a GPU). The refusals
that need a live reader — a descending offset, the 2^31 bounds, an oversized
write, in the header's order — are in test_reader_memtable_gpu.py."""
import ctypes
import os
import re

import pytest

import memtable_model
from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG = 1
SYMBOLS = ("dbeel_gpu_reader_put", "dbeel_gpu_reader_memtable_info",
           "dbeel_gpu_reader_memtable_fetch",
           "dbeel_gpu_reader_memtable_flush",
           "dbeel_gpu_reader_memtable_clear")


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def test_memtable_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in SYMBOLS + ("dbeel_memtable_put_stats", "dbeel_memtable_info"):
        assert sym in hdr, sym
    for sym in SYMBOLS + ("dbeel_lsm_reader_memtable_flush",):
        assert getattr(lib, sym, None) is not None, sym
    lsm_hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_lsm.h")).read()
    assert "dbeel_lsm_reader_memtable_flush" in lsm_hdr


def test_struct_mirrors_match_header_layout():
    _built()
    from dbeel_amd.engine import MemtableInfo, MemtablePutStats

    # 3 doubles then 6 u64 — no padding anywhere
    assert ctypes.sizeof(MemtablePutStats) == 3 * 8 + 6 * 8
    assert MemtablePutStats.writes_in.offset == 3 * 8
    assert [f for f, _ in MemtablePutStats._fields_] == [
        "h2d_ms", "order_ms", "merge_ms", "writes_in", "batch_entries",
        "replaced", "entries", "data_bytes", "prefix_tied"]
    assert ctypes.sizeof(MemtableInfo) == 4 * 8
    assert [f for f, _ in MemtableInfo._fields_] == [
        "entries", "data_bytes", "reserved_bytes", "puts"]
    # the header declares the fields in the mirrors' order
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    body = hdr[:hdr.index("} dbeel_memtable_put_stats;")]
    body = body[body.rindex("typedef struct {"):]
    pos = [re.search(r"\b%s\b[,;]" % f, body).start()
           for f, _ in MemtablePutStats._fields_]
    assert pos == sorted(pos)
    assert ("typedef struct { uint64_t entries, data_bytes, reserved_bytes, "
            "puts; } dbeel_memtable_info;") in hdr


def test_null_reader_is_refused_first_with_outputs_zeroed():
    """A NULL reader is the first check of every call: refused even when
    every other argument is bad too, with the outputs zeroed and
    freeable."""
    _built()
    import numpy as np

    from dbeel_amd.engine import (CompactResult, MemtableInfo,
                                  MemtablePutStats, _load_reader,
                                  _write_arrays)

    lib = _load_reader()
    n, ptrs, keep = _write_arrays([(b"k", b"v", 1), (b"a", b"", -1)])
    u64p = ctypes.POINTER(ctypes.c_uint64)

    st = MemtablePutStats()
    st.entries = 7
    assert lib.dbeel_gpu_reader_put(None, n, *ptrs,
                                    ctypes.byref(st)) == INVALID_ARG
    assert b"null reader" in lib.dbeel_gpu_last_error()
    assert st.entries == 0 and st.writes_in == 0
    # ... ahead of a NULL array, 2^31 writes, a descending offset and an
    # oversized write (arrays that only carry offsets)
    desc = np.array([1, 0, 0], dtype=np.uint64)
    huge = np.array([0, 1, 1 + 0xFFFFFFFF - 32], dtype=np.uint64)
    for args in ((n, None, ptrs[1], ptrs[2], ptrs[3], ptrs[4]),
                 (1 << 31, *ptrs),
                 (n, ptrs[0], desc.ctypes.data_as(u64p), *ptrs[2:]),
                 (n, ptrs[0], ptrs[1], ptrs[2], huge.ctypes.data_as(u64p),
                  ptrs[4]),
                 (0, None, None, None, None, None)):
        assert lib.dbeel_gpu_reader_put(None, *args, None) == INVALID_ARG
        assert b"null reader" in lib.dbeel_gpu_last_error()

    info = MemtableInfo()
    info.puts = 3
    assert lib.dbeel_gpu_reader_memtable_info(
        None, ctypes.byref(info)) == INVALID_ARG
    assert info.puts == 0
    assert lib.dbeel_gpu_reader_memtable_info(None, None) == INVALID_ARG

    res = CompactResult()
    res.entries_written = 9
    assert lib.dbeel_gpu_reader_memtable_fetch(
        None, ctypes.byref(res)) == INVALID_ARG
    assert not res.data and not res.index and res.entries_written == 0
    assert lib.dbeel_gpu_reader_memtable_fetch(None, None) == INVALID_ARG

    res.entries_written = 9
    bp = ctypes.POINTER(ctypes.c_uint8)()
    bn = ctypes.c_uint64(123)
    assert lib.dbeel_gpu_reader_memtable_flush(
        None, 1, ctypes.byref(res), ctypes.byref(bp),
        ctypes.byref(bn)) == INVALID_ARG
    assert lib.dbeel_gpu_last_error()
    assert not res.data and not res.index and res.entries_written == 0
    assert not bp and bn.value == 0
    assert lib.dbeel_gpu_reader_memtable_flush(
        None, 0, None, None, None) == INVALID_ARG

    lib.dbeel_gpu_reader_memtable_clear(None)  # a no-op, not a crash
    del keep


def test_null_reader_lsm_memtable_flush(tmp_path):
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    class _Null:
        _h = None

    with pytest.raises(DbeelGpuError) as ei:
        lsm.reader_memtable_flush(str(tmp_path), _Null(), [], 0)
    assert ei.value.code == INVALID_ARG
    assert os.listdir(tmp_path) == []


def test_model_self_check():
    memtable_model.self_check()
