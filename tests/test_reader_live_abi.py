"""CPU-side checks of the live-reader ABI (insert a flushed run, compact
resident runs, swap the list): the symbols are declared and exported, and a
NULL reader is refused by every new call before any device access (so these
run without a GPU)."""
import ctypes
import os

import pytest

from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

GPU_SYMBOLS = [
    "dbeel_gpu_reader_run_count",
    "dbeel_gpu_reader_insert_run",
    "dbeel_gpu_reader_compact_begin",
    "dbeel_gpu_reader_compact_commit",
    "dbeel_gpu_reader_compact_abort",
]
LSM_SYMBOLS = ["dbeel_lsm_reader_add", "dbeel_lsm_reader_compact"]

INVALID_ARG = 1


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def _run():
    from dbeel_amd.format import Entry, build_run

    return build_run([Entry(b"a", b"b", 1)])


def test_live_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in GPU_SYMBOLS:
        assert sym in hdr, sym
        assert getattr(lib, sym, None) is not None, sym
    assert "dbeel_reader_compact_stats" in hdr
    lsm_hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_lsm.h")).read()
    for sym in LSM_SYMBOLS:
        assert sym in lsm_hdr, sym
        assert getattr(lib, sym, None) is not None, sym
    # library-internal helpers stay internal
    assert getattr(lib, "dbeel_reader_run_data_len", None) is None


def test_stats_struct_matches_header_layout():
    _built()
    from dbeel_amd.engine import CompactTimings, ReaderCompactStats

    # dbeel_compact_timings, 2 doubles, 4 u64 — no padding anywhere
    assert ctypes.sizeof(ReaderCompactStats) == (
        ctypes.sizeof(CompactTimings) + 2 * 8 + 4 * 8)
    assert ReaderCompactStats.pipeline.offset == 0


def test_null_reader_gpu_calls():
    _built()
    from dbeel_amd.engine import (BloomView, CompactResult,
                                  ReaderCompactStats, _load_reader, _views)

    lib = _load_reader()
    assert lib.dbeel_gpu_reader_run_count(None) == 0
    views, keep = _views([_run()])
    assert lib.dbeel_gpu_reader_insert_run(None, 0, views, None) == INVALID_ARG
    assert lib.dbeel_gpu_last_error()
    bv = BloomView()
    assert lib.dbeel_gpu_reader_insert_run(
        None, 0, views, ctypes.byref(bv)) == INVALID_ARG

    pos = (ctypes.c_uint32 * 1)(0)
    res = CompactResult()
    st = ReaderCompactStats()
    bp = ctypes.POINTER(ctypes.c_uint8)()
    bn = ctypes.c_uint64(123)
    rc = lib.dbeel_gpu_reader_compact_begin(
        None, pos, 1, 1, 1, ctypes.byref(res), ctypes.byref(bp),
        ctypes.byref(bn), ctypes.byref(st))
    assert rc == INVALID_ARG
    # outputs are left in a freeable state
    assert not res.data and not res.index and not bp and bn.value == 0
    assert lib.dbeel_gpu_reader_compact_begin(
        None, pos, 1, 0, 0, None, None, None, None) == INVALID_ARG
    assert lib.dbeel_gpu_reader_compact_commit(None, 0) == INVALID_ARG
    lib.dbeel_gpu_reader_compact_abort(None)  # no-op, must not crash
    del keep


def test_null_reader_lsm_calls(tmp_path):
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    class _Null:
        _h = None

    d, i = _run()
    lsm.write_run_files(str(tmp_path), 0, d, i)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DbeelGpuError) as ei:
        lsm.reader_add(str(tmp_path), _Null(), [], 0)
    assert ei.value.code == INVALID_ARG
    with pytest.raises(DbeelGpuError) as ei:
        lsm.reader_compact(str(tmp_path), _Null(), [0], [0], 1, True)
    assert ei.value.code == INVALID_ARG
    assert sorted(os.listdir(tmp_path)) == before
