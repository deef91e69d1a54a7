"""CPU-side checks of the snapshot scan ABI (dbeel_gpu_reader_scan_snapshot,
dbeel_gpu_reader_scan_info, dbeel_gpu_reader_held_bytes, include/dbeel_gpu.h):
the symbols are declared and exported, the host-side validation refuses bad
flags and NULL handles before any device access (so these run without a GPU),
the ctypes struct has the C layout, and the host model checks itself."""
import ctypes
import os

from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

SYMBOLS = [
    "dbeel_gpu_reader_scan_snapshot",
    "dbeel_gpu_reader_scan_info",
    "dbeel_gpu_reader_held_bytes",
]

INVALID_ARG = 1


def _lib():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    from dbeel_amd.engine import _load_reader

    return _load_reader()


def _snapshot(lib, reader, flags):
    h = ctypes.c_void_p(123)
    rc = lib.dbeel_gpu_reader_scan_snapshot(reader, None, 0, None, 0, None,
                                            None, 0, 0, flags,
                                            ctypes.byref(h))
    return rc, h


def test_snapshot_symbols_declared_and_exported():
    lib = _lib()
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in SYMBOLS:
        assert sym in hdr, sym
        assert getattr(lib, sym, None) is not None, sym
    for name in ("DBEEL_SCAN_MEMTABLE", "DBEEL_SCAN_NEWEST_ONLY",
                 "dbeel_scan_snapshot_info"):
        assert name in hdr, name


def test_unknown_flags_refused_first():
    lib = _lib()
    # flags are checked before the reader: a NULL reader still names them
    for flags in (4, 0x80000000, 3 | 8):
        rc, h = _snapshot(lib, None, flags)
        assert rc == INVALID_ARG
        assert b"flags" in lib.dbeel_gpu_last_error()
        assert not h.value


def test_null_reader_with_valid_flags():
    lib = _lib()
    for flags in (0, 1, 2, 3):
        rc, h = _snapshot(lib, None, flags)
        assert rc == INVALID_ARG
        msg = lib.dbeel_gpu_last_error()
        assert b"null" in msg and b"flags" not in msg
        assert not h.value
    assert lib.dbeel_gpu_reader_scan_snapshot(
        None, None, 0, None, 0, None, None, 0, 0, 0, None) == INVALID_ARG


def test_scan_info_null():
    lib = _lib()
    from dbeel_amd.engine import ScanSnapshotInfo

    si = ScanSnapshotInfo()
    si.shadowed = 7
    assert lib.dbeel_gpu_reader_scan_info(None, ctypes.byref(si)) \
        == INVALID_ARG
    assert si.shadowed == 0  # cleared
    assert lib.dbeel_gpu_reader_scan_info(None, None) == INVALID_ARG
    assert lib.dbeel_gpu_last_error()


def test_held_bytes_null_is_zero():
    assert _lib().dbeel_gpu_reader_held_bytes(None) == 0


def test_info_struct_matches_header_layout():
    _lib()
    from dbeel_amd.engine import ScanSnapshotInfo as S

    # 2 u32 | 3 u64: no padding
    assert ctypes.sizeof(S) == 32
    assert (S.n_tables.offset, S.has_memtable.offset,
            S.table_candidates.offset, S.memtable_candidates.offset,
            S.shadowed.offset) == (0, 4, 8, 16, 24)


def test_flag_values_match_header():
    from dbeel_amd import engine

    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    assert "#define DBEEL_SCAN_MEMTABLE     1u" in hdr
    assert "#define DBEEL_SCAN_NEWEST_ONLY  2u" in hdr
    assert (engine.SCAN_MEMTABLE, engine.SCAN_NEWEST_ONLY) == (1, 2)


def test_model_self_check():
    import snapshot_model

    snapshot_model.self_check()
