"""CPU-side checks of the paged resident scan ABI
(dbeel_gpu_reader_scan_begin / _next / _end, include/dbeel_gpu.h): the
symbols and the page struct are declared and exported, and NULL handles are
refused before any device access (so these run without a GPU)."""
import ctypes
import os

from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

SYMBOLS = [
    "dbeel_gpu_reader_scan_begin",
    "dbeel_gpu_reader_scan_next",
    "dbeel_gpu_reader_scan_end",
]

INVALID_ARG = 1


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def test_scan_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in SYMBOLS:
        assert sym in hdr, sym
        assert getattr(lib, sym, None) is not None, sym
    assert "dbeel_scan_page" in hdr
    # the default window size is part of the contract
    assert "2^20" in hdr


def test_page_struct_matches_header_layout():
    _built()
    from dbeel_amd.engine import ScanPage

    # 4 u64 | int + 4 B padding | 4 doubles
    assert ctypes.sizeof(ScanPage) == 4 * 8 + 8 + 4 * 8
    assert ScanPage.done.offset == 32
    assert ScanPage.flag_ms.offset == 40


def test_begin_null_reader():
    _built()
    from dbeel_amd.engine import _load_reader

    lib = _load_reader()
    h = ctypes.c_void_p(123)
    rc = lib.dbeel_gpu_reader_scan_begin(None, None, 0, None, 0, None, None,
                                         0, 0, ctypes.byref(h))
    assert rc == INVALID_ARG
    assert lib.dbeel_gpu_last_error()
    assert not h.value  # left in a state scan_end accepts
    # a NULL out is refused as well
    assert lib.dbeel_gpu_reader_scan_begin(None, None, 0, None, 0, None, None,
                                           0, 0, None) == INVALID_ARG


def test_next_null_scan():
    _built()
    from dbeel_amd.engine import ScanPage, _load_reader

    lib = _load_reader()
    data = (ctypes.c_uint8 * 64)()
    index = (ctypes.c_uint8 * 16)()
    pg = ScanPage()
    pg.n_entries = 7
    rc = lib.dbeel_gpu_reader_scan_next(None, data, 64, index, 16, None,
                                        ctypes.byref(pg))
    assert rc == INVALID_ARG
    assert b"null" in lib.dbeel_gpu_last_error()
    assert pg.n_entries == 0 and pg.done == 0  # the page is cleared
    assert lib.dbeel_gpu_reader_scan_next(None, data, 64, index, 16, None,
                                          None) == INVALID_ARG


def test_end_null_is_noop():
    _built()
    from dbeel_amd.engine import _load_reader

    _load_reader().dbeel_gpu_reader_scan_end(None)
