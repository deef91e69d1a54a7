"""CPU-side checks of the put_entries / scan_apply ABI: the symbols are
declared and exported, the ctypes mirrors match the header, and what can be
refused without a reader or a scan is refused before any device access (so
these run without a GPU). The refusals that need a live reader or scan are in
test_reader_put_entries_gpu.py."""
import ctypes
import os
import re

import migrate_model
from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG = 1
SYMBOLS = ("dbeel_gpu_reader_put_entries", "dbeel_gpu_reader_scan_apply")


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def _header():
    return open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()


def test_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = _header()
    for sym in SYMBOLS + ("dbeel_put_entries_stats", "dbeel_apply_action",
                          "dbeel_scan_apply_stats"):
        assert sym in hdr, sym
    for sym in SYMBOLS:
        assert getattr(lib, sym, None) is not None, sym
    for name, val in (("DBEEL_APPLY_SKIP", 0), ("DBEEL_APPLY_PUT", 1),
                      ("DBEEL_APPLY_DELETE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name


def _field_positions(hdr, typedef_end, fields):
    body = hdr[:hdr.index(typedef_end)]
    body = body[body.rindex("typedef struct {"):]
    return [re.search(r"\b%s\b[,;]" % f, body).start() for f in fields]


def test_struct_mirrors_match_header_layout():
    _built()
    from dbeel_amd.engine import (APPLY_DELETE, APPLY_PUT, APPLY_SKIP,
                                  ApplyAction, PutEntriesStats,
                                  ScanApplyStats)

    assert (APPLY_SKIP, APPLY_PUT, APPLY_DELETE) == (0, 1, 2)
    hdr = _header()
    # 3 doubles then 7 u64 — no padding anywhere
    names = [f for f, _ in PutEntriesStats._fields_]
    assert names == ["h2d_ms", "order_ms", "merge_ms", "entries_in",
                     "selected", "batch_entries", "replaced", "entries",
                     "data_bytes", "prefix_tied"]
    assert ctypes.sizeof(PutEntriesStats) == 3 * 8 + 7 * 8
    assert PutEntriesStats.entries_in.offset == 3 * 8
    pos = _field_positions(hdr, "} dbeel_put_entries_stats;", names)
    assert pos == sorted(pos)
    # a double then 4 u64
    names = [f for f, _ in ScanApplyStats._fields_]
    assert names == ["apply_ms", "put_entries", "delete_entries", "skipped",
                     "groups"]
    assert ctypes.sizeof(ScanApplyStats) == 5 * 8
    assert ScanApplyStats.put_entries.offset == 8
    pos = _field_positions(hdr, "} dbeel_scan_apply_stats;", names)
    assert pos == sorted(pos)
    # int, then a pointer at its natural alignment
    assert [f for f, _ in ApplyAction._fields_] == ["kind", "dst"]
    assert ApplyAction.dst.offset == ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(ApplyAction) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert ("typedef struct { int kind; dbeel_gpu_reader* dst; } "
            "dbeel_apply_action;") in hdr


def test_put_entries_null_reader_is_refused_first_with_stats_zeroed():
    """A NULL reader is the first check: refused even when every other
    argument is bad too, with the stats zeroed."""
    _built()
    import numpy as np

    from dbeel_amd.engine import PutEntriesStats, _load_reader

    lib = _load_reader()
    d, x = migrate_model.encode_page([(b"k", b"v", 1), (b"a", b"", -1)])
    rid = np.zeros(2, dtype=np.uint32)
    take = np.ones(1, dtype=np.uint8)
    ts = np.zeros(16, dtype=np.uint8)
    good = dict(data=d.ctypes.data, data_len=d.nbytes, index=x.ctypes.data,
                n=2, rids=rid.ctypes.data, take=take.ctypes.data, n_take=1,
                mode=1, dts=ts.ctypes.data)

    def call(st=None, **kw):
        a = dict(good, **kw)
        return lib.dbeel_gpu_reader_put_entries(
            None, a["data"], a["data_len"], a["index"], a["n"], a["rids"],
            a["take"], a["n_take"], a["mode"], a["dts"],
            None if st is None else ctypes.byref(st))

    st = PutEntriesStats()
    st.entries = 7
    st.selected = 3
    assert call(st) == INVALID_ARG
    assert b"null reader" in lib.dbeel_gpu_last_error()
    assert st.entries == 0 and st.selected == 0 and st.entries_in == 0
    # ... ahead of NULL data / index, an unknown mode, DELETE without a
    # timestamp, range ids without a mask, 2^31 entries, and an empty page
    for kw in (dict(data=None), dict(index=None), dict(mode=0), dict(mode=3),
               dict(mode=2, dts=None), dict(take=None), dict(n_take=0),
               dict(n=1 << 31), dict(n=0, data=None, index=None)):
        assert call(**kw) == INVALID_ARG, kw
        assert b"null reader" in lib.dbeel_gpu_last_error(), kw


def test_scan_apply_null_scan_is_refused_first_with_outputs_zeroed():
    """A NULL scan (or page) is the first check of scan_apply, ahead of NULL
    actions, a count mismatch, an unknown kind, a NULL destination, a
    missing timestamp and empty page sizes; page and stats are zeroed."""
    _built()
    from dbeel_amd.engine import (ApplyAction, ScanApplyStats, ScanPage,
                                  _load_reader)

    lib = _load_reader()
    acts = (ApplyAction * 2)()
    acts[0].kind = 9       # unknown
    acts[1].kind = 2       # DELETE, no dst, no timestamp
    pg = ScanPage()
    pg.n_entries = 5
    pg.needed = 6
    st = ScanApplyStats()
    st.groups = 4
    st.skipped = 2
    for actions, n in ((acts, 2), (None, 0), (acts, 0)):
        pg.n_entries = 5
        st.groups = 4
        assert lib.dbeel_gpu_reader_scan_apply(
            None, actions, n, None, 0, 0, ctypes.byref(pg),
            ctypes.byref(st)) == INVALID_ARG
        assert b"null scan or page" in lib.dbeel_gpu_last_error()
        assert pg.n_entries == 0 and pg.needed == 0 and pg.done == 0
        assert st.groups == 0 and st.skipped == 0
    # a NULL page is named by the same check; stats are still zeroed
    st.groups = 4
    assert lib.dbeel_gpu_reader_scan_apply(
        None, acts, 2, None, 4096, 16, None,
        ctypes.byref(st)) == INVALID_ARG
    assert b"null scan or page" in lib.dbeel_gpu_last_error()
    assert st.groups == 0
    assert lib.dbeel_gpu_reader_scan_apply(
        None, None, 0, None, 0, 0, None, None) == INVALID_ARG


def test_python_surface_exists():
    _built()
    from dbeel_amd.engine import Reader, ReaderScan

    for cls, name in ((Reader, "put_entries"), (Reader, "migrate"),
                      (ReaderScan, "apply")):
        assert callable(getattr(cls, name, None)), name


def test_model_self_check():
    migrate_model.self_check()
