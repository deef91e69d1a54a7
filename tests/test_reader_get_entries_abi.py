"""CPU-side checks of dbeel_gpu_reader_get_entries / _compact_fetch
(include/dbeel_gpu.h): the symbols and types are declared and exported, the
ctypes mirrors match the header, NULL arguments are refused before any device
access (so these run without a GPU), and the host model the GPU tests compare
against agrees with parse_run on the golden fixtures and states the paging
rule. The refusals that need a live reader are in
test_reader_get_entries_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import get_entries_model as gem
from conftest import GOLDEN_CASES, REPO_ROOT, load_golden
from dbeel_amd.format import encode_entry, parse_run

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG = 1
SYMBOLS = ("dbeel_gpu_reader_get_entries", "dbeel_gpu_reader_compact_fetch")
TYPES = ("dbeel_get_buffers", "dbeel_get_page", "dbeel_get_stats")


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def test_symbols_and_types_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % sym, hdr), sym
        assert getattr(lib, sym, None) is not None, sym
    for t in TYPES:
        assert re.search(r"\}\s*%s;" % t, hdr), t
    # the contract says why a page is stateless and what that costs
    assert "2 %" in hdr and "stale" in hdr


def test_struct_mirrors_match_header_layout():
    _built()
    from dbeel_amd.engine import GetBuffers, GetPage

    assert ctypes.sizeof(GetBuffers) == 32
    assert ctypes.sizeof(GetPage) == 32
    assert [f for f, _ in GetBuffers._fields_] == [
        "hits", "record_offsets", "records", "records_cap"]
    assert [f for f, _ in GetPage._fields_] == [
        "n_done", "records_len", "records_total", "needed"]
    assert GetBuffers.records_cap.offset == 24 and GetPage.needed.offset == 24
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for name, cls in (("dbeel_get_buffers", GetBuffers),
                      ("dbeel_get_page", GetPage)):
        body = hdr[:hdr.index("} %s;" % name)]
        body = body[body.rindex("typedef struct {"):]
        pos = [re.search(r"\b%s;" % f, body).start()
               for f, _ in cls._fields_]
        assert pos == sorted(pos), name


def _args():
    from dbeel_amd.engine import (HIT_DTYPE, GetBuffers, LookupHit, _key_blob)

    ka, koff = _key_blob([b"k1", b"", b"k1"])
    hits = np.zeros(3, dtype=HIT_DTYPE)
    roff = np.full(4, 7, dtype=np.uint64)
    rec = np.full(64, 0xA5, dtype=np.uint8)
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    buf = GetBuffers(hits.ctypes.data_as(ctypes.POINTER(LookupHit)),
                     roff.ctypes.data_as(u64p), rec.ctypes.data_as(u8p), 64)
    return (ka.ctypes.data_as(u8p), koff.ctypes.data_as(u64p), buf,
            (ka, koff, hits, roff, rec))


def test_get_entries_null_arguments():
    """A NULL reader, buf or page is the first check: refused whatever the
    other arguments are, the page and stats zeroed, no buffer touched."""
    _built()
    from dbeel_amd.engine import GetPage, GetStats, _load_reader

    lib = _load_reader()
    kp, op, buf, keep = _args()
    ka, koff, hits, roff, rec = keep
    page, st = GetPage(), GetStats()
    page.n_done, st.hits = 9, 9
    call = lib.dbeel_gpu_reader_get_entries
    assert call(None, kp, op, 3, ctypes.byref(buf), ctypes.byref(page),
                ctypes.byref(st)) == INVALID_ARG
    assert b"null" in lib.dbeel_gpu_last_error()
    assert page.n_done == 0 and st.hits == 0
    # ahead of every later check: NULL keys, 2^32 keys, n_keys == 0
    assert call(None, None, None, 3, ctypes.byref(buf), ctypes.byref(page),
                None) == INVALID_ARG
    assert call(None, kp, op, 1 << 32, ctypes.byref(buf), ctypes.byref(page),
                None) == INVALID_ARG
    assert call(None, None, None, 0, ctypes.byref(buf), ctypes.byref(page),
                None) == INVALID_ARG
    # a handle that is never looked at: the three pointers are one check
    fake = (ctypes.c_uint8 * 8192)()
    assert call(fake, kp, op, 3, None, ctypes.byref(page),
                None) == INVALID_ARG
    assert call(fake, kp, op, 3, ctypes.byref(buf), None,
                None) == INVALID_ARG
    assert call(None, None, None, 0, None, None, None) == INVALID_ARG
    assert np.all(rec == 0xA5) and np.all(roff == 7)
    assert not hits.view(np.uint8).any()


def test_get_entries_key_batch_refusals_name_their_caller():
    """A key batch whose offsets descend, or of 2^32 keys, is refused before
    the reader handle is looked at or any device call is made: a zeroed
    buffer stands in for the reader. The message is get_entries' own and
    names the index; no caller buffer is touched."""
    _built()
    from dbeel_amd.engine import GetPage, _load_reader

    lib = _load_reader()
    kp, _, buf, keep = _args()
    ka, _, hits, roff, rec = keep
    koff = np.array([0, 2, 1, 4], dtype=np.uint64)  # descends at index 1
    op = koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    fake = (ctypes.c_uint8 * 8192)()
    call = lib.dbeel_gpu_reader_get_entries
    for n, text in (
            (3, b"reader_get_entries: key_offsets not ascending at 1"),
            (1 << 32, b"reader_get_entries: 2^32 or more keys in one batch")):
        page = GetPage()
        page.n_done = 9
        assert call(fake, kp, op, n, ctypes.byref(buf), ctypes.byref(page),
                    None) == INVALID_ARG
        assert lib.dbeel_gpu_last_error() == text
        assert page.n_done == 0
    assert np.all(rec == 0xA5) and np.all(roff == 7)
    assert not hits.view(np.uint8).any()
    assert not bytes(fake).strip(b"\0")


def test_compact_fetch_null_arguments():
    _built()
    from dbeel_amd.engine import _load_reader

    lib = _load_reader()
    call = lib.dbeel_gpu_reader_compact_fetch
    data = np.full(64, 0xA5, dtype=np.uint8)
    index = np.full(16, 0xA5, dtype=np.uint8)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    dp, ip = data.ctypes.data_as(u8p), index.ctypes.data_as(u8p)
    dl, il = ctypes.c_uint64(5), ctypes.c_uint64(5)
    ms = ctypes.c_double(5.0)
    assert call(None, dp, 64, ip, 16, ctypes.byref(dl), ctypes.byref(il),
                ctypes.byref(ms)) == INVALID_ARG
    assert b"null" in lib.dbeel_gpu_last_error()
    assert dl.value == 0 and il.value == 0 and ms.value == 0.0
    fake = (ctypes.c_uint8 * 8192)()  # never looked at: NULLs come first
    for a in ((None, 64, ip, 16, ctypes.byref(dl), ctypes.byref(il)),
              (dp, 64, None, 16, ctypes.byref(dl), ctypes.byref(il)),
              (dp, 64, ip, 16, None, ctypes.byref(il)),
              (dp, 64, ip, 16, ctypes.byref(dl), None)):
        assert call(fake, *a, None) == INVALID_ARG
        assert b"null" in lib.dbeel_gpu_last_error()
    assert call(None, None, 0, None, 0, None, None, None) == INVALID_ARG
    assert np.all(data == 0xA5) and np.all(index == 0xA5)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_model_agrees_with_parse_run(name):
    """Per key the model names the highest run holding it, the value's
    offset in that run's data, and a record that is the stored entry minus
    its key_len | key head."""
    runs, _, _ = load_golden(name)
    m = gem.Model(runs)
    newest = {}
    for r, (d, i) in enumerate(runs):
        off = 0
        for e in parse_run(d, i):
            newest[e.key] = (r, off, e)
            off += len(encode_entry(e))
    assert b"\xff" * 40 not in newest
    keys = sorted(newest) + [b"\xff" * 40] + sorted(newest)[:3]  # repeats
    hits, offsets, records, rc, page = m.expect(keys)
    assert len(hits) == len(keys) and len(offsets) == len(keys) + 1
    for q, k in enumerate(keys):
        rec = records[offsets[q]:offsets[q + 1]]
        if k not in newest:
            assert hits[q] == (-1, 0, 0, 0) and rec == b""
            continue
        r, off, e = newest[k]
        data = runs[r][0]
        run, tomb, voff, vlen = hits[q]
        assert (run, tomb, vlen) == (r, int(not e.data), len(e.data))
        assert data[voff:voff + vlen] == e.data
        assert rec == data[voff - 8:off + len(encode_entry(e))]
        assert len(rec) == 24 + vlen
        assert int.from_bytes(rec[-16:], "little", signed=True) == e.timestamp
    assert page["records_total"] == len(records) == offsets[-1]
    assert page["n_done"] == len(keys) and page["needed"] == 0
    assert rc == 0
    assert m.entries(keys) == [
        (newest[k][2].data, newest[k][2].timestamp) if k in newest else None
        for k in keys]


def test_model_memtable_wins_and_is_reported_past_the_runs():
    import memtable_model
    from dbeel_amd.format import Entry, build_run

    run = build_run([Entry(b"a", b"old", 100), Entry(b"b", b"keep", 1)])
    mt = memtable_model.Memtable()
    mt.put([(b"a", b"first", 500), (b"c", b"", 3), (b"a", b"last", -7)])
    m = gem.Model([run], mt)
    hits, offsets, records, rc, page = m.expect([b"a", b"b", b"c", b"d"])
    assert [h[0] for h in hits] == [1, 0, 1, -1]
    assert m.entries([b"a", b"b", b"c", b"d"]) == [
        (b"last", -7), (b"keep", 1), (b"", 3), None]
    assert offsets == [0, 28, 56, 80, 80] and rc == 0
    md = mt.run()[0]
    assert md[hits[0][2]:hits[0][2] + 4] == b"last"


def test_paging_rule_on_a_hand_written_offset_list():
    gem.self_check()
    #       q0: 30 B   q1: absent   q2: 24 B   q3: 46 B   q4, q5: absent
    off = [0, 30, 30, 54, 100, 100, 100]
    page = lambda cap: gem.paging(off, cap)
    # exact fit: everything, the trailing absents included
    assert page(100) == (0, {"n_done": 6, "records_len": 100,
                             "records_total": 100, "needed": 0})
    assert page(1 << 40)[1]["n_done"] == 6
    # one byte short: q3 does not fit, and neither do the absents behind it
    assert page(99) == (0, {"n_done": 3, "records_len": 54,
                            "records_total": 100, "needed": 46})
    # a boundary in the middle, and one byte before it; the absent q1 rides
    # with q0
    assert page(54)[1]["n_done"] == 3
    assert page(53) == (0, {"n_done": 2, "records_len": 30,
                            "records_total": 100, "needed": 24})
    assert page(30)[1] == {"n_done": 2, "records_len": 30,
                           "records_total": 100, "needed": 24}
    # the first record over the cap
    assert page(29) == (gem.ITEM_TOO_LARGE,
                        {"n_done": 0, "records_len": 0,
                         "records_total": 100, "needed": 30})
    assert page(0)[0] == gem.ITEM_TOO_LARGE
    # only absents: done at cap 0
    assert gem.paging([0, 0, 0], 0) == (0, {"n_done": 2, "records_len": 0,
                                            "records_total": 0, "needed": 0})
    # leading absents do not turn a too-large first RECORD into progress
    # forever: they are done, the record behind them is the next call's q0
    assert gem.paging([0, 0, 40], 10) == (0, {"n_done": 1, "records_len": 0,
                                              "records_total": 40,
                                              "needed": 40})
    assert gem.paging([0], 0)[0] == 0
