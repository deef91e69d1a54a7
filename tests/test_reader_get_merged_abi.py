"""CPU-side checks of dbeel_gpu_reader_get_merged (include/dbeel_gpu.h): the
symbol and types are declared and exported, the ctypes mirrors match the
header, a NULL reader, buf or page is refused before any device access (so
these run without a GPU), and the host model the GPU tests compare against
states the winner, tie and stale rules and pages as get_entries' model does.
The refusals that need a live reader are in test_reader_get_merged_gpu.py."""
import ctypes
import os
import re

import numpy as np

import get_entries_model as gem
import merge_model as mm
from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG = 1
TYPES = ("dbeel_merge_source", "dbeel_merge_hit", "dbeel_merge_buffers",
         "dbeel_merge_stats")


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def _header():
    return open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()


def test_symbol_and_types_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = _header()
    assert re.search(r"\bint\s+dbeel_gpu_reader_get_merged\(", hdr)
    assert getattr(lib, "dbeel_gpu_reader_get_merged", None) is not None
    for t in TYPES:
        assert re.search(r"\}\s*%s;" % t, hdr), t
    for name, val in (("DBEEL_MERGE_ANSWERS", 0), ("DBEEL_MERGE_READER", 1),
                      ("DBEEL_MERGE_MAX_SOURCES", 15)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    # the contract names the tie rule and where the local answer stands
    assert "max_by_key" in hdr and "LAST" in hdr


def test_struct_mirrors_match_header_layout():
    _built()
    from dbeel_amd import engine as E

    assert ctypes.sizeof(E.MergeHit) == 24 == E.MERGE_HIT_DTYPE.itemsize
    assert ctypes.sizeof(E.MergeSource) == 32
    assert ctypes.sizeof(E.MergeBuffers) == 32
    assert ctypes.sizeof(E.MergeStats) == 64
    assert [(f, getattr(E.MergeHit, f).offset)
            for f, _ in E.MergeHit._fields_] == [
        ("source", 0), ("is_tombstone", 4), ("value_len", 8),
        ("stale_mask", 16)]
    assert [E.MERGE_HIT_DTYPE.fields[f][1]
            for f in E.MERGE_HIT_DTYPE.names] == [0, 4, 8, 16]
    assert E.MERGE_HIT_DTYPE.names == tuple(
        f for f, _ in E.MergeHit._fields_)
    assert [(f, getattr(E.MergeSource, f).offset)
            for f, _ in E.MergeSource._fields_] == [
        ("kind", 0), ("reader", 8), ("record_offsets", 16), ("records", 24)]
    assert [(f, getattr(E.MergeBuffers, f).offset)
            for f, _ in E.MergeBuffers._fields_] == [
        ("hits", 0), ("record_offsets", 8), ("records", 16),
        ("records_cap", 24)]
    assert [f for f, _ in E.MergeStats._fields_] == [
        "h2d_ms", "search_ms", "pick_ms", "gather_ms", "d2h_ms", "winners",
        "tombstones", "from_local"]
    assert E.MergeStats.from_local.offset == 56
    assert (E.MERGE_ANSWERS, E.MERGE_READER, E.MERGE_MAX_SOURCES) == (0, 1, 15)
    hdr = _header()
    for name, cls in (("dbeel_merge_source", E.MergeSource),
                      ("dbeel_merge_hit", E.MergeHit),
                      ("dbeel_merge_buffers", E.MergeBuffers),
                      ("dbeel_merge_stats", E.MergeStats)):
        body = hdr[:hdr.index("} %s;" % name)]
        body = body[body.rindex("typedef struct {"):]
        pos = [re.search(r"\b%s[;,]" % f, body).start()
               for f, _ in cls._fields_]
        assert pos == sorted(pos), name


def test_get_merged_null_arguments():
    """A NULL local reader, buf or page is the first check: refused whatever
    the other arguments are, the page and stats zeroed, no buffer touched."""
    _built()
    from dbeel_amd.engine import (MERGE_HIT_DTYPE, GetPage, MergeBuffers,
                                  MergeHit, MergeSource, MergeStats,
                                  _key_blob, _load_reader)

    lib = _load_reader()
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    ka, koff = _key_blob([b"k1", b"", b"k1"])
    hits = np.zeros(3, dtype=MERGE_HIT_DTYPE)
    roff = np.full(4, 7, dtype=np.uint64)
    rec = np.full(64, 0xA5, dtype=np.uint8)
    buf = MergeBuffers(hits.ctypes.data_as(ctypes.POINTER(MergeHit)),
                       roff.ctypes.data_as(u64p), rec.ctypes.data_as(u8p), 64)
    kp, op = ka.ctypes.data_as(u8p), koff.ctypes.data_as(u64p)
    srcs = (MergeSource * 1)()
    srcs[0].kind = 7  # never looked at: the NULLs come first
    page, st = GetPage(), MergeStats()
    page.n_done, st.winners, st.pick_ms = 9, 9, 9.0
    call = lib.dbeel_gpu_reader_get_merged
    assert call(None, kp, op, 3, srcs, 1, ctypes.byref(buf),
                ctypes.byref(page), ctypes.byref(st)) == INVALID_ARG
    assert b"null" in lib.dbeel_gpu_last_error()
    assert page.n_done == 0 and st.winners == 0 and st.pick_ms == 0.0
    # ahead of every later check: NULL keys, 2^32 keys, 16 sources, n == 0
    assert call(None, None, None, 3, None, 0, ctypes.byref(buf),
                ctypes.byref(page), None) == INVALID_ARG
    assert call(None, kp, op, 1 << 32, None, 16, ctypes.byref(buf),
                ctypes.byref(page), None) == INVALID_ARG
    assert call(None, None, None, 0, None, 0, ctypes.byref(buf),
                ctypes.byref(page), None) == INVALID_ARG
    # a handle that is never looked at: the three pointers are one check
    fake = (ctypes.c_uint8 * 8192)()
    assert call(fake, kp, op, 3, None, 0, None, ctypes.byref(page),
                None) == INVALID_ARG
    assert call(fake, kp, op, 3, None, 0, ctypes.byref(buf), None,
                None) == INVALID_ARG
    assert call(None, None, None, 0, None, 0, None, None, None) == INVALID_ARG
    assert np.all(rec == 0xA5) and np.all(roff == 7)
    assert not hits.view(np.uint8).any()


def test_get_merged_key_batch_refusals_name_their_caller():
    """A key batch whose offsets descend, or of 2^32 keys, is refused before
    the reader handle is looked at or any device call is made: a zeroed
    buffer stands in for the local reader and there are no sources. The
    message is get_merged's own and names the index; no caller buffer is
    touched."""
    _built()
    from dbeel_amd.engine import (MERGE_HIT_DTYPE, GetPage, MergeBuffers,
                                  MergeHit, _load_reader)

    lib = _load_reader()
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    ka = np.frombuffer(b"abcd", dtype=np.uint8)
    koff = np.array([0, 2, 1, 4], dtype=np.uint64)  # descends at index 1
    hits = np.zeros(3, dtype=MERGE_HIT_DTYPE)
    roff = np.full(4, 7, dtype=np.uint64)
    rec = np.full(64, 0xA5, dtype=np.uint8)
    buf = MergeBuffers(hits.ctypes.data_as(ctypes.POINTER(MergeHit)),
                       roff.ctypes.data_as(u64p), rec.ctypes.data_as(u8p), 64)
    kp, op = ka.ctypes.data_as(u8p), koff.ctypes.data_as(u64p)
    fake = (ctypes.c_uint8 * 8192)()
    call = lib.dbeel_gpu_reader_get_merged
    for n, text in (
            (3, b"reader_get_merged: key_offsets not ascending at 1"),
            (1 << 32, b"reader_get_merged: 2^32 or more keys in one batch")):
        page = GetPage()
        page.n_done = 9
        assert call(fake, kp, op, n, None, 0, ctypes.byref(buf),
                    ctypes.byref(page), None) == INVALID_ARG
        assert lib.dbeel_gpu_last_error() == text
        assert page.n_done == 0
    assert np.all(rec == 0xA5) and np.all(roff == 7)
    assert not hits.view(np.uint8).any()
    assert not bytes(fake).strip(b"\0")


def test_model_self_check():
    mm.self_check()


def test_model_paging_is_get_entries_paging():
    """The model's page over the winners' sizes is get_entries_model.paging
    on the same offsets, at random caps, boundaries included."""
    from dbeel_amd.format import Entry, build_run

    rng = np.random.default_rng(11)
    for trial in range(20):
        n = int(rng.integers(0, 12))
        keys = [b"k%02d" % i for i in range(n)]
        mk = lambda: gem.Model([build_run(
            [Entry(k, bytes(int(rng.integers(0, 40))), int(rng.integers(0, 4)))
             for k in keys if rng.random() < 0.6])])
        local, a, b = mk(), mk(), mk()
        sources = [a, mm.answers_of(b, keys)]
        _, offsets, records, rc0, page0 = mm.expect(keys, local, sources)
        assert (rc0, page0) == gem.paging(offsets, offsets[-1])
        assert page0["n_done"] == n and len(records) == offsets[-1]
        caps = {0, 23, 24, offsets[-1]} | set(offsets) | {
            max(o - 1, 0) for o in offsets} | {
            int(rng.integers(0, offsets[-1] + 2)) for _ in range(4)}
        for cap in sorted(caps):
            h, off, rec, rc, page = mm.expect(keys, local, sources, cap)
            assert off == offsets and rec == records
            assert (rc, page) == gem.paging(offsets, cap)
