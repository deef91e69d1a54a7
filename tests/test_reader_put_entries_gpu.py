"""GPU tests of Reader.put_entries / ReaderScan.apply / Reader.migrate: a page
exactly as a paged scan writes it goes into a memtable as puts or as
tombstones, from the host or without leaving the device
(tasks/migration.rs:62-131; the receiver's set_with_timestamp, shards.rs:768).

Oracle: tests/migrate_model.py feeding memtable_model.Memtable
(batch_model.flush_run over the arrivals) for bytes and counts, a second
reader fed the decoded writes through the untouched Reader.put, and a FRESH
Reader for answers — never the path under test.
"""
import numpy as np
import pytest

import batch_model
import migrate_model
import snapshot_model
from dbeel_amd import engine
from dbeel_amd.engine import DbeelGpuError, Reader
from memtable_model import I128_MAX, I128_MIN, Memtable, gen, key_pool
from migrate_model import DELETE, PUT, decode_page, encode_page
from pymm3 import between_cmp, murmur3_32

pytestmark = pytest.mark.gpu

INVALID_ARG, CORRUPT, ITEM_TOO_LARGE = 1, 2, 3
POOL = key_pool(11, 160)


@pytest.fixture(params=["radix", "merge"])
def order(request, monkeypatch):
    """The order stage's environment switch, read by the engine per call."""
    monkeypatch.setenv("DBEEL_BATCH_ORDER", request.param)
    return request.param


_BASE = None
# a destination's only table: one key no test writes (a reader needs a run)
DEST = [batch_model.flush_run([(b"\xff unrelated", b"x", 0)])]


def _base():
    """Two small runs over POOL, built once and never changed."""
    global _BASE
    if _BASE is None:
        _BASE = [batch_model.flush_run(gen(1, 120, POOL[::3])),
                 batch_model.flush_run(gen(2, 90, POOL[1::4]))]
    return _BASE


def _code(fn, *a, **kw):
    with pytest.raises(DbeelGpuError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _state(rd, keys=POOL):
    """Everything a refused or empty call must leave as it was."""
    hits, voff, values, _ = rd.get_raw(keys)
    return (rd.memtable_info, rd.memtable_fetch(), hits.tobytes(),
            voff.tobytes(), values.tobytes())


def _assert_memtable(rd, model):
    info = rd.memtable_info
    assert info["entries"] == model.entries
    assert info["data_bytes"] == model.data_bytes
    assert rd.memtable_fetch() == model.run()


def _put_entries(rd, model, writes, rids=None, take=None, delete_ts=None):
    """One put_entries on both sides; stats and bytes against the model."""
    d, x = encode_page(writes)
    before = model.entries
    exp = migrate_model.apply(
        model, writes, rids, take, PUT if delete_ts is None else DELETE,
        delete_ts)
    st = rd.put_entries(
        d, x, None if rids is None else np.asarray(rids, dtype=np.uint32),
        None if take is None else np.asarray(take, dtype=np.uint8),
        delete_ts=delete_ts)
    assert st["entries_in"] == len(writes)
    assert st["selected"] == len(migrate_model.selected(writes, rids, take))
    if exp is not None:
        assert st["batch_entries"] == exp[0]
        assert st["replaced"] == exp[1]
        assert st["entries"] == model.entries == before + exp[0] - exp[1]
        assert st["data_bytes"] == model.data_bytes
    _assert_memtable(rd, model)
    return st


# ---- 1. parity ----

@pytest.mark.parametrize("start", ["empty", "nonempty"])
def test_parity_chain(order, start):
    """Into an empty and a non-empty memtable, then a second page: the bytes
    are the model's, and those of a second reader fed the decoded writes
    through put."""
    model = Memtable()
    with Reader(_base(), device=0) as rd, Reader(_base(), device=0) as ref:
        if start == "nonempty":
            w0 = gen(3, 80, POOL)
            model.put(w0)
            rd.put(w0)
            ref.put(w0)
        for seed, n in ((4, 200), (5, 150)):
            writes = gen(seed, n, POOL)
            st = _put_entries(rd, model, writes)
            assert st["prefix_tied"] == batch_model.prefix_tied(writes)
            d, x = encode_page(writes)
            ref.put(decode_page(d, x))
            assert rd.memtable_fetch() == ref.memtable_fetch()
            assert rd.memtable_info["puts"] == ref.memtable_info["puts"]
        with Reader(_base() + [model.run()], device=0) as fresh:
            assert rd.get(POOL) == fresh.get(POOL)
            assert rd.get_entries(POOL) == fresh.get_entries(POOL)


# ---- 2. shapes: the smallest at which each stage can go wrong ----

def _shape_cases():
    rng = np.random.default_rng(21)
    rb = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    klens = list(range(0, 10)) + [15, 16, 17]
    vlens = [0, 1, 7, 8, 9, 15, 16, 17]
    shared = b"prefix8!"
    return {
        "single": [(b"k", b"v", 1)],
        "single_empty_key_tombstone": [(b"", b"", -1)],
        "key_lengths": [(b"K" * n, rb(5), n) for n in klens],
        "value_lengths": [(b"v%02d" % n, rb(n), -n) for n in vlens],
        "value_200000": [(b"a", b"x", 1), (b"big", rb(200_000), 2),
                         (b"c", b"y", 3)],
        "zero_padding": [(b"ab\0\0", b"3", 3), (b"ab", b"1", 1),
                         (b"ab\0", b"2", 2), (b"ab\0\0", b"4", 0)],
        "shared_prefix_64": [(shared + rb(int(rng.integers(0, 6))), rb(3), i)
                             for i in range(64)],
        "one_key_5_descending": [(b"same", b"v%d" % i, 100 - i)
                                 for i in range(5)],
        "extreme_timestamps": [(b"lo", b"1", I128_MIN), (b"hi", b"2", I128_MAX),
                               (b"lo", b"", I128_MAX), (b"z", b"3", -1),
                               (b"hi", b"4", I128_MIN)],
        "only_tombstones": [(k, b"", i) for i, k in enumerate(POOL[:40])],
    }


SHAPES = _shape_cases()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(order, name):
    """Each shape into an empty memtable and again on top of puts."""
    writes = SHAPES[name]
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        _put_entries(rd, model, writes)
        model2 = Memtable()
        rd.memtable_clear()
        w0 = gen(6, 60, POOL) + [(b"ab", b"old", 5), (b"same", b"old", 6)]
        model2.put(w0)
        rd.put(w0)
        _put_entries(rd, model2, writes)
        keys = sorted({w[0] for w in writes})
        with Reader(_base() + [model2.run()], device=0) as fresh:
            assert rd.get_entries(keys) == fresh.get_entries(keys)


def test_every_entry_repeats_a_held_key(order):
    """replaced is the model's count when the whole page overwrites."""
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        w0 = [(k, b"first", 1) for k in POOL[:50]]
        model.put(w0)
        rd.put(w0)
        page = [(k, b"second" + k[:2], -i) for i, k in enumerate(POOL[:50])]
        page += page[:10]
        st = _put_entries(rd, model, page)
        assert st["replaced"] == 50 and st["batch_entries"] == 50
        assert st["entries"] == 50


# ---- 3. selection ----

def test_take_selecting_nothing_is_a_noop():
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        w0 = gen(7, 40, POOL)
        model.put(w0)
        rd.put(w0)
        before = _state(rd)
        writes = gen(8, 30, POOL)
        rids = [i % 4 for i in range(30)]
        st = _put_entries(rd, model, writes, rids, [0, 0, 0, 0])
        assert st["selected"] == 0 and st["entries"] == model.entries
        assert _state(rd) == before  # puts included
        # ... and into an empty memtable
        rd.memtable_clear()
        st = rd.put_entries(*encode_page(writes),
                            np.asarray(rids, dtype=np.uint32),
                            np.zeros(4, dtype=np.uint8))
        assert st["selected"] == 0
        assert rd.memtable_info["puts"] == 0 == rd.memtable_info["entries"]


def test_mask_selects_ids_0_and_2_of_4(order):
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        writes = gen(9, 120, POOL)
        rids = [int(r) for r in
                np.random.default_rng(9).integers(0, 4, len(writes))]
        st = _put_entries(rd, model, writes, rids, [1, 0, 7, 0])
        assert 0 < st["selected"] < len(writes)
        # a later unselected arrival of a key must not beat a selected one
        page = [(b"dup", b"selected", 1), (b"dup", b"unselected", 2)]
        _put_entries(rd, model, page, [0, 1], [1, 0, 1, 0])
        assert rd.get([b"dup"]) == [b"selected"]


def test_selected_id_past_n_take_is_invalid_arg():
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        w0 = gen(10, 40, POOL)
        model.put(w0)
        rd.put(w0)
        before = _state(rd)
        d, x = encode_page(gen(12, 20, POOL))
        rids = np.zeros(20, dtype=np.uint32)
        rids[13] = 4
        assert _code(rd.put_entries, d, x, rids,
                     np.ones(4, dtype=np.uint8)) == INVALID_ARG
        assert _state(rd) == before
        _assert_memtable(rd, model)


# ---- 4. DELETE ----

@pytest.mark.parametrize("dts", [12345, -1, I128_MIN, I128_MAX])
def test_delete(order, dts):
    """Tombstones carry delete_ts; a key repeated in the page gives one; the
    24-byte record comes back from get_entries; a flush keeps it all."""
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        w0 = gen(13, 50, POOL)
        model.put(w0)
        rd.put(w0)
        page = gen(14, 60, POOL[::2]) + [(POOL[2], b"again", 9)] * 3
        rids = [i % 3 for i in range(len(page))]
        st = _put_entries(rd, model, page, rids, [1, 0, 1], delete_ts=dts)
        gone = sorted({w[0] for w, r in zip(page, rids) if r != 1})
        assert st["batch_entries"] == len(gone)
        assert rd.get_entries(gone) == [(b"", dts)] * len(gone)
        hits, roff, view, _, _ = rd.get_entries_raw(gone[:1])
        assert int(roff[1] - roff[0]) == 24
        assert view.tobytes()[:24] == bytes(8) + dts.to_bytes(
            16, "little", signed=True)
        # no mask: every entry
        _put_entries(rd, model, page, delete_ts=dts)
        answers = rd.get_entries(POOL)
        data, index, _ = rd.memtable_flush(fetch=True)
        assert (data, index) == model.run()
        assert rd.get_entries(POOL) == answers
        with Reader(_base() + [(data, index)], device=0) as fresh:
            assert fresh.get_entries(POOL) == answers


# ---- 5. refused pages ----

def _corrupt_pages():
    writes = [(b"key%d" % i, b"value%d" % i, i) for i in range(6)]
    d, x = encode_page(writes)
    rec = lambda a: a.view(engine.INDEX_DTYPE)
    out = {}
    a = x.copy()
    rec(a)["offset"][4] = len(d) + 1
    out["offset_past_data_len"] = (d, a)
    a = x.copy()
    rec(a)["key_size"][2] = 7
    out["key_size_below_8"] = (d, a)
    a = x.copy()
    rec(a)["key_size"][3] -= 1  # the entry's own klen field now disagrees
    out["klen_field_disagrees"] = (d, a)
    a = x.copy()
    rec(a)["offset"][5] -= 3    # starts inside its predecessor
    out["offset_overlaps_predecessor"] = (d, a)
    return out


CORRUPT_PAGES = _corrupt_pages()


@pytest.mark.parametrize("name", sorted(CORRUPT_PAGES))
@pytest.mark.parametrize("mode", [PUT, DELETE])
def test_refused_pages(name, mode):
    """Rejection tests like the suite's corrupt-run cases, not fault probes:
    every page here is caught by load_entry (offset past data_len,
    key_size < 8) or entry_consistent (klen field against the index record,
    successor offset) in the stage kernel BEFORE anything is read through
    the entry, the host reads the verdict before any later kernel is
    launched, and every offset and size stays inside the uploaded page."""
    d, x = CORRUPT_PAGES[name]
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        w0 = gen(15, 40, POOL)
        model.put(w0)
        rd.put(w0)
        before = _state(rd)
        kw = {} if mode == PUT else {"delete_ts": 5}
        assert _code(rd.put_entries, d, x, **kw) == CORRUPT
        # unselected entries are validated too
        assert _code(rd.put_entries, d, x, np.zeros(6, dtype=np.uint32),
                     np.zeros(1, dtype=np.uint8), **kw) == CORRUPT
        assert _state(rd) == before
        _assert_memtable(rd, model)


def test_host_refusals_with_a_live_reader():
    """The header's order past the NULL reader, with nothing changed."""
    import ctypes

    lib = engine._load_reader()
    d, x = encode_page([(b"k", b"v", 1)])
    rid = np.zeros(1, dtype=np.uint32)
    take = np.ones(1, dtype=np.uint8)
    ts = np.zeros(16, dtype=np.uint8)
    with Reader(_base(), device=0) as rd:
        before = _state(rd)

        def call(**kw):
            a = dict(data=d.ctypes.data, index=x.ctypes.data, n=1,
                     rids=rid.ctypes.data, take=take.ctypes.data, n_take=1,
                     mode=1, dts=ts.ctypes.data)
            a.update(kw)
            rc = lib.dbeel_gpu_reader_put_entries(
                rd._h, a["data"], d.nbytes, a["index"], a["n"], a["rids"],
                a["take"], a["n_take"], a["mode"], a["dts"], None)
            return rc, lib.dbeel_gpu_last_error()

        for kw, word in ((dict(data=None, mode=0), b"null data"),
                         (dict(index=None, mode=9), b"null data"),
                         (dict(mode=0, dts=None, take=None), b"mode"),
                         (dict(mode=2, dts=None, take=None), b"delete_ts"),
                         (dict(take=None, n=1 << 31), b"take"),
                         (dict(n_take=0, n=1 << 31), b"take"),
                         (dict(n=1 << 31), b"2^31 - 1 per page")):
            rc, msg = call(**kw)
            assert rc == INVALID_ARG and word in msg, (kw, msg)
        # memtable entries + page entries: refused on the host as well
        rd.put([(b"held", b"v", 1)])
        before = _state(rd)
        rc, msg = call(n=(1 << 31) - 1)
        assert rc == INVALID_ARG and b"together" in msg, msg
        assert call(n=0, data=None, index=None)[0] == 0
        assert _state(rd) == before


# ---- 6. scan_apply ----

Q = 1 << 30
RANGES = [(0, Q), (Q, 2 * Q), (2 * Q, 3 * Q), (3 * Q, 0xFFFFFFFF)]
DTS = 777_000_000_000
_SRC = None


def _source():
    """-> (3 tables with overlapping keys, memtable writes); every hash
    range holds keys of every segment's pool (checked with pymm3)."""
    global _SRC
    if _SRC is None:
        tables = [batch_model.flush_run(gen(31, 150, POOL[:110])),
                  batch_model.flush_run(gen(32, 120, POOL[40:])),
                  batch_model.flush_run(gen(33, 100, POOL[::2]))]
        mem = gen(34, 70, POOL[20:140])
        _SRC = (tables, mem)
        keys = {w[0] for w in mem}
        for j, (a, b) in enumerate(RANGES):
            assert any(between_cmp(murmur3_32(k, 0), a, b) for k in keys), j
    return _SRC


def _yielded(tables, mem_run, memtable, newest_only, ranges=RANGES):
    """The scan's entries in yield order with their first range ids."""
    segs = snapshot_model.segments(tables, mem_run if memtable else None)
    model = snapshot_model.snapshot_model(segs, hash_ranges=ranges,
                                          newest_only=newest_only)
    page = decode_page(model[0], model[1])
    rids = (snapshot_model.first_range_ids(model, ranges) if ranges
            else None)
    return page, rids


def _drain(sc, actions, page_bytes, **kw):
    pages = 0
    tot = {"put_entries": 0, "delete_entries": 0, "skipped": 0, "groups": 0}
    while True:
        pg, st = sc.apply(actions, page_bytes, **kw)
        assert pg["d2h_ms"] == 0
        pages += 1
        for k in tot:
            tot[k] += st[k]
        if pg["done"]:
            return pages, tot


@pytest.mark.parametrize("flags", ["plain", "newest_memtable"])
def test_scan_apply_four_actions(order, flags):
    """[put->A, delete->source, skip, put->B] over 3 tables + memtable in
    many small pages: A, B and the source's tombstones are the model's, and
    A and B equal the host route (scan_next + put_entries, same masks) byte
    for byte."""
    tables, mem = _source()
    newest = flags == "newest_memtable"
    memtable = True
    src_model = Memtable()
    src_model.put(mem)
    page, rids = _yielded(tables, src_model.run(), memtable, newest)
    assert len(set(rids)) == 4
    with Reader(tables, device=0) as src, Reader(DEST, device=0) as A, \
            Reader(_base(), device=0) as B, Reader(DEST, device=0) as A2, \
            Reader(_base(), device=0) as B2:
        src.put(mem)
        actions = [("put", A), ("delete", src), ("skip",), ("put", B)]
        sc = src.snapshot_open(hash_ranges=RANGES, max_candidates=64,
                               memtable=memtable, newest_only=newest)
        pages, tot = _drain(sc, actions, 4096, delete_ts=DTS)
        sc.close()
        assert pages > 4
        mems = migrate_model.migrate(
            [(page, rids)],
            [("put", "A"), ("delete", "S"), ("skip",), ("put", "B")], DTS)
        assert tot["put_entries"] == (len(mems["A"].arrivals)
                                      + len(mems["B"].arrivals))
        assert tot["delete_entries"] == len(mems["S"].arrivals)
        assert tot["skipped"] == sum(1 for r in rids if r == 2)
        _assert_memtable(A, mems["A"])
        _assert_memtable(B, mems["B"])
        src_model.put(mems["S"].arrivals)
        _assert_memtable(src, src_model)
        deleted = sorted({w[0] for w in mems["S"].arrivals})
        assert src.get_entries(deleted) == [(b"", DTS)] * len(deleted)
        assert src.held_bytes == 0
        # the host route
        data = np.empty(4096, dtype=np.uint8)
        index = np.empty(16 * 128, dtype=np.uint8)
        rid = np.empty(128, dtype=np.uint32)
        with Reader(tables, device=0) as src2:
            src2.put(mem)
            sc = src2.snapshot_open(hash_ranges=RANGES, max_candidates=64,
                                    memtable=memtable, newest_only=newest)
            while True:
                pg = sc.next(data, index, rid)
                n = pg["n_entries"]
                if n:
                    args = (data[:pg["data_len"]], index[:16 * n], rid[:n])
                    A2.put_entries(*args, np.array([1, 0, 0, 0], np.uint8))
                    B2.put_entries(*args, np.array([0, 0, 0, 1], np.uint8))
                if pg["done"]:
                    break
            sc.close()
        assert A.memtable_fetch() == A2.memtable_fetch()
        assert B.memtable_fetch() == B2.memtable_fetch()


def test_plain_and_newest_only_destinations_answer_alike():
    tables, mem = _source()
    got = []
    for newest in (False, True):
        with Reader(tables, device=0) as src, Reader(DEST, device=0) as A:
            src.put(mem)
            st = src.migrate([("put", A)] * 4, hash_ranges=RANGES,
                             flags=engine.SCAN_MEMTABLE
                             | (engine.SCAN_NEWEST_ONLY if newest else 0),
                             page_bytes=4096, max_candidates=64)
            assert st["pages"] > 4 and st["skipped"] == 0
            assert st["groups"] <= st["pages"]
            assert src.held_bytes == 0
            got.append((A.get_entries(POOL), A.memtable_fetch()))
    assert got[0] == got[1]
    with Reader(tables, device=0) as fresh:
        fresh.put(mem)
        keys = [k for k in POOL
                if any(between_cmp(murmur3_32(k, 0), a, b)
                       for a, b in RANGES)]
        with Reader([got[0][1]], device=0) as dest:
            assert dest.get_entries(keys) == fresh.get_entries(keys)


def test_scan_without_hash_ranges_takes_one_action(order):
    tables, mem = _source()
    with Reader(tables, device=0) as src, Reader(DEST, device=0) as A:
        sc = src.scan_open(max_candidates=64)
        assert _code(sc.apply, [("put", A)] * 2, 4096) == INVALID_ARG
        _drain(sc, [("put", A)], 4096)
        sc.close()
        page, _ = _yielded(tables, None, False, False, ranges=None)
        model = Memtable()
        model.put(page)
        _assert_memtable(A, model)
        # ... and one SKIP action moves nothing
        sc = src.scan_open(max_candidates=64)
        pages, tot = _drain(sc, [("skip",)], 4096)
        sc.close()
        assert tot["groups"] == 0 and tot["skipped"] == len(page)
        _assert_memtable(A, model)


def test_item_too_large_then_a_larger_page():
    big = bytes(np.random.default_rng(5).integers(0, 256, 200_000,
                                                  dtype=np.uint8))
    run = batch_model.flush_run([(b"a", b"1", 1), (b"big", big, 2),
                                 (b"c", b"3", 3)])
    with Reader([run], device=0) as src, Reader(DEST, device=0) as A:
        sc = src.scan_open()
        pg, st = sc.apply([("put", A)], 4096)
        assert pg["n_entries"] == 1 and not pg["done"]
        with pytest.raises(DbeelGpuError) as ei:
            sc.apply([("put", A)], 4096)
        assert ei.value.code == ITEM_TOO_LARGE
        assert ei.value.page["needed"] == 32 + 3 + 200_000
        assert A.memtable_info["entries"] == 1  # nothing applied
        assert A.memtable_info["puts"] == 1
        # the cursor has not moved: a larger page takes the entry
        pg, st = sc.apply([("put", A)], ei.value.page["needed"])
        assert pg["n_entries"] == 1 and st["put_entries"] == 1
        pg, st = sc.apply([("put", A)], 4096)
        assert pg["done"]
        sc.close()
        assert A.memtable_fetch() == run


def test_host_refusals_leave_the_cursor():
    tables, mem = _source()
    with Reader(tables, device=0) as src, Reader(DEST, device=0) as A:
        def rest(sc):
            out = []
            data = np.empty(1 << 20, dtype=np.uint8)
            index = np.empty(16 * 4096, dtype=np.uint8)
            while True:
                pg = sc.next(data, index)
                out.append((data[:pg["data_len"]].tobytes(),
                            index[:16 * pg["n_entries"]].tobytes()))
                if pg["done"]:
                    return out

        sc0 = src.snapshot_open(hash_ranges=RANGES[:2], max_candidates=64)
        sc0.apply([("skip",), ("skip",)], 4096)
        expect = rest(sc0)
        sc0.close()

        sc = src.snapshot_open(hash_ranges=RANGES[:2], max_candidates=64)
        sc.apply([("skip",), ("skip",)], 4096)
        ok = [("put", A), ("skip",)]
        for bad in (dict(actions=ok[:1]), dict(actions=ok + ok),
                    dict(actions=[(7, A), ("skip",)]),
                    dict(actions=[("put", None), ("skip",)]),
                    dict(actions=[("delete", None), ("skip",)],
                         delete_ts=1),
                    dict(actions=[("delete", A), ("skip",)]),
                    dict(page_bytes=0), dict(page_entries=0)):
            kw = dict(actions=ok, page_bytes=4096)
            kw.update(bad)
            assert _code(sc.apply, **kw) == INVALID_ARG, bad
        assert A.memtable_info["puts"] == 0
        assert rest(sc) == expect
        sc.close()
        # a stale scan: the list changed under a plain scan
        sc = src.scan_open(hash_ranges=RANGES[:2])
        src.insert_run(0, _base()[0])
        assert _code(sc.apply, ok, 4096) == INVALID_ARG
        sc.close()
        assert A.memtable_info["puts"] == 0
        assert src.held_bytes == 0


def test_put_into_the_scans_own_reader(order):
    """dst == the scan's reader under PUT: the snapshot (memtable segment
    included) holds its buffers, the memtable grows under it."""
    tables, mem = _source()
    model = Memtable()
    model.put(mem)
    page, _ = _yielded(tables, model.run(), True, False, ranges=None)
    with Reader(tables, device=0) as src:
        src.put(mem)
        st = src.migrate([("put", src)], page_bytes=4096, max_candidates=64)
        assert st["put_entries"] == len(page) and st["pages"] > 4
        model.put(page)
        _assert_memtable(src, model)
        assert src.held_bytes == 0


# ---- 7. the shared merge helper, through the untouched put ----

def test_put_and_flush_after_put_entries(order):
    model = Memtable()
    with Reader(_base(), device=0) as rd:
        _put_entries(rd, model, gen(41, 90, POOL))
        _put_entries(rd, model, gen(42, 40, POOL), delete_ts=-3)
        w = gen(43, 110, POOL)
        batch_entries, replaced = model.put(w)
        st = rd.put(w)
        assert (st["batch_entries"], st["replaced"]) == (batch_entries,
                                                         replaced)
        assert st["entries"] == model.entries
        _assert_memtable(rd, model)
        data, index, _ = rd.memtable_flush(fetch=True)
        assert (data, index) == model.run()
        assert rd.memtable_info["entries"] == 0
        with Reader(_base() + [model.run()], device=0) as fresh:
            assert rd.get_entries(POOL) == fresh.get_entries(POOL)
