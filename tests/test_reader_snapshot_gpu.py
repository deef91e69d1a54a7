"""GPU tests of the snapshot scan (engine.Reader.snapshot / snapshot_pages /
snapshot_open, include/dbeel_gpu.h dbeel_gpu_reader_scan_snapshot): the
memtable as the last segment, scans that survive every edit of the reader,
NEWEST_ONLY's shadow pass in both variants, the 65-segment boundary, and the
held-bytes accounting.

The host model is snapshot_model (pymm3.scan_model over tables + memtable run;
newest_only drops an entry whose key a later segment holds). Every comparison
is byte equality of data, rebased index and range ids.
"""
import numpy as np
import pytest

import memtable_model
import snapshot_model as sm
from dbeel_amd.engine import DbeelGpuError, Job, Reader
from dbeel_amd.format import INDEX_DTYPE, Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs

pytestmark = pytest.mark.gpu

INVALID_ARG = 1

PLAIN = [(1 << 28, 1 << 30), (3 << 30, (3 << 30) + (1 << 29))]
WRAPPED = [(1 << 30, 2 << 30), (3 << 30, 1 << 28)]  # second one wraps

FILTER_NAMES = ["none", "keyrange", "hash", "hash_wrapped", "both",
                "both_wrapped"]

# (page_bytes, page_entries, max_candidates): one large page, then small ones
BIG = (1 << 22, 1 << 15, 0)
SHAPES = {"big": BIG, "mc7": (1 << 22, 1 << 15, 7),
          "mc64": (1 << 22, 1 << 15, 64), "pe5": (1 << 22, 5, 0)}


def _filters(keys):
    keys = sorted(keys)
    krange = dict(start_key=keys[int(0.3 * len(keys))],
                  end_key=keys[int(0.7 * len(keys))])
    return {
        "none": {},
        "keyrange": krange,
        "hash": dict(hash_ranges=PLAIN),
        "hash_wrapped": dict(hash_ranges=WRAPPED),
        "both": dict(krange, hash_ranges=PLAIN),
        "both_wrapped": dict(krange, hash_ranges=WRAPPED),
    }


def _paged(rd, kw, shape, memtable=False, newest_only=False, between=None,
           opener=None):
    """Drive one snapshot scan page by page. Returns (data, index, n, ids,
    pages, info): the concatenation with offsets rebased, the range ids, the
    per-page dicts and the scan's info after the last page. between(page_no)
    runs after each page."""
    pb, pe, mc = shape
    data = np.empty(pb, dtype=np.uint8)
    index = np.empty(pe * 16, dtype=np.uint8)
    rid = np.empty(pe, dtype=np.uint32) if kw.get("hash_ranges") else None
    datas, recs, rids, pages = [], [], [], []
    off = 0
    sc = (opener() if opener else
          rd.snapshot_open(max_candidates=mc, memtable=memtable,
                           newest_only=newest_only, **kw))
    with sc:
        while True:
            pg = sc.next(data, index, rid)
            pages.append(pg)
            n = pg["n_entries"]
            assert n <= pe and pg["data_len"] <= pb and pg["needed"] == 0
            if n:
                rec = index[:n * 16].view(INDEX_DTYPE).copy()
                ends = np.cumsum(rec["full_size"].astype(np.uint64))
                assert rec["offset"][0] == 0
                assert np.array_equal(rec["offset"][1:], ends[:-1])
                assert int(ends[-1]) == pg["data_len"]
                rec["offset"] += np.uint64(off)
                off += pg["data_len"]
                recs.append(rec.tobytes())
                datas.append(data[:pg["data_len"]].tobytes())
                if rid is not None:
                    rids.append(rid[:n].copy())
            if between is not None:
                between(len(pages))
            if pg["done"]:
                break
            assert len(pages) < 100000
        pg = sc.next(data, index, rid)  # a finished scan stays finished
        assert pg["done"] == 1 and pg["n_entries"] == 0
        info = sc.info()
    ids = (np.concatenate(rids).tolist() if rids else [])
    ib = b"".join(recs)
    return b"".join(datas), ib, len(ib) // 16, ids, pages, info


def _check(got, segs, kw, newest_only):
    """got = _paged's result; segs = the snapshot's segments."""
    d, i, n, ids, pages, info = got
    md, mi, mn = sm.snapshot_model(segs, newest_only=newest_only, **kw)
    assert (n, i, d) == (mn, mi, md)
    if kw.get("hash_ranges"):
        assert ids == sm.first_range_ids((md, mi, mn), kw["hash_ranges"])
    in_range = sm.scan_model(segs, kw.get("start_key"), kw.get("end_key"))[2]
    assert sum(p["candidates"] for p in pages) == in_range
    assert (info["table_candidates"] + info["memtable_candidates"]
            == in_range)
    assert info["shadowed"] == (sm.shadowed_count(segs, **kw)
                                if newest_only else 0)


def _puts(keys, seed, n=200):
    """n puts over the key population (repeats, ~15 % tombstones) and a few
    keys no table holds, in two batches."""
    pool = sorted(keys)[::3] + [b"", b"zz-new-1", b"zz-new-2"]
    w = memtable_model.gen(seed, n, pool)
    return [w[:n // 2], w[n // 2:]]


class _Base:
    def __init__(self):
        runs = make_runs(4, 300, 16, 64, overlap_frac=0.5,
                         tombstone_frac=0.15, seed=71)
        self.runs = [(bytes(d), bytes(i)) for d, i in runs]
        self.keys = sorted({e.key for d, i in self.runs
                            for e in parse_run(d, i)})
        self.filters = _filters(self.keys)
        self.batches = _puts(self.keys, 5)
        mt = memtable_model.Memtable()
        for b in self.batches:
            mt.put(b)
        self.mem_run = mt.run()
        self.segs = sm.segments(self.runs, self.mem_run)
        self.plain = Reader(self.runs, device=0)      # empty memtable
        self.reader = Reader(self.runs, device=0)     # tables + memtable
        for b in self.batches:
            self.reader.put(b)

    def fresh(self):
        rd = Reader(self.runs, device=0)
        for b in self.batches:
            rd.put(b)
        return rd

    def close(self):
        self.plain.close()
        self.reader.close()


@pytest.fixture(scope="module")
def base():
    b = _Base()
    yield b
    b.close()


@pytest.fixture(params=["narrow", "full"])
def variant(request, monkeypatch):
    """Both shadow-pass variants; the switch is read on every page."""
    monkeypatch.setenv("DBEEL_SCAN_SHADOW", request.param)
    return request.param


# ---- 1. flags == 0 is the old scan ----

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_flags0_equals_scan(base, name, shape):
    kw = base.filters[name]
    for rd in (base.plain, base.reader):  # the memtable neither appears
        want = rd.scan(return_range_ids=True, **kw)
        d, i, n, ids, pages, info = _paged(rd, kw, SHAPES[shape])
        assert (d, i, n) == want[:3]
        assert ids == want[3].tolist()
        assert info["has_memtable"] == 0 and info["n_tables"] == 4
        assert info["memtable_candidates"] == 0 and info["shadowed"] == 0
    pb, pe, mc = SHAPES[shape]
    assert base.plain.snapshot(page_bytes=pb, page_entries=pe,
                               max_candidates=mc, **kw) == want[:3]


def test_old_scan_info(base):
    with base.reader.scan_open() as sc:
        info = sc.info()
    total = sum(len(i) // 16 for _, i in base.runs)
    assert info == dict(n_tables=4, has_memtable=0, table_candidates=total,
                        memtable_candidates=0, shadowed=0)


# ---- 2. the memtable as the last segment ----

def test_memtable_run_is_the_model(base):
    assert base.reader.memtable_fetch() == base.mem_run
    assert len(base.mem_run[1]) // 16 >= 60


@pytest.mark.parametrize("mode", ["all", "newest-narrow", "newest-full"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_memtable_segment(base, name, shape, mode, monkeypatch):
    newest = mode != "all"
    if newest:
        monkeypatch.setenv("DBEEL_SCAN_SHADOW", mode.split("-")[1])
    kw = base.filters[name]
    got = _paged(base.reader, kw, SHAPES[shape], memtable=True,
                 newest_only=newest)
    _check(got, base.segs, kw, newest)
    info = got[5]
    assert info["has_memtable"] == 1 and info["n_tables"] == 4
    assert info["table_candidates"] == sm.scan_model(
        base.runs, kw.get("start_key"), kw.get("end_key"))[2]
    assert info["memtable_candidates"] == sm.scan_model(
        [base.mem_run], kw.get("start_key"), kw.get("end_key"))[2]
    # no page mixes table entries with memtable entries
    seen = 0
    for p in got[4]:
        assert (seen + p["candidates"] <= info["table_candidates"]
                or seen >= info["table_candidates"])
        seen += p["candidates"]


@pytest.mark.parametrize("name", FILTER_NAMES)
def test_empty_memtable_changes_nothing(base, name):
    kw = base.filters[name]
    a = _paged(base.plain, kw, SHAPES["mc64"], memtable=True)
    b = _paged(base.plain, kw, SHAPES["mc64"])
    assert a[:4] == b[:4] and a[5] == b[5]
    assert a[5]["has_memtable"] == 0


@pytest.mark.parametrize("newest", [False, True], ids=["all", "newest"])
def test_no_table_entries_only_memtable(base, newest):
    # a reader cannot be opened over zero runs, and no edit empties the
    # list: one table without entries is the nearest state there is
    with Reader([(b"", b"")], device=0) as rd:
        for b in base.batches:
            rd.put(b)
        for name in FILTER_NAMES:
            kw = base.filters[name]
            for shape in ("big", "mc7", "pe5"):
                got = _paged(rd, kw, SHAPES[shape], memtable=True,
                             newest_only=newest)
                _check(got, [base.mem_run], kw, newest)
                assert got[5]["n_tables"] == 1
                assert got[5]["table_candidates"] == 0
                # the memtable segment starts with the first page
                assert got[4][0]["n_entries"] or not got[2]
        # without the flag there is nothing to yield
        assert rd.snapshot() == (b"", b"", 0)


# ---- 3. a snapshot survives every edit ----

def _new_run(base, seed):
    rng = np.random.default_rng(seed)
    ks = [base.keys[int(j)] for j in
          sorted(set(rng.integers(0, len(base.keys), 40).tolist()))]
    return build_run([Entry(k, b"new%d" % seed, 7) for k in ks])


def _edit_insert(base, rd):
    rd.insert_run(1, _new_run(base, 1))


def _edit_write_batch(base, rd):
    rd.write_batch(memtable_model.gen(9, 50, base.keys[::5]))


def _edit_put_twice(base, rd):
    # the first put leaves the held buffer as the spare, the second would
    # write into it
    rd.put(memtable_model.gen(10, 30, base.keys[::7]))
    rd.put(memtable_model.gen(11, 30, base.keys[::11]))


def _edit_flush(base, rd):
    rd.memtable_flush()
    rd.put(memtable_model.gen(12, 30, base.keys[::7]))
    rd.put(memtable_model.gen(13, 30, base.keys[::11]))


def _edit_clear(base, rd):
    rd.memtable_clear()
    rd.put(memtable_model.gen(14, 30, base.keys[::7]))
    rd.put(memtable_model.gen(15, 30, base.keys[::11]))


def _edit_compact(base, rd):
    rd.compact([1, 2], 1, keep_tombstones=False)


def _edit_compact_abort(base, rd):
    rd.compact_begin([0, 3], keep_tombstones=True)
    rd.compact_abort()


# name -> (edit, does the old scan go stale)
EDITS = {
    "insert_run": (_edit_insert, True),
    "write_batch": (_edit_write_batch, True),
    "put_twice": (_edit_put_twice, False),
    "memtable_flush": (_edit_flush, True),
    "memtable_clear": (_edit_clear, False),
    "compact": (_edit_compact, True),
    "compact_abort": (_edit_compact_abort, False),
}


def _old_scan_state(sc):
    data = np.empty(1 << 16, dtype=np.uint8)
    index = np.empty(16 * 64, dtype=np.uint8)
    try:
        sc.next(data, index)
        return "live"
    except DbeelGpuError as e:
        assert e.code == INVALID_ARG and "stale" in str(e)
        return "stale"


@pytest.mark.parametrize("edit", list(EDITS) + ["all"])
def test_survives_edits(base, edit, variant):
    rd = base.fresh()
    try:
        kw = base.filters["both"]
        shape = (1 << 22, 1 << 15, 32)
        todo = list(EDITS) if edit == "all" else [edit]
        stale = any(EDITS[e][1] for e in todo)
        old = rd.scan_open(max_candidates=64)
        assert _old_scan_state(old) == "live"

        def between(page_no):
            # one edit after each of the first pages
            if page_no <= len(todo):
                EDITS[todo[page_no - 1]][0](base, rd)

        got = _paged(rd, kw, shape, memtable=True, newest_only=True,
                     between=between)
        assert len(got[4]) > len(todo)  # pages were left after the edits
        _check(got, base.segs, kw, True)
        assert _old_scan_state(old) == ("stale" if stale else "live")
        old.close()
        assert rd.held_bytes == 0
        # and the plain snapshot, edited under, too
        rd2 = base.fresh()
        try:
            def between2(page_no):
                if page_no <= len(todo):
                    EDITS[todo[page_no - 1]][0](base, rd2)
            got = _paged(rd2, {}, shape, memtable=True, between=between2)
            _check(got, base.segs, {}, False)
        finally:
            rd2.close()
    finally:
        rd.close()


# ---- 4. 64 tables + the memtable = 65 segments ----

def test_65_segments(variant):
    runs = []
    for r in range(64):
        es = [Entry(b"shared", b"t%02d" % r, r)]
        if r == 0:
            es.append(Entry(b"only0", b"x", 1))
        elif r % 2 == 0:
            es.append(Entry(b"k%02d" % r, b"v", r))
        runs.append(build_run(sorted(es, key=lambda e: e.key)))
    writes = [(b"shared", b"from-mem", 0), (b"onlymem", b"m", 0)]
    mem_run = memtable_model.batch_model.flush_run(writes)
    segs = sm.segments(runs, mem_run)
    assert len(segs) == 65
    with Reader(runs, device=0) as rd:
        rd.put(writes)
        assert rd.n_runs == 64
        for shape in ("big", "mc7", "pe5"):
            got = _paged(rd, {}, SHAPES[shape], memtable=True)
            _check(got, segs, {}, False)
            info = got[5]
            assert info["n_tables"] == 64 and info["has_memtable"] == 1
            assert info["memtable_candidates"] == 2
        # one roomy page cannot take all 65: the boundary page is short
        pages = _paged(rd, {}, BIG, memtable=True)[4]
        assert len(pages) == 2
        assert pages[0]["candidates"] == info["table_candidates"]
        assert pages[0]["done"] == 0 and pages[1]["n_entries"] == 2
        for shape in ("big", "mc7", "pe5"):
            got = _paged(rd, {}, SHAPES[shape], memtable=True,
                         newest_only=True)
            _check(got, segs, {}, True)
            es = parse_run(got[0], got[1])
            shared = [e for e in es if e.key == b"shared"]
            assert [e.data for e in shared] == [b"from-mem"]
            assert {b"only0", b"onlymem"} <= {e.key for e in es}
            assert got[5]["shadowed"] == 64
        # without the memtable flag table 63's version is the last one
        got = _paged(rd, {}, BIG, newest_only=True)
        _check(got, sm.segments(runs), {}, True)
        assert [e.data for e in parse_run(got[0], got[1])
                if e.key == b"shared"] == [b"t63"]


# ---- 5. NEWEST_ONLY shapes ----

def _run_bloom(run):
    with Job([run], device=0) as job:
        job.run(True)
        return job.bloom()


class _Shapes:
    """Four crafted tables (filters on 1 and 3) + a memtable."""

    def __init__(self):
        rng = np.random.default_rng(17)
        pool = sorted({bytes(rng.integers(97, 123, int(rng.integers(3, 20)),
                                          dtype=np.uint8))
                       for _ in range(700)})
        tied = [b"SAMEPFX8" + b"%03d" % j for j in range(60)]
        t = [dict() for _ in range(4)]

        def put(r, k, v, ts=1):
            t[r][k] = Entry(k, v, ts)

        for r in range(4):  # filler with heavy overlap; > 256 per table
            for j in rng.permutation(len(pool))[:330].tolist():
                put(r, pool[j], b"" if rng.random() < 0.15 else b"f%d" % r)
        # a stretch of 40 keys equal in the first 8 bytes in the LATER table
        for k in tied:
            put(0, k, b"old")
        for j, k in enumerate(tied):
            if j % 3:
                put(2, k, b"newer")
        # proper prefix: b"ab" vs b"abc"; only the equal key shadows
        put(0, b"ab", b"0")
        put(1, b"abc", b"1")
        put(3, b"ab", b"3")
        put(0, b"abcd", b"kept")
        # the empty key
        put(0, b"", b"e0")
        put(2, b"", b"e2")
        # tombstone shadows value; value shadows tombstone
        put(0, b"tomb-over-value", b"v")
        put(2, b"tomb-over-value", b"")
        put(1, b"value-over-tomb", b"")
        put(3, b"value-over-tomb", b"v")
        # only an EARLIER segment repeats it: table 3's stays
        put(0, b"earlier-repeat", b"a")
        put(3, b"earlier-repeat", b"b")
        # single version: a pending compaction output holding it is no shadow
        put(0, b"only-here", b"solo")
        put(1, b"only-there", b"solo")
        self.runs = [build_run([d[k] for k in sorted(d)]) for d in t]
        assert all(len(i) // 16 > 256 for _, i in self.runs)
        self.blooms = [None, _run_bloom(self.runs[1]), None,
                       _run_bloom(self.runs[3])]
        self.writes = ([(k, b"m", 5) for k in tied[::4]]
                       + [(b"ab", b"", 0), (b"", b"em", 0),
                          (b"value-over-tomb", b"", 0), (b"mem-only", b"x", 0)]
                       + [(pool[j], b"pm", 0) for j in range(0, 700, 9)])
        self.mem_run = memtable_model.batch_model.flush_run(self.writes)
        self.keys = sorted({e.key for d, i in self.runs
                            for e in parse_run(d, i)})
        self.filters = _filters(self.keys)
        self.filters["tied"] = dict(start_key=tied[5], end_key=tied[50])
        self.reader = Reader(self.runs, blooms=self.blooms, device=0)
        self.reader.put(self.writes)


@pytest.fixture(scope="module")
def shapes():
    s = _Shapes()
    yield s
    s.reader.close()


# one-candidate windows (a candidate and its shadower never share a window)
# on the small filters only
_SHAPE_CASES = [(n, sh) for n in ("none", "keyrange", "hash", "both", "tied")
                for sh in ("big", "mc7", "mc64", "pe5", "mc300")]
_SHAPE_CASES += [("tied", "mc1"), ("both", "mc1")]


@pytest.mark.parametrize("mem", [False, True], ids=["tables", "memtable"])
@pytest.mark.parametrize("name,shape", _SHAPE_CASES)
def test_newest_only_shapes(shapes, name, shape, mem, variant):
    s = shapes
    shp = {"mc1": (1 << 22, 1 << 15, 1),
           "mc300": (1 << 22, 1 << 15, 300)}.get(shape) or SHAPES[shape]
    kw = s.filters[name]
    segs = sm.segments(s.runs, s.mem_run if mem else None)
    got = _paged(s.reader, kw, shp, memtable=mem, newest_only=True)
    _check(got, segs, kw, True)
    if name == "none":
        es = {(e.key, e.data) for e in parse_run(got[0], got[1])}
        if mem:
            assert (b"ab", b"") in es and (b"", b"em") in es
            assert (b"value-over-tomb", b"") in es
        else:
            assert (b"ab", b"3") in es and (b"", b"e2") in es
            assert (b"value-over-tomb", b"v") in es
        assert (b"tomb-over-value", b"") in es
        assert (b"abc", b"1") in es and (b"abcd", b"kept") in es
        assert (b"earlier-repeat", b"b") in es
        assert (b"earlier-repeat", b"a") not in es
        if shape in ("big", "mc300"):
            # a window of >= 257 candidates crossed a table boundary
            assert max(p["candidates"] for p in got[4]) >= 257


def test_pending_output_does_not_shadow(shapes, variant):
    s = shapes
    rd = Reader(s.runs, blooms=s.blooms, device=0)
    try:
        rd.compact_begin([0, 1], keep_tombstones=True, bloom=True)
        got = _paged(rd, {}, SHAPES["mc64"], newest_only=True)
        _check(got, sm.segments(s.runs), {}, True)
        keys = [e.key for e in parse_run(got[0], got[1])]
        assert keys.count(b"only-here") == 1
        assert keys.count(b"only-there") == 1
        rd.compact_abort()
    finally:
        rd.close()


# ---- 6. cross-check with the read path ----

def test_newest_only_is_what_gets_answer(base, variant):
    rd = base.reader
    got = _paged(rd, {}, SHAPES["mc64"], memtable=True, newest_only=True)
    _check(got, base.segs, {}, True)
    emitted = sm.snapshot_entries(base.segs, newest_only=True)
    keys = [e.key for _, e in emitted]
    assert sorted(keys) == sorted({e.key for d, i in base.segs
                                   for e in parse_run(d, i)})
    hits, voff, values, _ = rd.get_raw(keys)
    blob = values.tobytes()
    for q, (seg, e) in enumerate(emitted):
        assert int(hits["run"][q]) == seg
        assert int(hits["is_tombstone"][q]) == (1 if e.data == b"" else 0)
        assert blob[int(voff[q]):int(voff[q + 1])] == e.data
    assert [e.key for e in parse_run(got[0], got[1])] == keys


# ---- 7. accounting ----

def test_held_bytes_accounting(base):
    rd = base.fresh()
    try:
        tb0 = rd.table_bytes
        res0 = rd.memtable_info["reserved_bytes"]
        singles = []
        for r in (1, 2):
            with Reader([base.runs[r]], device=0) as one:
                singles.append(one.table_bytes)
        a = rd.snapshot_open(memtable=True, max_candidates=64)
        b = rd.snapshot_open(memtable=True, newest_only=True)
        assert rd.held_bytes == 0
        assert rd.table_bytes == tb0
        out = rd.compact([1, 2], 1, keep_tombstones=False)
        # the list let go of two tables; the scans keep them, counted once
        assert rd.held_bytes == sum(singles)
        with Reader([base.runs[0], (out[0], out[1]), base.runs[3]],
                    device=0) as fresh:
            assert rd.table_bytes == fresh.table_bytes
        # a put that displaces the held memtable buffer
        rd.put(memtable_model.gen(21, 20, base.keys[::9]))
        assert rd.held_bytes == sum(singles)  # the held one is the spare now
        rd.put(memtable_model.gen(22, 20, base.keys[::9]))
        assert rd.held_bytes > sum(singles)
        held_mem = rd.held_bytes - sum(singles)
        assert rd.memtable_info["reserved_bytes"] > 0
        # b still yields the snapshot; _paged ends it
        _check(_paged(rd, {}, BIG, opener=lambda: b), base.segs, {}, True)
        assert rd.held_bytes == sum(singles) + held_mem  # a holds them all
        _check(_paged(rd, {}, SHAPES["mc64"], opener=lambda: a), base.segs,
               {}, False)
        assert rd.held_bytes == 0
        assert rd.memtable_info["reserved_bytes"] >= res0
        assert res0 > 0
    finally:
        rd.close()


def test_failed_begin_changes_nothing(base):
    rd = base.reader
    before = (rd.table_bytes, rd.held_bytes, rd.memtable_info)
    from dbeel_amd.engine import ReaderScan

    with pytest.raises(DbeelGpuError) as ei:
        ReaderScan(rd, None, None, None, 0, snapshot_flags=8)
    assert ei.value.code == INVALID_ARG and "flags" in str(ei.value)
    assert (rd.table_bytes, rd.held_bytes, rd.memtable_info) == before


def test_close_with_open_snapshots(base):
    rd = base.fresh()
    a = rd.snapshot_open(memtable=True, newest_only=True, max_candidates=7)
    b = rd.snapshot_open()
    data = np.empty(1 << 16, dtype=np.uint8)
    index = np.empty(16 * 64, dtype=np.uint8)
    a.next(data, index)
    rd.compact([0, 1], 0, keep_tombstones=True)
    rd.put(memtable_model.gen(31, 10, base.keys[::9]))
    rd.put(memtable_model.gen(32, 10, base.keys[::9]))
    assert rd.held_bytes > 0
    rd.close()  # ends both scans, frees what they held
    with pytest.raises(ValueError):
        a.next(data, index)
    b.close()  # a no-op on an ended scan


# ---- 8. seeded fuzz ----

def _fuzz_alphabet():
    ks = [b"", b"a", b"ab", b"abc", b"abcdefgh", b"abcdefgh\0",
          b"abcdefghi", b"abcdefghij"]
    ks += [b"PFXPFXPF" + bytes([65 + j]) * (1 + j % 3) for j in range(20)]
    ks += [b"k%02d" % j for j in range(60 - len(ks))]
    assert len(set(ks)) == 60
    return sorted(ks)


def test_fuzz(variant):
    alpha = _fuzz_alphabet()
    rng = np.random.default_rng(2024 if variant == "narrow" else 2025)

    def rand_run(tag):
        n = int(rng.integers(0, 41))
        ks = sorted({alpha[int(j)] for j in rng.integers(0, 60, n)})
        return build_run([Entry(k, b"" if rng.random() < 0.2
                                else b"%s-%d" % (tag, j), int(j))
                          for j, k in enumerate(ks)])

    def rand_writes(n):
        return [(alpha[int(rng.integers(0, 60))],
                 b"" if rng.random() < 0.2 else b"w%d" % j, j)
                for j in range(n)]

    for trial in range(30):
        n_tables = int(rng.integers(1, 7))
        runs = [rand_run(b"t%d" % r) for r in range(n_tables)]
        blooms = [(_run_bloom(r) if len(r[1]) and rng.random() < 0.3
                   else None) for r in runs]
        writes = rand_writes(int(rng.integers(0, 40)))
        mem = bool(rng.integers(0, 2))
        newest = bool(rng.integers(0, 2))
        kw = {}
        if rng.random() < 0.5:
            a, b = sorted(rng.integers(0, 60, 2).tolist())
            kw.update(start_key=alpha[a], end_key=alpha[b])
        if rng.random() < 0.5:
            kw["hash_ranges"] = PLAIN if rng.random() < 0.7 else WRAPPED
        shape = (1 << 16, int(rng.integers(1, 50)),
                 int(rng.integers(1, 80)))
        mem_run = (memtable_model.batch_model.flush_run(writes)
                   if writes else None)
        segs = sm.segments(runs, mem_run if mem else None)
        edit = int(rng.integers(0, 7))
        with Reader(runs, blooms=blooms, device=0) as rd:
            if writes:
                rd.put(writes)

            def between(page_no):
                if page_no != 1:
                    return
                if edit == 0:
                    rd.insert_run(int(rng.integers(0, rd.n_runs + 1)),
                                  rand_run(b"ins"))
                elif edit == 1:
                    rd.write_batch(rand_writes(10))
                elif edit == 2:
                    rd.put(rand_writes(10))
                    rd.put(rand_writes(10))
                elif edit == 3:
                    rd.memtable_flush()
                    rd.put(rand_writes(5))
                    rd.put(rand_writes(5))
                elif edit == 4:
                    rd.memtable_clear()
                    rd.put(rand_writes(5))
                    rd.put(rand_writes(5))
                elif edit == 5 and rd.n_runs >= 2:
                    rd.compact([0, rd.n_runs - 1], 0,
                               keep_tombstones=bool(rng.integers(0, 2)))
                elif edit == 6 and rd.n_runs >= 1:
                    rd.compact_begin([0], keep_tombstones=True)
                    rd.compact_abort()

            got = _paged(rd, kw, shape, memtable=mem, newest_only=newest,
                         between=between)
            try:
                _check(got, segs, kw, newest)
            except AssertionError:
                print("fuzz trial", trial, "tables", n_tables, "mem", mem,
                      "newest", newest, "kw", kw, "shape", shape, "edit",
                      edit)
                raise
            assert rd.held_bytes == 0
