"""GPU tests of the paged migration scan over the resident tables
(engine.Reader.scan / scan_pages / scan_open, include/dbeel_gpu.h
dbeel_gpu_reader_scan_*).

The host model is pymm3.scan_model — AsyncIter's yield order (runs
ascending, key order within a run), no dedup, no tombstone filter, key range
[start, end) and between_cmp hash ranges. dbeel_gpu_scan (engine.scan) is the
parity yardstick: whatever the page capacities and the candidate window, the
pages concatenated are its bytes.

A note on the wrapped hash range: the reference's between_cmp
(tasks/migration.rs:54-60) is true for EVERY hash when end < start, so a
range set that contains a wrapped range keeps every entry. The cases below
therefore hold one set of plain ranges (which keeps some entries and drops
some — asserted on the CPU) and one set whose SECOND range wraps (keeps
everything; which entries fall to the wrapped range shows in range_ids).
"""
import numpy as np
import pytest

from dbeel_amd.engine import DbeelGpuError, Reader, scan
from dbeel_amd.format import INDEX_DTYPE, Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs
from pymm3 import between_cmp, murmur3_32, scan_model

pytestmark = pytest.mark.gpu

INVALID_ARG, ITEM_TOO_LARGE = 1, 3

PLAIN = [(1 << 28, 1 << 30), (3 << 30, (3 << 30) + (1 << 29))]
WRAPPED = [(1 << 30, 2 << 30), (3 << 30, 1 << 28)]  # second one wraps


class _Shared:
    """test_reader_gpu's input; models computed once, read-only."""

    def __init__(self):
        runs = make_runs(4, 3000, 16, 64, overlap_frac=0.5,
                         tombstone_frac=0.15, seed=55)
        self.runs = [(bytes(d), bytes(i)) for d, i in runs]
        keys = sorted(e.key for d, i in self.runs for e in parse_run(d, i))
        self.total = len(keys)
        krange = dict(start_key=keys[int(0.3 * len(keys))],
                      end_key=keys[int(0.7 * len(keys))])
        self.filters = {
            "none": {},
            "keyrange": krange,
            "hash": dict(hash_ranges=PLAIN),
            "hash_wrapped": dict(hash_ranges=WRAPPED),
            "both": dict(krange, hash_ranges=PLAIN),
            "both_wrapped": dict(krange, hash_ranges=WRAPPED),
        }
        self.model = {k: scan_model(self.runs, **kw)
                      for k, kw in self.filters.items()}
        # entries inside the key range alone: what a scan may examine
        self.in_range = {
            k: scan_model(self.runs, kw.get("start_key"),
                          kw.get("end_key"))[2]
            for k, kw in self.filters.items()}
        self.reader = Reader(self.runs, device=0)


@pytest.fixture(scope="module")
def shared():
    s = _Shared()
    yield s
    s.reader.close()


FILTER_NAMES = ["none", "keyrange", "hash", "hash_wrapped", "both",
                "both_wrapped"]


def _recs(index_bytes):
    return np.frombuffer(index_bytes, dtype=INDEX_DTYPE)


def _paged(rd, kw, page_bytes, page_entries, max_candidates,
           between=None):
    """Drive one scan page by page through caller buffers. Checks every
    page's own shape (offsets from 0, dense); returns the concatenation
    with offsets rebased, the range ids, the summed candidates and the
    page count. between(page_no, rd) runs after each page."""
    data = np.empty(page_bytes, dtype=np.uint8)
    index = np.empty(page_entries * 16, dtype=np.uint8)
    rid = (np.empty(page_entries, dtype=np.uint32)
           if kw.get("hash_ranges") else None)
    datas, recs, rids = [], [], []
    cand = pages = off = 0
    with rd.scan_open(max_candidates=max_candidates, **kw) as sc:
        while True:
            pg = sc.next(data, index, rid)
            pages += 1
            n = pg["n_entries"]
            assert n <= page_entries and pg["data_len"] <= page_bytes
            assert pg["needed"] == 0
            cand += pg["candidates"]
            if n:
                rec = index[:n * 16].view(INDEX_DTYPE).copy()
                sizes = rec["full_size"].astype(np.uint64)
                ends = np.cumsum(sizes)
                assert rec["offset"][0] == 0
                assert np.array_equal(rec["offset"][1:], ends[:-1])
                assert int(ends[-1]) == pg["data_len"]
                rec["offset"] += np.uint64(off)
                off += pg["data_len"]
                recs.append(rec.tobytes())
                datas.append(data[:pg["data_len"]].tobytes())
                if rid is not None:
                    rids.append(rid[:n].copy())
            else:
                assert pg["data_len"] == 0
            if between is not None:
                between(pages, rd)
            if pg["done"]:
                break
        # a finished scan stays finished
        pg = sc.next(data, index, rid)
        assert pg["done"] == 1 and pg["n_entries"] == 0
        assert pg["candidates"] == 0
    ids = np.concatenate(rids) if rids else np.zeros(0, dtype=np.uint32)
    index_bytes = b"".join(recs)
    return (b"".join(datas), index_bytes, len(index_bytes) // 16, ids, cand,
            pages)


def _first_range(key, ranges):
    h = murmur3_32(key, 0)
    return next(j for j, (s, t) in enumerate(ranges) if between_cmp(h, s, t))


def _model_ids(model, ranges):
    d, i, _ = model
    return np.array([_first_range(e.key, ranges) for e in parse_run(d, i)],
                    dtype=np.uint32)


# ---- unpaged parity ----

@pytest.mark.parametrize("name", FILTER_NAMES)
def test_unpaged_parity(shared, name):
    s = shared
    kw = s.filters[name]
    md, mi, mn = s.model[name]
    if name in ("hash", "both", "both_wrapped"):
        assert 0 < mn < s.total  # the filter keeps some and drops some
    if name == "hash_wrapped":
        assert mn == s.total  # between_cmp's wrapped case matches all
    if name == "keyrange":
        assert 0 < mn < s.total and mn == s.in_range[name]
    gd, gi, gn = scan(s.runs, device=0, **kw)
    assert (gn, gi, gd) == (mn, mi, md)
    rd_, ri, rn = s.reader.scan(**kw)
    assert (rn, ri, rd_) == (mn, mi, md)
    # one page holds everything: the unpaged call is a single page
    pages = list(s.reader.scan_pages(**kw))
    assert len(pages) == 1 and pages[0][2] == mn
    assert (pages[0][3] is None) == ("hash_ranges" not in kw)


# ---- paging invariance ----

# (page_bytes, page_entries, max_candidates); None = roomy. Entries here are
# 112 B (value) or 48 B (tombstone).
def _configs():
    cfg = [("mc%d" % mc, None, None, mc)
           for mc in (1, 7, 255, 256, 257, 4096)]
    cfg += [("pe%d" % pe, None, pe, 0) for pe in (1, 3, 1000)]
    cfg += [("exact5", "exact", None, 0), ("exact5-1", "exact-1", None, 0)]
    return cfg


# the four filters of the unpaged test, and the wrapped set on the key range
PAGING_FILTERS = ["none", "keyrange", "hash", "both", "both_wrapped"]


@pytest.mark.parametrize("cfg", _configs(), ids=lambda c: c[0])
@pytest.mark.parametrize("name", PAGING_FILTERS)
def test_paging_invariance(shared, name, cfg):
    s = shared
    kw = s.filters[name]
    md, mi, mn = s.model[name]
    _, pb, pe, mc = cfg
    sizes = _recs(mi)["full_size"]
    if pb in ("exact", "exact-1"):
        # room for exactly the first 5 survivors / one byte short of it
        pb = int(sizes[:5].sum()) - (pb == "exact-1")
    pb = pb or 1 << 22
    pe = pe or 1 << 15
    d, i, n, ids, cand, pages = _paged(s.reader, kw, pb, pe, mc)
    assert (n, i, d) == (mn, mi, md)
    # every in-range entry is examined exactly once, nothing else ever is
    assert cand == s.in_range[name]
    if "hash_ranges" in kw:
        assert np.array_equal(ids, _model_ids(s.model[name],
                                              kw["hash_ranges"]))
    if mc:
        assert pages >= -(-s.in_range[name] // mc)
    if cfg[0] == "exact5" and mn >= 5:
        # the first page took exactly the five that fit
        first = next(iter(s.reader.scan_pages(page_bytes=pb, **kw)))
        assert first[2] == 5 and len(first[0]) == pb
    if cfg[0] == "exact5-1" and mn >= 5:
        first = next(iter(s.reader.scan_pages(page_bytes=pb, **kw)))
        assert first[2] == 4


# ---- bounds ----

def _neighbours(k):
    out = {k, k + b"\0", k + b"\xff"}
    if k:
        out.add(k[:-1])
        if k[-1]:
            out.add(k[:-1] + bytes([k[-1] - 1]) + b"\xff\xff")
        if k[-1] != 0xFF:
            out.add(k[:-1] + bytes([k[-1] + 1]))
    return out


def test_bounds_equal_prefix_and_padding():
    rng = np.random.default_rng(7)
    pre = b"SAMEPFX8"
    tails = {b"", b"\0", b"\0\0", b"\0\x01", b"\x01", b"\xff" * 41}
    while len(tails) < 40:
        ln = int(rng.integers(1, 42))
        tails.add(bytes(rng.integers(0, 256, ln, dtype=np.uint8))
                  if rng.integers(0, 2) else bytes(ln))
    same = sorted(pre + t for t in tails)
    assert len(same) == 40 and max(map(len, same)) == 49
    special = [b"", b"ab", b"ab\0", b"ab\0\0"]
    keys = sorted(special + same)

    def run(ks, ts):
        return build_run([Entry(k, b"" if j % 5 == 0 else b"v" * (j % 9 + 1),
                                ts + j) for j, k in enumerate(sorted(ks))])

    runs = [run(keys, 100), run(keys[::2], 200), (b"", b""),
            run(keys[1::3], 300), run(special, 400)]
    probes = set()
    for k in keys:
        probes |= _neighbours(k)
    probes |= {b"a", b"ac", b"SAMEPFX", b"SAMEPFX9", b"\xff" * 60}
    probes = sorted(probes)
    cases = [dict(start_key=p) for p in probes]
    cases += [dict(end_key=p) for p in probes]
    cases += [dict(start_key=p, end_key=p) for p in probes[::7]]  # empty
    pick = rng.integers(0, len(probes), (120, 2))
    cases += [dict(start_key=probes[a], end_key=probes[b])
              for a, b in pick]  # start < end and start > end alike
    cases += [dict(end_key=b""), dict(start_key=b"", end_key=b""),
              dict(start_key=b""), dict(start_key=b"ab", end_key=b"ab\0"),
              dict(start_key=b"ab\0\0", end_key=b"ab")]
    with Reader(runs, device=0) as rd:
        for c, kw in enumerate(cases):
            exp = scan_model(runs, **kw)
            got = rd.scan(**kw)
            assert got == exp, kw
            if c % 5 == 0 or len(kw) == 2 and c % 2:
                # and through a window that splits every table
                got = rd.scan(max_candidates=3, page_entries=2, **kw)
                assert got == exp, kw
    assert scan_model(runs, end_key=b"")[2] == 0
    assert scan_model(runs, start_key=b"ab", end_key=b"ab\0")[2] == 2
    assert scan_model(runs, start_key=pre, end_key=pre + b"\0")[2] > 0


# ---- range ids ----

def test_range_ids_first_match(shared):
    s = shared
    ranges = [(0, 3 << 30), (1 << 30, 2 << 30), (2 << 30, 2**32 - 1),
              (5, 0)]  # overlapping; the last one wraps (matches all)
    model = scan_model(s.runs, hash_ranges=ranges)
    exp = _model_ids(model, ranges)
    assert set(exp.tolist()) == {0, 2, 3} or set(exp.tolist()) == {0, 2}
    assert 1 not in exp  # shadowed by range 0: "first" matters
    d, i, n, ids = s.reader.scan(hash_ranges=ranges, return_range_ids=True)
    assert (d, i, n) == model
    assert np.array_equal(ids, exp)
    d, i, n, ids = s.reader.scan(hash_ranges=ranges, page_entries=1000,
                                 max_candidates=1500, return_range_ids=True)
    assert (d, i, n) == model
    assert np.array_equal(ids, exp)
    # order of the ranges decides the id, not the match set
    rev = ranges[::-1]
    d, i, n, ids = s.reader.scan(hash_ranges=rev, return_range_ids=True)
    assert (d, i, n) == model
    assert np.array_equal(ids, _model_ids(model, rev))
    assert set(ids.tolist()) == {0}


# ---- too-large item ----

@pytest.mark.parametrize("name", ["none", "hash"])
def test_item_too_large_then_continue(shared, name):
    s = shared
    kw = s.filters[name]
    md, mi, mn = s.model[name]
    first = int(_recs(mi)["full_size"][0])
    small = np.empty(first - 1, dtype=np.uint8)
    index = np.empty(16 * 4096, dtype=np.uint8)
    rid = (np.empty(4096, dtype=np.uint32) if "hash_ranges" in kw else None)
    big = np.empty(1 << 22, dtype=np.uint8)
    with s.reader.scan_open(**kw) as sc:
        for _ in range(2):  # the cursor does not move: same answer twice
            with pytest.raises(DbeelGpuError) as ei:
                sc.next(small, index, rid)
            assert ei.value.code == ITEM_TOO_LARGE
            assert ei.value.page["needed"] == first
            assert ei.value.page["n_entries"] == 0
            assert ei.value.page["data_len"] == 0
            assert ei.value.page["done"] == 0
        datas, recs, off, cand = [], [], 0, 0
        while True:
            pg = sc.next(big, index, rid)
            n = pg["n_entries"]
            rec = index[:n * 16].view(INDEX_DTYPE).copy()
            rec["offset"] += np.uint64(off)
            off += pg["data_len"]
            recs.append(rec.tobytes())
            datas.append(big[:pg["data_len"]].tobytes())
            cand += pg["candidates"]
            if pg["done"]:
                break
    assert (b"".join(datas), b"".join(recs)) == (md, mi)
    assert cand == s.in_range[name]


def test_argument_validation(shared):
    s = shared
    data = np.empty(4096, dtype=np.uint8)
    index = np.empty(64, dtype=np.uint8)
    with s.reader.scan_open() as sc:
        for d, x in ((data[:0], index), (data, index[:15])):
            with pytest.raises(DbeelGpuError) as ei:
                sc.next(d, x)
            assert ei.value.code == INVALID_ARG
        # refused calls left the scan where it was
        pg = sc.next(data, index)
        assert pg["n_entries"] > 0


# ---- liveness ----

def _new_reader(s):
    return Reader(s.runs, device=0)


def test_compact_begin_does_not_disturb_a_scan(shared):
    s = shared
    md, mi, mn = s.model["hash"]

    def between(page_no, rd):
        if page_no == 2:
            rd.compact_begin([0, 1], True, fetch=False)
        if page_no == 4:
            rd.compact_abort()

    with _new_reader(s) as rd:
        d, i, n, ids, cand, pages = _paged(
            rd, s.filters["hash"], 1 << 22, 700, 0, between=between)
        assert pages > 4
        assert (n, i, d) == (mn, mi, md)
        # a compaction left pending is invisible as well
        rd.compact_begin([1, 2], False, fetch=False)
        assert rd.scan(**s.filters["hash"]) == (md, mi, mn)


def _assert_stale(sc, data, index):
    with pytest.raises(DbeelGpuError) as ei:
        sc.next(data, index)
    assert ei.value.code == INVALID_ARG
    assert "stale" in str(ei.value)


def test_commit_and_insert_make_scans_stale(shared):
    s = shared
    data = np.empty(1 << 22, dtype=np.uint8)
    index = np.empty(16 * 500, dtype=np.uint8)
    extra = build_run([Entry(b"", b"", 9), Entry(b"zz-flushed", b"new", 10)])
    with _new_reader(s) as rd:
        sc = rd.scan_open()
        other = rd.scan_open(start_key=b"\x80")
        assert sc.next(data, index)["n_entries"] == 500
        cd, ci, _, _ = rd.compact_begin([0, 1], True)
        assert sc.next(data, index)["n_entries"] == 500  # still good
        rd.compact_commit(0)
        _assert_stale(sc, data, index)
        _assert_stale(sc, data, index)
        _assert_stale(other, data, index)
        sc.close()
        other.close()
        now = [(cd, ci), s.runs[2], s.runs[3]]
        assert rd.scan() == scan_model(now)
        kw = s.filters["both"]
        assert rd.scan(page_entries=333, **kw) == scan_model(now, **kw)

        sc = rd.scan_open(**kw)
        assert sc.next(data, index)["n_entries"] > 0
        rd.insert_run(1, extra)
        _assert_stale(sc, data, index)
        sc.close()
        now.insert(1, extra)
        assert rd.scan() == scan_model(now)
        assert rd.scan(max_candidates=1000, **kw) == scan_model(now, **kw)


def test_close_reader_with_scan_open(shared):
    s = shared
    data = np.empty(1 << 16, dtype=np.uint8)
    index = np.empty(16 * 10, dtype=np.uint8)
    rd = _new_reader(s)
    sc = rd.scan_open()
    abandoned = rd.scan_open(hash_ranges=PLAIN)
    assert sc.next(data, index)["n_entries"] == 10
    gen = rd.scan_pages(page_entries=10)
    assert next(gen)[2] == 10  # a generator parked mid-scan
    rd.close()
    with pytest.raises(ValueError):
        sc.next(data, index)
    sc.close()
    abandoned.close()
    gen.close()
    # the library is fine afterwards
    assert s.reader.scan(**s.filters["both"]) == s.model["both"]


# ---- pinned pages ----

def test_pinned_pages(shared):
    s = shared
    for name in ("none", "both"):
        kw = s.filters[name]
        assert s.reader.scan(pinned=True, **kw) == s.model[name]
        got = s.reader.scan(pinned=True, page_bytes=100_000,
                            page_entries=777, **kw)
        assert got == s.model[name]


# ---- entry sizes (k_copy's geometry variants) ----

def test_large_values():
    runs = make_runs(2, 300, 16, 4096, overlap_frac=0.3, tombstone_frac=0.1,
                     seed=77)
    runs = [(bytes(d), bytes(i)) for d, i in runs]
    kw = dict(hash_ranges=[(0, 3 << 30)])
    with Reader(runs, device=0) as rd:
        for k in ({}, kw):
            exp = scan_model(runs, **k)
            assert 0 < exp[2]
            assert rd.scan(**k) == exp
            assert rd.scan(page_bytes=100_000, **k) == exp
            assert rd.scan(page_bytes=4144, **k) == exp  # one value a page


def test_minimal_entries():
    # 32-byte entries: empty key, empty value — one per run (keys are unique
    # inside a run), plus a run that mixes one in
    e32 = [build_run([Entry(b"", b"", t)]) for t in (1, 2, 3, 4, 5)]
    mixed = build_run([Entry(b"", b"", 6), Entry(b"k", b"v", 7)])
    runs = e32[:3] + [mixed] + e32[3:]
    exp = scan_model(runs)
    assert exp[2] == 7 and len(exp[0]) == 6 * 32 + 34
    with Reader(runs, device=0) as rd:
        assert rd.scan() == exp
        for pb in (32, 33, 64, 95, 96):
            if pb >= 34:
                assert rd.scan(page_bytes=pb) == exp
            else:
                # the 34-byte entry cannot fit a 32-byte page
                with pytest.raises(DbeelGpuError) as ei:
                    rd.scan(page_bytes=pb)
                assert ei.value.code == ITEM_TOO_LARGE
                assert ei.value.page["needed"] == 34
        assert rd.scan(end_key=b"k") == scan_model(runs, end_key=b"k")
        assert rd.scan(start_key=b"\0") == scan_model(runs, start_key=b"\0")
        only = rd.scan(hash_ranges=[(0, 1)])
        assert only == scan_model(runs, hash_ranges=[(0, 1)])
