"""GPU tests of dbeel_gpu_reader_get_entries (engine.Reader.get_entries /
get_entries_raw) and dbeel_gpu_reader_compact_fetch
(Reader.compact_fetch_into), include/dbeel_gpu.h.

The host model is get_entries_model: the reference's get_entry read path
(memtable first, then the HIGHEST run index, whatever the timestamps) with the
record of a found key — a tombstone included — being the stored
`data_len | data | timestamp`. Every call below goes through _call, which
hands the engine buffers with guard elements behind hits, record_offsets and
records and checks that nothing past the result was written.
"""
import ctypes

import numpy as np
import pytest

import batch_model
import get_entries_model as gem
import memtable_model
import oracle
from conftest import load_golden
from dbeel_amd.engine import (HIT_DTYPE, DbeelGpuError, GetBuffers, GetPage,
                              GetStats, Job, LookupHit, Reader, _key_blob,
                              pin_host, unpin_host)
from dbeel_amd.format import Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs

pytestmark = pytest.mark.gpu

INVALID_ARG, ITEM_TOO_LARGE = 1, 3
HIT_FIELDS = ("run", "is_tombstone", "value_offset", "value_len")
COUNTERS = ("bloom_probes", "bloom_skips", "searches", "hits", "tombstones")
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
GUARD = 0xA5
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)


def _call(rd, keys, cap=None, pinned=False):
    """One get_entries call into guarded buffers. cap None = a first call
    with cap 0 learns records_total (a hit at query 0 then answers
    ITEM_TOO_LARGE with the offsets complete), then the call proper.
    -> (rc, hits, offsets, delivered bytes, page dict, stats dict)."""
    n = len(keys)
    ka, koff = _key_blob(keys)
    if cap is None:
        h0 = np.zeros(n, dtype=HIT_DTYPE)
        o0 = np.zeros(n + 1, dtype=np.uint64)
        rc, pg, _ = rd._get_entries_into(ka, koff, h0, o0, None, 0)
        assert rc in (0, ITEM_TOO_LARGE)
        cap = int(pg.records_total)
    hits = np.frombuffer(bytes([GUARD]) * ((n + 2) * HIT_DTYPE.itemsize),
                         dtype=HIT_DTYPE).copy()
    roff = np.full(n + 1 + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rec = np.full(cap + 64, GUARD, dtype=np.uint8)
    if pinned:
        pin_host(rec)
    try:
        rc, page, st = rd._get_entries_into(ka, koff, hits, roff, rec, cap)
    finally:
        if pinned:
            unpin_host(rec)
    page, st = page.as_dict(), st.as_dict()
    assert np.all(hits[n:].view(np.uint8) == GUARD), "hits guard"
    assert np.all(roff[n + 1:] == 0xA5A5A5A5A5A5A5A5), "offsets guard"
    rl = page["records_len"]
    assert rl <= cap
    assert np.all(rec[rl:] == GUARD), "bytes at or past records_len"
    return rc, hits[:n].copy(), roff[:n + 1].copy(), rec[:rl].tobytes(), \
        page, st


def _check(rd, model, keys, cap=None, pinned=False):
    """The call's whole answer against the model's for the same cap."""
    ehits, eoff, erec, erc, epage = model.expect(keys, cap)
    rc, hits, roff, rec, page, st = _call(rd, keys, cap, pinned)
    assert rc == erc
    assert page == epage
    eh = gem.hits_array(ehits, HIT_DTYPE)
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], eh[f]), f
    assert roff.tolist() == eoff
    assert rec == erec[:epage["records_len"]]
    return rc, hits, roff, rec, page, st


def _assert_raw_equal(got, exp):
    for f in HIT_FIELDS:
        assert np.array_equal(got[0][f], exp[0][f]), f
    assert np.array_equal(got[1], exp[1])
    assert got[2].tobytes() == exp[2].tobytes()


def _run_bloom(run):
    with Job([run], device=0) as job:
        job.run(True)
        return job.bloom()


def _absent(n, seed=99, klen=16):
    rng = np.random.default_rng(seed)
    return [b"\xfe" + bytes(rng.integers(0, 256, klen - 1, dtype=np.uint8))
            for _ in range(n)]


class _Parity:
    """test_reader_gpu's inputs, built once and read-only."""

    def __init__(self):
        runs = make_runs(4, 3000, 16, 64, overlap_frac=0.5,
                         tombstone_frac=0.15, seed=55)
        self.runs = [(bytes(d), bytes(i)) for d, i in runs]
        self.model = gem.Model(self.runs)
        rng = np.random.default_rng(3)
        present = sorted(self.model.where)
        self.present = [present[int(rng.integers(0, len(present)))]
                        for _ in range(500)]
        self.absent = [bytes(rng.integers(0, 256, 16, dtype=np.uint8))
                       for _ in range(100)]
        assert not any(k in self.model.where for k in self.absent)
        self.queries = self.present + self.absent
        self.tomb = [k for k in present if not self.model.where[k][2].data]
        self.live = [k for k in present if self.model.where[k][2].data]
        assert self.tomb and self.live


@pytest.fixture(scope="module")
def parity():
    return _Parity()


# ---- 1. parity ----

@pytest.mark.parametrize("filters", [False, True], ids=["plain", "filters"])
def test_parity(parity, filters):
    p = parity
    blooms = [_run_bloom(r) for r in p.runs] if filters else None
    with Reader(p.runs, blooms=blooms, device=0) as rd:
        before = rd.get_raw(p.queries)
        rc, hits, roff, rec, page, st = _check(rd, p.model, p.queries)
        after = rd.get_raw(p.queries)  # the scratch is shared
        assert rd.get_entries(p.queries) == p.model.entries(p.queries)
        assert rd.get_entries(p.queries, page_bytes=100) == \
            p.model.entries(p.queries)
        # the public raw call, its own buffer
        h2, o2, view, pg2, _ = rd.get_entries_raw(p.queries)
        assert np.array_equal(h2, hits) and np.array_equal(o2, roff)
        assert view.tobytes() == rec and pg2 == page
    assert rc == 0 and page["n_done"] == len(p.queries)
    _assert_raw_equal(after, before)
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], before[0][f]), f
    for c in COUNTERS:
        assert st[c] == before[3][c] == after[3][c], c
    assert (st["bloom_probes"] > 0) == filters
    n_tomb = int(hits["is_tombstone"].sum())
    assert n_tomb and st["tombstones"] == n_tomb
    assert page["records_total"] == \
        int(before[1][-1]) + 24 * int((hits["run"] >= 0).sum())


# ---- 2. read-path order and timestamps ----

def test_read_path_order_and_timestamps():
    old = build_run([Entry(b"deleted", b"still-here", I128_MAX),
                     Entry(b"only-old", b"o", I128_MIN),
                     Entry(b"same-key", b"old-value", 1000)])
    new = build_run([Entry(b"deleted", b"", -1),
                     Entry(b"same-key", b"new-value", 10),  # OLDER timestamp
                     Entry(b"zero", b"z", 0),
                     Entry(b"zmax", b"", I128_MAX),
                     Entry(b"zmin", b"m", I128_MIN)])
    keys = [b"same-key", b"deleted", b"only-old", b"nowhere", b"zero",
            b"zmax", b"zmin"]
    model = gem.Model([old, new])
    with Reader([old, new], device=0) as rd:
        rc, hits, roff, rec, page, _ = _check(rd, model, keys)
        got = rd.get_entries(keys)
    assert got == [(b"new-value", 10), (b"", -1), (b"o", I128_MIN), None,
                   (b"z", 0), (b"", I128_MAX), (b"m", I128_MIN)]
    assert hits["run"].tolist() == [1, 1, 0, -1, 1, 1, 1]
    assert hits["is_tombstone"].tolist() == [0, 1, 0, 0, 0, 1, 0]
    # a found tombstone: 24 bytes, data_len 0 and its own timestamp
    t = rec[int(roff[1]):int(roff[2])]
    assert t == bytes(8) + (-1).to_bytes(16, "little", signed=True)
    assert roff[3] == roff[4]  # absent: an empty range


# ---- 3. copy edges ----

VLENS = (list(range(18)) + [39, 40, 41, 487, 488, 489, 511, 512, 513, 1000,
                            4097, 200_000])


def _value(rng, n):
    return bytes(rng.integers(1, 256, n, dtype=np.uint8))


class _Edges:
    """Every value length under every key length 1..9, spread over three
    runs; `flip` decides which end of the length list sorts first, so that
    the first entry of a run, the last entry of a run and the last entry of
    the last run (its record ends where the slab's data ends) are short ones
    in one arrangement and the longest in the other."""

    def __init__(self, flip):
        rng = np.random.default_rng(17 + flip)
        per_run = [[], [], []]
        for j, v in enumerate(VLENS):
            lead = len(VLENS) - j if flip else j + 1
            for klen in range(1, 10):
                key = bytes([lead] + [klen] * (klen - 1))
                per_run[j % 3].append(
                    Entry(key, _value(rng, v), int(rng.integers(-2**62, 2**62))))
        self.runs = [build_run(sorted(es, key=lambda e: e.key))
                     for es in per_run]
        self.model = gem.Model(self.runs)
        self.keys = sorted(self.model.where)
        assert len(self.keys) == 9 * len(VLENS)
        # the placements named above hold
        ends = [[len(parse_run(d, i)[at].data) for d, i in self.runs]
                for at in (0, -1)]
        assert ends == ([[1000, 4097, 200_000], [0, 1, 2]] if flip
                        else [[0, 1, 2], [1000, 4097, 200_000]])


@pytest.mark.parametrize("flip", [0, 1], ids=["short-first", "long-first"])
def test_copy_edges(flip):
    e = _Edges(flip)
    rng = np.random.default_rng(5)
    repeats = [k for k in e.keys[::7] for _ in range(2)] + \
        [e.keys[int(j)] for j in rng.integers(0, len(e.keys), 40)]
    aligned = set()
    with Reader(e.runs, device=0) as rd:
        for keys in (e.keys, e.keys[::-1], repeats):
            keys = keys[:40] + [b"\xff-absent"] + keys[40:]
            rc, hits, roff, rec, page, _ = _check(rd, e.model, keys)
            assert rc == 0 and page["n_done"] == len(keys)
            aligned |= {(int(o) % 8, int(v) % 8) for o, v in
                        zip(roff[:-1], hits["value_offset"])}
    # every destination alignment against every source alignment
    assert len(aligned) == 64


def test_copy_edges_empty_key():
    """Key length 0: the entry is the first and the last of its run and of
    the slab. One tiny reader per value length; the repeat gives the second
    copy a destination of every alignment."""
    rng = np.random.default_rng(23)
    for v in VLENS:
        run = build_run([Entry(b"", _value(rng, v), -v - 1)])
        model = gem.Model([run])
        with Reader([run], device=0) as rd:
            _check(rd, model, [b"", b"", b"x", b""])
            assert rd.get_entries([b""])[0][1] == -v - 1


# ---- 4. caps ----

class _Caps:
    def __init__(self, p):
        rng = np.random.default_rng(8)
        pick = lambda pool, n: [pool[int(j)]
                                for j in rng.integers(0, len(pool), n)]
        self.keys = ([p.tomb[0]] + pick(p.live, 60) + p.absent[:5]
                     + pick(p.tomb, 10) + pick(p.live, 60) + p.absent[5:9])
        _, self.off, self.rec, _, _ = p.model.expect(self.keys)
        self.total = self.off[-1]
        self.mid = self.off[70]  # a record boundary in the middle
        assert self.off[1] == 24 and 24 < self.mid < self.total
        assert self.off[70] > self.off[69]


@pytest.fixture(scope="module")
def caps(parity):
    return _Caps(parity)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_caps(parity, caps, pinned):
    p, c = parity, caps
    n = len(c.keys)
    with Reader(p.runs, device=0) as rd:
        rc, _, _, _, page, _ = _check(rd, p.model, c.keys, c.total, pinned)
        assert rc == 0 and page["n_done"] == n and page["needed"] == 0
        # one byte short: the last RECORD is out, and the absents behind it
        rc, _, _, _, page, _ = _check(rd, p.model, c.keys, c.total - 1, pinned)
        assert rc == 0 and page["n_done"] == n - 5
        rc, _, _, _, page, _ = _check(rd, p.model, c.keys, c.mid, pinned)
        assert rc == 0 and page["records_len"] == c.mid
        assert page["n_done"] >= 70
        rc, _, _, _, page, _ = _check(rd, p.model, c.keys, c.mid - 1, pinned)
        assert rc == 0 and page["n_done"] == 69
        assert page["needed"] == c.off[70] - c.off[69]
        # query 0 is a tombstone: 24 bytes hold exactly it
        rc, hits, _, rec, page, _ = _check(rd, p.model, c.keys, 24, pinned)
        assert rc == 0 and page["n_done"] == 1 and len(rec) == 24
        assert hits["is_tombstone"][0] == 1
        rc, _, _, _, page, _ = _check(rd, p.model, c.keys, 23, pinned)
        assert rc == ITEM_TOO_LARGE and page["needed"] == 24
        # cap 0: only absent keys are all done ...
        rc, hits, roff, rec, page, _ = _check(rd, p.model, p.absent, 0, pinned)
        assert rc == 0 and page["n_done"] == len(p.absent) and rec == b""
        # ... a present query 0 is too large, hits and offsets complete
        rc, hits, roff, rec, page, _ = _check(rd, p.model, c.keys[1:], 0,
                                              pinned)
        assert rc == ITEM_TOO_LARGE
        assert page["n_done"] == 0 and page["records_len"] == 0
        assert page["needed"] == c.off[2] - c.off[1] > 24
        assert page["records_total"] == c.total - 24
        assert int(roff[-1]) == c.total - 24 and hits["run"][0] >= 0
        # the Python wrapper carries the same on its exception
        with pytest.raises(DbeelGpuError) as ei:
            rd.get_entries_raw(c.keys[1:], records_cap=0)
        assert ei.value.code == ITEM_TOO_LARGE
        assert ei.value.page["needed"] == page["needed"]
        assert np.array_equal(ei.value.record_offsets, roff)


@pytest.mark.parametrize("cap", [24, 1 << 10, 64 << 10])
def test_call_again_loop_reassembles_the_one_shot_bytes(parity, caps, cap):
    p, c = parity, caps
    with Reader(p.runs, device=0) as rd:
        rec = np.full(cap + 64, GUARD, dtype=np.uint8)
        pin_host(rec)
        try:
            done, parts, calls = 0, [], 0
            while done < len(c.keys):
                try:
                    hits, roff, view, page, _ = rd.get_entries_raw(
                        c.keys[done:], records=rec, records_cap=cap)
                except DbeelGpuError as e:
                    # only a record over the cap may stop the loop
                    assert e.code == ITEM_TOO_LARGE and cap == 24
                    assert e.page["needed"] > cap
                    big = np.empty(e.page["needed"], dtype=np.uint8)
                    hits, roff, view, page, _ = rd.get_entries_raw(
                        c.keys[done:done + 1], records=big)
                    assert page["n_done"] == 1
                assert page["n_done"] > 0
                assert roff.tolist() == \
                    [o - c.off[done] for o in c.off[done:done + len(roff)]]
                parts.append(view.tobytes())
                done += page["n_done"]
                calls += 1
            assert np.all(rec[cap:] == GUARD)
        finally:
            unpin_host(rec)
    assert b"".join(parts) == c.rec
    assert calls > 1 or cap >= c.total
    if cap == 24:
        with Reader(p.runs, device=0) as rd:
            assert rd.get_entries(c.keys, page_bytes=24) == \
                p.model.entries(c.keys)


# ---- 5. memtable ----

POOL = memtable_model.key_pool(41, 300)


def batch_model_run(seed):
    """~120 entries drawn from the whole pool: runs overlap each other."""
    return batch_model.flush_run(memtable_model.gen(seed, 150, POOL))


def _mem_base():
    return [batch_model_run(s) for s in (1, 2)]


def test_memtable_hits_then_flush_is_byte_identical():
    tables = _mem_base()
    mt = memtable_model.Memtable()
    keys = POOL[::2] + _absent(20) + POOL[1::5]
    with Reader(tables, device=0) as rd:
        for seed in (7, 8):
            w = memtable_model.gen(seed, 120, POOL[::4])
            rd.put(w)
            mt.put(w)
        # an earlier arrival with the larger timestamp loses
        w = [(b"arrival", b"first", 9000), (b"arrival", b"second", -9000),
             (b"gone", b"", I128_MIN)]
        rd.put(w)
        mt.put(w)
        keys = keys + [b"arrival", b"gone"]
        model = gem.Model(tables, mt)
        before_raw = rd.get_raw(keys)
        rc, hits, roff, rec, page, st = _check(rd, model, keys)
        assert rc == 0
        assert (hits["run"] == 2).sum() >= mt.entries // 3
        assert hits["run"][-2:].tolist() == [2, 2]
        assert rd.get_entries([b"arrival", b"gone"]) == [
            (b"second", -9000), (b"", I128_MIN)]
        for c in COUNTERS:
            assert st[c] == before_raw[3][c], c
        rd.memtable_flush(fetch=False)
        assert rd.n_runs == 3 and rd.memtable_info["entries"] == 0
        rc2, hits2, roff2, rec2, page2, _ = _check(
            rd, gem.Model(tables + [mt.run()]), keys)
        assert hits2.tobytes() == hits.tobytes()
        assert roff2.tobytes() == roff.tobytes() and rec2 == rec
        assert page2 == page


def test_memtable_over_64_tables():
    """run == 64 lies past the descriptor's arrays: the memtable's data
    pointer is chosen before they are indexed."""
    tiny = [build_run([Entry(b"k%02d" % r, b"v" * (r % 19), r - 30)])
            for r in range(64)]
    mt = memtable_model.Memtable()
    w = [(b"k07", b"", 1), (b"new", b"value", I128_MAX),
         (b"k63", b"over", -3), (b"new", b"value-2", 0)]
    keys = [b"k%02d" % r for r in range(64)] + [b"new", b"none", b"k63"]
    with Reader(tiny, device=0) as rd:
        rd.put(w)
        mt.put(w)
        rc, hits, _, _, _, _ = _check(rd, gem.Model(tiny, mt), keys)
        assert hits["run"][[7, 63, 64, 65, 66]].tolist() == [64, 64, 64, -1, 64]
        got = rd.get_entries(keys)
        assert got[7] == (b"", 1) and got[64] == (b"value-2", 0)
        assert got[63] == (b"over", -3) and got[5] == (b"v" * 5, -25)
        _check(rd, gem.Model(tiny, mt), keys, cap=100)


# ---- 6. after edits ----

def _same_as_fresh(live, runs, keys):
    assert live.n_runs == len(runs)
    got = _check(live, gem.Model(runs), keys)
    with Reader(runs, device=0) as fresh:
        exp = _call(fresh, keys)
    assert got[0] == exp[0] == 0
    assert got[1].tobytes() == exp[1].tobytes()
    assert got[2].tobytes() == exp[2].tobytes()
    assert got[3] == exp[3] and got[4] == exp[4]


def test_after_insert_compact_and_write_batch():
    runs = [batch_model_run(s) for s in (1, 2, 3)]
    extra = batch_model.flush_run(memtable_model.gen(9, 100, POOL[::2]))
    keys = POOL + _absent(30)
    with Reader(runs, device=0) as rd:
        rd.insert_run(1, extra)
        runs.insert(1, extra)
        _same_as_fresh(rd, runs, keys)
        for keep in (True, False):
            rd.compact([0, 2], 1, keep, fetch=False)
            od, oi, _ = oracle.compact([runs[0], runs[2]], keep)
            runs = [r for p, r in enumerate(runs) if p not in (0, 2)]
            runs.insert(1, (od, oi))
            _same_as_fresh(rd, runs, keys)
        w = memtable_model.gen(12, 90, POOL[::3])
        rd.write_batch(w, fetch=False)
        runs.append(batch_model.flush_run(w))
        _same_as_fresh(rd, runs, keys)


# ---- 7. refusals on a live reader ----

def test_refusals_in_header_order(parity):
    p = parity
    keys = p.queries[:50]
    ka, koff = _key_blob(keys)
    n = len(keys)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    roff = np.zeros(n + 1, dtype=np.uint64)
    rec = np.zeros(1 << 16, dtype=np.uint8)
    desc = koff.copy()
    desc[3] = desc[2] - 1
    kp, op, dp = (ka.ctypes.data_as(U8P), koff.ctypes.data_as(U64P),
                  desc.ctypes.data_as(U64P))
    hp = hits.ctypes.data_as(ctypes.POINTER(LookupHit))
    rp, cp = roff.ctypes.data_as(U64P), rec.ctypes.data_as(U8P)
    with Reader(p.runs, device=0) as rd:
        lib, h = rd._lib, rd._h
        before = _call(rd, keys)
        tb = rd.table_bytes

        def refused(word, k, o, nk, buf, page=True):
            pg = GetPage()
            pg.needed = 5
            st = GetStats()
            rc = lib.dbeel_gpu_reader_get_entries(
                h, k, o, nk, None if buf is None else ctypes.byref(buf),
                ctypes.byref(pg) if page else None, ctypes.byref(st))
            assert rc == INVALID_ARG
            assert word in lib.dbeel_gpu_last_error(), \
                lib.dbeel_gpu_last_error()
            assert pg.needed == (0 if page else 5)  # a given page is zeroed

        good =GetBuffers(hp, rp, cp, rec.size)
        no_hits = GetBuffers(None, rp, None, 8)
        no_roff = GetBuffers(hp, None, None, 8)
        no_rec = GetBuffers(hp, rp, None, 8)
        # 1. NULL buf or page, whatever else is wrong
        refused(b"buf or page", None, dp, 1 << 32, None)
        refused(b"buf or page", None, dp, 1 << 32, no_hits, page=False)
        # 2. NULL keys / key_offsets / hits / record_offsets, ahead of 3-5
        refused(b"hits or", None, dp, 1 << 32, no_rec)
        refused(b"hits or", kp, None, 1 << 32, no_rec)
        refused(b"hits or", kp, dp, 1 << 32, no_hits)
        refused(b"hits or", kp, dp, 1 << 32, no_roff)
        # 3. NULL records with a cap, ahead of 4-5
        refused(b"null records", kp, dp, 1 << 32, no_rec)
        # 4. 2^32 keys, ahead of the offsets being read
        refused(b"2^32", kp, dp, 1 << 32, good)
        # 5. a descending offset
        refused(b"not ascending at 2", kp, dp, n, good)
        assert not hits.view(np.uint8).any() and not roff.any()
        assert not rec.any()

        # legal edge inputs: no keys at all, with and without the arrays
        pg = GetPage()
        pg.needed = 5
        roff[0] = 77
        assert lib.dbeel_gpu_reader_get_entries(
            h, None, None, 0, ctypes.byref(good), ctypes.byref(pg), None) == 0
        assert roff[0] == 0 and pg.as_dict() == {
            "n_done": 0, "records_len": 0, "records_total": 0, "needed": 0}
        none = GetBuffers(None, None, None, 0)
        assert lib.dbeel_gpu_reader_get_entries(
            h, None, None, 0, ctypes.byref(none), ctypes.byref(pg), None) == 0
        assert rd.get_entries([]) == []
        hh, oo, view, page, _ = rd.get_entries_raw([])
        assert len(hh) == 0 and oo.tolist() == [0] and len(view) == 0
        # NULL records is legal with cap 0
        zero = GetBuffers(hp, rp, None, 0)
        assert lib.dbeel_gpu_reader_get_entries(
            h, kp, op, n, ctypes.byref(zero), ctypes.byref(pg),
            None) in (0, ITEM_TOO_LARGE)
        assert pg.records_total == before[4]["records_total"]

        # the reader answers as before
        assert rd.table_bytes == tb
        after = _call(rd, keys)
        assert after[1].tobytes() == before[1].tobytes()
        assert after[2].tobytes() == before[2].tobytes()
        assert after[3] == before[3] and after[4] == before[4]


def test_zero_length_key_is_legal():
    run = build_run([Entry(b"", b"empty-key-value", 5), Entry(b"a", b"", 6)])
    with Reader([run], device=0) as rd:
        _check(rd, gem.Model([run]), [b"a", b"", b"", b"b"])
        assert rd.get_entries([b"", b"a", b"b"]) == [
            (b"empty-key-value", 5), (b"", 6), None]


# ---- 8. compact_fetch ----

@pytest.mark.parametrize("keep", [True, False], ids=["keep", "drop"])
def test_compact_fetch(keep):
    runs = [batch_model_run(s) for s in (1, 2, 3)]
    od, oi, _ = oracle.compact(runs[:2], keep)
    assert od and oi
    with Reader(runs, device=0) as rd:
        small = np.zeros(8, dtype=np.uint8)
        with pytest.raises(DbeelGpuError) as ei:   # nothing pending
            rd.compact_fetch_into(small, small)
        assert ei.value.code == INVALID_ARG
        data, index, _, _ = rd.compact_begin([0, 1], keep, fetch=True)
        assert (data, index) == (od, oi)
        darr = np.full(len(od) + 64, GUARD, dtype=np.uint8)
        iarr = np.full(len(oi) + 64, GUARD, dtype=np.uint8)
        # a short data cap, then a short index cap: the sizes needed, nothing
        # written, the pending table kept
        for d, i in ((darr[:len(od) - 1], iarr), (darr, iarr[:len(oi) - 1]),
                     (darr[:0], iarr[:0])):
            with pytest.raises(DbeelGpuError) as ei:
                rd.compact_fetch_into(d, i)
            assert ei.value.code == ITEM_TOO_LARGE
            assert (ei.value.data_len, ei.value.index_len) == \
                (len(od), len(oi))
            assert np.all(darr == GUARD) and np.all(iarr == GUARD)
        for pinned in (False, True, False):
            darr[:] = GUARD
            iarr[:] = GUARD
            if pinned:
                pin_host(darr)
                pin_host(iarr)
            try:
                dl, il, ms = rd.compact_fetch_into(darr[:len(od)],
                                                   iarr[:len(oi) + 7])
            finally:
                if pinned:
                    unpin_host(darr)
                    unpin_host(iarr)
            assert (dl, il) == (len(od), len(oi)) and ms >= 0.0
            assert darr[:dl].tobytes() == od and iarr[:il].tobytes() == oi
            assert np.all(darr[dl:] == GUARD) and np.all(iarr[il:] == GUARD)
        rd.compact_commit(0)
        with pytest.raises(DbeelGpuError) as ei:   # nothing pending any more
            rd.compact_fetch_into(darr, iarr)
        assert ei.value.code == INVALID_ARG
        new_runs = [(od, oi), runs[2]]
        _same_as_fresh(rd, new_runs, POOL)
        # begin without a host copy, fetch, abort: the list is unchanged
        od2, oi2, _ = oracle.compact(new_runs, keep)
        rd.compact_begin([0, 1], keep, fetch=False)
        darr = np.full(len(od2) + 64, GUARD, dtype=np.uint8)
        iarr = np.full(len(oi2) + 64, GUARD, dtype=np.uint8)
        dl, il, _ = rd.compact_fetch_into(darr, iarr)
        assert darr[:dl].tobytes() == od2 and iarr[:il].tobytes() == oi2
        assert np.all(darr[dl:] == GUARD) and np.all(iarr[il:] == GUARD)
        rd.compact_abort()
        _same_as_fresh(rd, new_runs, POOL)


def test_compact_fetch_empty_output():
    runs, _, drop = load_golden("all_tombstones")
    assert drop == (b"", b"")
    darr = np.full(64, GUARD, dtype=np.uint8)
    iarr = np.full(64, GUARD, dtype=np.uint8)
    with Reader(runs, device=0) as rd:
        rd.compact_begin(list(range(len(runs))), False, fetch=False)
        assert rd.compact_fetch_into(darr, iarr)[:2] == (0, 0)
        assert np.all(darr == GUARD) and np.all(iarr == GUARD)
        rd.compact_commit(0)
        assert rd.n_runs == 1
        key = next(e.key for d, i in runs for e in parse_run(d, i))
        assert rd.get_entries([key]) == [None]
