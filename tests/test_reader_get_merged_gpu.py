"""GPU tests of dbeel_gpu_reader_get_merged (engine.Reader.get_merged_raw /
get_merged / get_replicated), include/dbeel_gpu.h.

The host model is merge_model: the reference's replicated get — the sources'
answers in order, the local one last, max_by_key(timestamp) with the last
maximum winning, the tombstone test only afterwards — over
get_entries_model readers and raw answer pairs. Every call below goes through
_call, which hands the engine buffers with canary bytes behind hits,
record_offsets and records and checks that nothing past the result was
written; every comparison with the model is field by field and byte by byte.
"""
import ctypes

import numpy as np
import pytest

import get_entries_model as gem
import memtable_model
import merge_model as mm
from dbeel_amd.engine import (MERGE_HIT_DTYPE, DbeelGpuError, GetPage,
                              MergeBuffers, MergeHit, MergeSource, MergeStats,
                              Reader, _key_blob, pin_host, unpin_host)
from dbeel_amd.format import Entry, build_run

pytestmark = pytest.mark.gpu

INVALID_ARG, CORRUPT, ITEM_TOO_LARGE = 1, 2, 3
HIT_FIELDS = ("source", "is_tombstone", "value_len", "stale_mask")
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
GUARD = 0xA5
GUARD64 = 0xA5A5A5A5A5A5A5A5
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)


def _run(entries):
    """(key, data, ts) triples -> one run, keys sorted."""
    return build_run([Entry(*e) for e in sorted(entries)])


def _pair(model, keys):
    """A replica's get_entries answer as the arrays the call takes."""
    off, rec = mm.answers_of(model, keys)
    return (np.array(off, dtype=np.uint64),
            np.frombuffer(rec, dtype=np.uint8).copy())


def _call(rd, keys, sources, cap=None, pinned=False):
    """One get_merged call into guarded buffers. cap None = a first call with
    cap 0 learns records_total, then the call proper.
    -> (rc, hits, offsets, delivered bytes, page dict, stats dict)."""
    n = len(keys)
    ka, koff = _key_blob(keys)
    srcs, keep = Reader._merge_sources(sources)
    ns = len(sources)
    if cap is None:
        h0 = np.zeros(n, dtype=MERGE_HIT_DTYPE)
        o0 = np.zeros(n + 1, dtype=np.uint64)
        rc, pg, _ = rd._get_merged_into(ka, koff, srcs, ns, h0, o0, None, 0)
        assert rc in (0, ITEM_TOO_LARGE)
        cap = int(pg.records_total)
    hits = np.frombuffer(bytes([GUARD]) * ((n + 2) * MERGE_HIT_DTYPE.itemsize),
                         dtype=MERGE_HIT_DTYPE).copy()
    roff = np.full(n + 1 + 2, GUARD64, dtype=np.uint64)
    rec = np.full(cap + 64, GUARD, dtype=np.uint8)
    if pinned:
        pin_host(rec)
    try:
        rc, page, st = rd._get_merged_into(ka, koff, srcs, ns, hits, roff,
                                           rec, cap)
    finally:
        if pinned:
            unpin_host(rec)
    del keep
    page, st = page.as_dict(), st.as_dict()
    assert np.all(hits[n:].view(np.uint8) == GUARD), "hits guard"
    assert np.all(roff[n + 1:] == GUARD64), "offsets guard"
    rl = page["records_len"]
    assert rl <= cap
    assert np.all(rec[rl:] == GUARD), "bytes at or past records_len"
    if rc == CORRUPT:  # nothing at all may have been written
        assert np.all(hits.view(np.uint8) == GUARD)
        assert np.all(roff == GUARD64) and np.all(rec == GUARD)
    return rc, hits[:n].copy(), roff[:n + 1].copy(), rec[:rl].tobytes(), \
        page, st


def _hits_array(hits):
    return (np.array(hits, dtype=MERGE_HIT_DTYPE) if hits
            else np.zeros(0, dtype=MERGE_HIT_DTYPE))


def _check(rd, local, keys, sources, msources, cap=None, pinned=False):
    """The call's whole answer against the model's for the same cap. sources
    are what the engine gets (Readers and array pairs), msources the same
    candidates for the model (Models and pairs)."""
    ehits, eoff, erec, erc, epage = mm.expect(keys, local, msources, cap)
    rc, hits, roff, rec, page, st = _call(rd, keys, sources, cap, pinned)
    assert rc == erc
    assert page == epage
    eh = _hits_array(ehits)
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], eh[f]), f
    assert roff.tolist() == eoff
    assert rec == erec[:epage["records_len"]]
    if rc == 0:
        found = eh["source"] >= 0
        assert st["winners"] == int(found.sum())
        assert st["tombstones"] == int(eh["is_tombstone"].sum())
        assert st["from_local"] == int((eh["source"] == len(sources)).sum())
    return rc, hits, roff, rec, page, st


def _loop(rd, keys, sources, cap):
    """The stateless paging loop over the raw call: the remaining keys, every
    pair advanced and rebased. -> (hits, record bytes) concatenated."""
    hits_all, blob = [], b""
    p = 0
    while p < len(keys):
        sl = [s if isinstance(s, Reader)
              else (s[0][p:] - s[0][p], s[1][int(s[0][p]):])
              for s in sources]
        rc, hits, roff, rec, page, _ = _call(rd, keys[p:], sl, cap)
        assert rc == 0 and page["n_done"] > 0
        assert len(rec) == page["records_len"] == int(roff[page["n_done"]])
        hits_all.append(hits[:page["n_done"]])
        blob += rec
        p += page["n_done"]
    return np.concatenate(hits_all), blob


class _Trio:
    """Three small readers' worth of runs over overlapping keys, built once
    and read-only: 2-3 runs of at most 300 entries each."""

    def __init__(self, seed=5):
        rng = np.random.default_rng(seed)
        pool = memtable_model.key_pool(seed, 400, max_klen=24)
        self.pool = pool
        self.runs = []
        for r in range(3):
            runs = []
            for _ in range(2 + (r == 0)):
                ks = sorted({pool[int(i)]
                             for i in rng.integers(0, len(pool), 150)})
                runs.append(_run([
                    (k, b"" if rng.random() < 0.1 else
                     memtable_model.rand_bytes(rng, rng.integers(1, 70)),
                     int(rng.integers(0, 6)) if rng.random() < 0.3
                     else int(rng.integers(-10**12, 10**12)))
                    for k in ks]))
            self.runs.append(runs)
        self.models = [gem.Model(r) for r in self.runs]
        self.absent = [b"\xfe-absent-%d" % i for i in range(40)]


@pytest.fixture(scope="module")
def trio():
    return _Trio()


# ---- 1. equivalence with get_entries ----

@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
def test_no_sources_is_get_entries(trio, cut):
    keys = trio.pool[::2] + trio.absent + trio.pool[:5]
    with Reader(trio.runs[0], device=0) as rd:
        eh, eoff, eview, epage, _ = rd.get_entries_raw(keys)
        cap = int(eoff[len(keys) // 2]) + 3 if cut else int(eoff[-1])
        eh, eoff, eview, epage, _ = rd.get_entries_raw(keys, records_cap=cap)
        rc, hits, roff, rec, page, st = _check(rd, trio.models[0], keys, [],
                                               [], cap)
    assert rc == 0 and page == epage
    assert (page["n_done"] < len(keys)) == cut
    assert np.array_equal(roff, eoff) and rec == eview.tobytes()
    assert np.array_equal(hits["source"], np.where(eh["run"] >= 0, 0, -1))
    assert np.array_equal(hits["value_len"], eh["value_len"])
    assert np.array_equal(hits["is_tombstone"], eh["is_tombstone"])
    assert not hits["stale_mask"].any()


# ---- 2. timestamp order ----

def test_timestamp_order():
    """Per key three timestamps, the greatest placed at each candidate in
    turn: differing only in the low half with bit 63 set, only in the high
    half, negative, and the i128 extremes."""
    triples = [
        ((1 << 63) - 1, 1 << 63, (1 << 63) + 1),        # low half, bit 63
        (1, (1 << 63) | 1, (1 << 64) - 1),
        (1 << 64, 2 << 64, 3 << 64),                    # high half only
        ((1 << 64) | (1 << 63), 2 << 64, (2 << 64) | 1),
        (-3, -2, -1),                                   # negative
        (-(1 << 64), -(1 << 63), -1),
        (-(2 << 64), -(1 << 64) - 1, -(1 << 64)),
        (I128_MIN, 0, I128_MAX),
        (I128_MIN, I128_MIN + 1, -1),
        (-1, 0, 1 << 63),
        (1 << 64, I128_MAX - 1, I128_MAX),
    ]
    ents = [[], [], []]
    keys, want = [], []
    for i, tr in enumerate(triples):
        assert tr[0] < tr[1] < tr[2]
        for rot in range(3):
            k = b"t%02d-%d" % (i, rot)
            keys.append(k)
            for c in range(3):
                # candidate c holds the greatest when c == rot
                t = tr[2] if c == rot else tr[(c - rot - 1) % 3 % 2]
                ents[c].append((k, b"cand%d" % c, t))
            want.append(rot)
    models = [gem.Model([_run(e)]) for e in ents]
    local = models[2]
    msrc = [models[0], models[1]]
    with Reader([_run(ents[2])], device=0) as rd:
        src = [_pair(m, keys) for m in msrc]
        rc, hits, roff, rec, page, _ = _check(rd, local, keys, src,
                                              [tuple(s) for s in src])
        got = rd.get_merged(keys, src)
    assert rc == 0 and hits["source"].tolist() == want
    assert [g[2] for g in got] == want
    assert got == mm.merged(keys, local, msrc)
    assert all(int(h["stale_mask"]) == 0b111 & ~(1 << int(h["source"]))
               for h in hits)


# ---- 3. ties ----

def test_ties():
    ents = [[], [], []]

    def put(k, *ts):
        for c, t in enumerate(ts):
            if t is not None:
                ents[c].append((k, b"%s-by-%d" % (k, c), t))

    put(b"all-tie", 7, 7, 7)          # the highest index, local, wins
    put(b"remote-tie", 7, 7, None)    # 1 wins, local absent -> stale
    put(b"tie-01-old2", 9, 9, 3)      # 1 wins, local older
    put(b"tie-02", 5, 1, 5)           # local ties with remote 0: local wins
    put(b"tie-12-absent0", None, -4, -4)
    put(b"tie-max", I128_MAX, I128_MAX, I128_MAX - 1)
    put(b"tie-min", I128_MIN, None, I128_MIN)
    for e in ents:
        e.append((b"zz-pad", b"p", 0))
    keys = [b"all-tie", b"remote-tie", b"tie-01-old2", b"tie-02",
            b"tie-12-absent0", b"tie-max", b"tie-min"]
    models = [gem.Model([_run(e)]) for e in ents]
    with Reader([_run(ents[2])], device=0) as rd, \
            Reader([_run(ents[1])], device=0) as r1:
        src = [_pair(models[0], keys), r1]
        rc, hits, roff, rec, page, _ = _check(rd, models[2], keys, src,
                                              [models[0], models[1]])
        got = rd.get_merged(keys, src)
    assert hits["source"].tolist() == [2, 1, 1, 2, 2, 1, 2]
    assert hits["stale_mask"].tolist() == [0, 0b100, 0b100, 0b010, 0b001,
                                           0b100, 0b010]
    assert got[0] == (b"all-tie-by-2", 7, 2)
    assert got[3] == (b"tie-02-by-2", 5, 2)
    assert got[5] == (b"tie-max-by-1", I128_MAX, 1)


# ---- 4. tombstones, 5. absent keys ----

def test_tombstones_and_absent_keys():
    ents = [
        [(b"dead-new", b"", 50), (b"dead-old", b"", 1), (b"only-dead", b"", 0),
         (b"pad", b"p", 0)],
        [(b"dead-new", b"value", 49), (b"dead-old", b"kept", 2),
         (b"dead-tie", b"", 5), (b"pad", b"p", 0)],
        [(b"dead-new", b"older", -50), (b"dead-tie", b"alive", 5),
         (b"pad", b"p", 0)],
    ]
    keys = [b"dead-new", b"dead-old", b"only-dead", b"dead-tie", b"nowhere",
            b"", b"nowhere"]
    models = [gem.Model([_run(e)]) for e in ents]
    with Reader([_run(ents[2])], device=0) as rd:
        src = [_pair(models[0], keys), _pair(models[1], keys)]
        rc, hits, roff, rec, page, st = _check(rd, models[2], keys, src,
                                               models[:2])
        assert rd.get_replicated(keys, src) == \
            [None, b"kept", None, b"alive", None, None, None]
        assert rd.get_merged(keys, src)[:4] == [
            (b"", 50, 0), (b"kept", 2, 1), (b"", 0, 0), (b"alive", 5, 2)]
    assert hits["source"].tolist() == [0, 1, 0, 2, -1, -1, -1]
    assert hits["is_tombstone"].tolist() == [1, 0, 1, 0, 0, 0, 0]
    # a winning tombstone is a 24-byte record: data_len 0 and its timestamp
    assert rec[:24] == bytes(8) + (50).to_bytes(16, "little", signed=True)
    # nobody holds the key: an empty range and no stale bit
    assert roff[4] == roff[5] == roff[6] == roff[7]
    assert hits["stale_mask"][4:].tolist() == [0, 0, 0]
    assert hits["stale_mask"][:4].tolist() == [0b110, 0b101, 0b110, 0b001]
    assert st["winners"] == 4 and st["tombstones"] == 2


# ---- 6. sizes and alignment ----

VLENS = [0, 1, 7, 8, 9, 63, 64, 65, 200_000]


class _Sizes:
    """257 + keys of 0..9 bytes so records sit at every alignment in the
    tables; the winner of key i is candidate i % 3, its value length cycling
    through VLENS, the losers carrying other lengths."""

    def __init__(self):
        rng = np.random.default_rng(21)
        keys = [b""] + sorted({memtable_model.rand_bytes(
            rng, rng.integers(1, 10)) for _ in range(300)})[:259]
        self.keys = keys
        ents = [[], [], []]
        big = 0
        for i, k in enumerate(keys):
            vl = VLENS[i % len(VLENS)]
            if vl == 200_000:
                big += 1
                if big > 1:
                    vl = 33
            for c in range(3):
                if c == i % 3:
                    data = memtable_model.rand_bytes(rng, vl)
                    ents[c].append((k, data, 1000 + i))
                elif (i + c) % 4:
                    ents[c].append((k, memtable_model.rand_bytes(
                        rng, VLENS[(i + c) % 8]), int(rng.integers(0, 999))))
        self.runs = [[_run(e[0::2]), _run(e[1::2])] for e in ents]
        self.models = [gem.Model(r) for r in self.runs]


@pytest.fixture(scope="module")
def sizes():
    return _Sizes()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_alignment_and_batch_shapes(sizes, n):
    z = sizes
    # the big value (key 8) is in every batch but the first; duplicates and
    # the zero-length key are in every batch of more than one key
    keys = [z.keys[8]] if n == 1 else (
        [z.keys[0], z.keys[8], z.keys[8]] + z.keys[1:n - 3] + [z.keys[0]])
    assert len(keys) == n
    with Reader(z.runs[2], device=0) as rd, \
            Reader(z.runs[1], device=0) as r1:
        src = [_pair(z.models[0], keys), r1]
        rc, hits, roff, rec, page, _ = _check(
            rd, z.models[2], keys, src, [z.models[0], z.models[1]],
            pinned=(n == 257))
    assert rc == 0 and page["n_done"] == n
    assert 200_000 in hits["value_len"].tolist()
    if n >= 63:
        assert set(VLENS) <= set(hits["value_len"].tolist())
        assert set(hits["source"].tolist()) == {0, 1, 2}
        assert len({int(o) % 8 for o in roff}) == 8  # every destination phase


# ---- 7. reader sources ----

def test_reader_sources_memtable_and_liveness(trio):
    keys = trio.pool[::3] + trio.absent[:5]
    m0, m1, m2 = trio.models
    with Reader(trio.runs[0], device=0) as rd, \
            Reader(trio.runs[1], device=0) as r1, \
            Reader(trio.runs[2], device=0) as r2:
        tb = (rd.table_bytes, r1.table_bytes)
        _check(rd, m0, keys, [r1, r2], [m1, m2])
        # a put into a source changes the winner of the next call: the call
        # is live and keeps nothing
        k_new, k_old = keys[0], keys[1]
        mt = memtable_model.Memtable()
        writes = [(k_new, b"from-r2-memtable", 10**15),
                  (k_old, b"too-old", -10**15),
                  (trio.absent[0], b"", 10**15 + 1)]
        mt.put(writes)
        r2.put(writes)
        m2b = gem.Model(trio.runs[2], mt)
        rc, hits, roff, rec, page, _ = _check(rd, m0, keys, [r1, r2],
                                              [m1, m2b])
        got = rd.get_merged(keys, [r1, r2])
        assert got[0] == (b"from-r2-memtable", 10**15, 1)
        assert got ==mm.merged(keys, m0, [m1, m2b])
        q = keys.index(trio.absent[0])
        assert hits["source"][q] == 1 and hits["is_tombstone"][q] == 1
        assert rd.get_replicated(keys, [r1, r2])[q] is None
        # the local reader's own memtable, and the sources' plain gets, are
        # as they were
        mtl = memtable_model.Memtable()
        wl = [(k_new, b"local-newest", 10**15 + 5)]
        mtl.put(wl)
        rd.put(wl)
        m0b = gem.Model(trio.runs[0], mtl)
        _check(rd, m0b, keys, [r2, r1], [m2b, m1], cap=500)
        assert rd.get_merged(keys[:1], [r2, r1]) == \
            [(b"local-newest", 10**15 + 5, 2)]
        assert r2.get_entries(keys) == m2b.entries(keys)
        assert r1.get_entries(keys) == m1.entries(keys)
        assert (rd.table_bytes, r1.table_bytes) == tb  # scratch not counted


# ---- 8. source count ----

def test_fifteen_sources_winner_in_each_position():
    n_c = 16
    ents = [[(b"pad", b"p", 0)] for _ in range(n_c)]
    keys = []
    for w in range(n_c):
        k = b"win-at-%02d" % w
        keys.append(k)
        for c in range(n_c):
            if (c + w) % 5 == 4 and c != w:
                continue  # some candidates do not hold the key
            ents[c].append((k, b"v%d/%d" % (c, w) * (1 + c % 3),
                            100 if c == w else (c * 7 + w) % 90))
    keys += [b"pad", b"none"]
    models = [gem.Model([_run(e)]) for e in ents]
    readers = {3: None, 9: None, 14: None}
    try:
        for c in readers:
            readers[c] = Reader([_run(ents[c])], device=0)
        with Reader([_run(ents[15])], device=0) as rd:
            src = [readers[c] if c in readers else _pair(models[c], keys)
                   for c in range(15)]
            rc, hits, roff, rec, page, _ = _check(rd, models[15], keys, src,
                                                  models[:15])
            got = rd.get_merged(keys, src, page_bytes=64)
    finally:
        for r in readers.values():
            if r is not None:
                r.close()
    assert hits["source"].tolist() == list(range(16)) + [15, -1]
    assert hits["stale_mask"][16] == 0  # sixteen candidates tie on "pad"
    assert got == mm.merged(keys, models[15], models[:15])
    assert [g[2] for g in got[:16]] == list(range(16))


# ---- 9. paging ----

def test_paging(trio):
    keys = trio.pool[1::2][:150] + trio.absent[:3]
    m0, m1, m2 = trio.models
    with Reader(trio.runs[0], device=0) as rd, \
            Reader(trio.runs[1], device=0) as r1:
        src = [r1, _pair(m2, keys)]
        msrc = [m1, m2]
        rc, hits, roff, rec, page, _ = _check(rd, m0, keys, src, msrc)
        assert rc == 0 and page["n_done"] == len(keys)
        total = page["records_total"]
        one = max(int(roff[q + 1] - roff[q]) for q in range(len(keys)))
        for cap in (one, total // 3):
            _check(rd, m0, keys, src, msrc, cap)
            lh, lblob = _loop(rd, keys, src, cap)
            for f in HIT_FIELDS:
                assert np.array_equal(lh[f], hits[f]), (cap, f)
            assert lblob == rec
        # cap 24: only tombstone winners and absent keys fit
        dead = [k for k, h in zip(keys, hits) if h["source"] < 0
                or h["is_tombstone"]]
        assert len(dead) > 3
        _check(rd, m0, dead, [r1, _pair(m2, dead)], msrc, 24)
        lh, lblob = _loop(rd, dead, [r1, _pair(m2, dead)], 24)
        eh, eoff, erec, _, _ = mm.expect(dead, m0, msrc)
        assert lblob == erec and lh["source"].tolist() == [h[0] for h in eh]
        # a first record over the cap: ITEM_TOO_LARGE, needed set, hits and
        # offsets complete (compared by _check)
        first = next(q for q in range(len(keys)) if hits["value_len"][q] > 0)
        sub = keys[first:]
        ssrc = [r1, _pair(m2, sub)]
        need = 24 + int(hits["value_len"][first])
        rc, h2, o2, rec2, pg2, _ = _check(rd, m0, sub, ssrc, msrc, need - 1)
        assert rc == ITEM_TOO_LARGE and rec2 == b""
        assert pg2 == {"n_done": 0, "records_len": 0,
                       "records_total": int(o2[-1]), "needed": need}
        assert np.array_equal(h2["source"], hits["source"][first:])
        with pytest.raises(DbeelGpuError) as ei:
            rd.get_merged_raw(sub, ssrc, records_cap=need - 1)
        assert ei.value.code == ITEM_TOO_LARGE
        assert ei.value.page["needed"] == need
        assert np.array_equal(ei.value.record_offsets, o2)
        # the wrappers page, growing once for a record over the page
        assert rd.get_merged(keys, src, page_bytes=40) == \
            mm.merged(keys, m0, msrc)
        assert rd.get_replicated(keys, src, page_bytes=total // 3) == \
            mm.replicated(keys, m0, msrc)
        # n_keys == 0
        rc, h0, o0, rec0, pg0, _ = _call(rd, [], [r1, (np.zeros(
            1, dtype=np.uint64), np.zeros(0, dtype=np.uint8))], cap=16)
        assert rc == 0 and o0.tolist() == [0] and rec0 == b""
        assert pg0 == {"n_done": 0, "records_len": 0, "records_total": 0,
                       "needed": 0}
        assert rd.get_merged([], src[:1]) == []


# ---- 10. refusals ----

def test_host_refusals_in_header_order(trio):
    keys = trio.pool[:20]
    m0, m1, _ = trio.models
    ka, koff = _key_blob(keys)
    n = len(keys)
    with Reader(trio.runs[0], device=0) as rd, \
            Reader(trio.runs[1], device=0) as r1:
        lib = rd._lib
        hits = np.frombuffer(bytes([GUARD]) * (n * 24),
                             dtype=MERGE_HIT_DTYPE).copy()
        roff = np.full(n + 1, GUARD64, dtype=np.uint64)
        rec = np.full(4096, GUARD, dtype=np.uint8)
        good_off, good_rec = _pair(m1, keys)

        def buf(h=hits, o=roff, r=rec, cap=4096):
            return MergeBuffers(
                None if h is None else h.ctypes.data_as(
                    ctypes.POINTER(MergeHit)),
                None if o is None else o.ctypes.data_as(U64P),
                None if r is None else r.ctypes.data_as(U8P), cap)

        def answers(off=good_off, r=good_rec):
            s = MergeSource()
            s.kind = 0
            if off is not None:
                s.record_offsets = off.ctypes.data_as(U64P)
            if r is not None:
                s.records = r.ctypes.data_as(U8P)
            return s

        def reader(h):
            s = MergeSource()
            s.kind, s.reader = 1, h
            return s

        def kind(k):
            s = MergeSource()
            s.kind = k
            return s

        def refused(word, srcs, n_src=None, b=None, kp=ka, op=koff, nk=n,
                    local=rd._h):
            arr = (MergeSource * max(len(srcs), 1))(*srcs)
            page, st = GetPage(), MergeStats()
            page.n_done, st.winners = 9, 9
            b = buf() if b is None else b
            rc = lib.dbeel_gpu_reader_get_merged(
                local, None if kp is None else kp.ctypes.data_as(U8P),
                None if op is None else op.ctypes.data_as(U64P), nk,
                arr if srcs or n_src is None else None,
                len(srcs) if n_src is None else n_src, ctypes.byref(b),
                ctypes.byref(page), ctypes.byref(st))
            msg = lib.dbeel_gpu_last_error().decode()
            assert rc == INVALID_ARG, msg
            assert word in msg, msg
            assert page.n_done == 0 and st.winners == 0

        bad_kind, null_rd = kind(2), reader(None)
        null_off = answers(off=None)
        desc = good_off.copy()
        desc[2] = desc[3] + 1
        from1 = good_off + 1
        # 1 comes before everything (a NULL local with bad everything else)
        refused("null reader", [bad_kind], local=None, kp=None)
        # 2: get_entries' checks come before any look at the sources
        refused("null keys", [bad_kind], kp=None)
        refused("null keys", [bad_kind], b=buf(h=None))
        refused("null keys", [bad_kind], b=buf(o=None))
        refused("null records", [bad_kind], b=buf(r=None))
        refused("2^32", [bad_kind], nk=1 << 32)
        bad_koff = koff.copy()
        bad_koff[2] = bad_koff[3] + 1
        refused("not ascending", [bad_kind], op=bad_koff)
        # 3 before 4
        refused("at most 15", [bad_kind] * 16)
        refused("null sources", [], n_src=2)
        # 4 before 5, whatever the position
        refused("unknown kind", [null_rd, bad_kind])
        refused("unknown kind", [kind(-1)])
        # 5 before 6
        refused("no reader", [null_off, null_rd])
        refused("local reader itself", [null_off, reader(rd._h)])
        # 6 before 7
        refused("null record_offsets", [answers(off=desc), null_off])
        refused("null records", [answers(off=from1), answers(r=None)])
        # 7
        refused("start at", [answers(off=from1)])
        refused("not ascending", [answers(), answers(off=desc)])
        # a NULL records with no record bytes is legal
        empty = np.zeros(n + 1, dtype=np.uint64)
        assert np.all(hits.view(np.uint8) == GUARD)
        assert np.all(roff == GUARD64) and np.all(rec == GUARD)
        # and the readers answer as ever
        _check(rd, m0, keys, [(empty, None), r1, (good_off, good_rec)],
               [(empty.tolist(), b""), m1, (good_off.tolist(),
                                            good_rec.tobytes())])


def test_corrupt_answers(trio):
    keys = trio.pool[:40]
    m0, m1, m2 = trio.models
    off, rec = mm.answers_of(m1, keys)
    q = next(i for i in range(len(keys))
             if off[i + 1] - off[i] > 24 and off[i] > 0)
    # a 23-byte record: query q's answer loses its last byte
    short_rec = rec[:off[q] + 23] + rec[off[q + 1]:]
    short_off = off[:q + 1] + [o - (off[q + 1] - off[q] - 23)
                               for o in off[q + 1:]]
    # a data_len that is off by one
    dl = int.from_bytes(rec[off[q]:off[q] + 8], "little")
    wrong = rec[:off[q]] + (dl + 1).to_bytes(8, "little") + rec[off[q] + 8:]
    arr = lambda o, r: (np.array(o, dtype=np.uint64),
                        np.frombuffer(r, dtype=np.uint8).copy())
    with Reader(trio.runs[0], device=0) as rd, \
            Reader(trio.runs[2], device=0) as r2:
        before = rd.get_entries_raw(keys)
        for bad in (arr(short_off, short_rec), arr(off, wrong)):
            rc, _, _, _, page, _ = _call(rd, keys, [r2, bad], cap=1 << 16)
            assert rc == CORRUPT
            msg = rd._lib.dbeel_gpu_last_error().decode()
            assert "source 1" in msg and "query %d" % q in msg
            assert page == {"n_done": 0, "records_len": 0,
                            "records_total": 0, "needed": 0}
            with pytest.raises(DbeelGpuError) as ei:
                rd.get_merged(keys, [r2, bad])
            assert ei.value.code == CORRUPT
            # the next valid call on the same readers is correct
            _check(rd, m0, keys, [r2, arr(off, rec)], [m2, m1])
        after = rd.get_entries_raw(keys)
        assert np.array_equal(before[1], after[1])
        assert before[2].tobytes() == after[2].tobytes()
        assert r2.get_entries(keys) == m2.entries(keys)


# ---- 11. random ----

@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random(seed):
    rng = np.random.default_rng(1000 + seed)
    pool = memtable_model.key_pool(seed, 500, max_klen=20)

    def runs():
        out = []
        for _ in range(int(rng.integers(2, 4))):
            ks = sorted({pool[int(i)] for i in rng.integers(0, len(pool), 90)})
            out.append(_run([
                (k, b"" if rng.random() < 0.1 else
                 memtable_model.rand_bytes(rng, rng.integers(1, 50)),
                 int(rng.integers(0, 4)) if rng.random() < 0.3
                 else int(rng.integers(-10**9, 10**9)) << int(
                     rng.integers(0, 80)))
                for k in ks]))
        return out

    sets = [runs() for _ in range(5)]
    models = [gem.Model(r) for r in sets]
    keys = [pool[int(i)] for i in rng.integers(0, len(pool), 960)] + \
        [b"\xfd-none-%d" % i for i in range(40)]
    with Reader(sets[0], device=0) as rd, \
            Reader(sets[1], device=0) as r1, \
            Reader(sets[2], device=0) as r2:
        order = rng.permutation(4)
        cands = [(r1, models[1]), (r2, models[2]),
                 (_pair(models[3], keys), models[3]),
                 (_pair(models[4], keys), models[4])]
        src = [cands[int(i)][0] for i in order]
        msrc = [cands[int(i)][1] for i in order]
        _, eoff, _, _, _ = mm.expect(keys, models[0], msrc)
        cap = int(rng.integers(eoff[1], eoff[-1] + 1))
        rc, hits, roff, rec, page, _ = _check(rd, models[0], keys, src, msrc,
                                              cap)
        assert rc == 0
        assert len(set(hits["source"].tolist())) == 6  # -1 and every candidate
        assert rd.get_merged(keys, src, page_bytes=cap) == \
            mm.merged(keys, models[0], msrc)
        assert rd.get_replicated(keys, src, page_bytes=1 << 14) == \
            mm.replicated(keys, models[0], msrc)
