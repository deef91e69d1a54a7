"""GPU tests of the reader's resident memtable (engine.Reader.put /
memtable_info / memtable_fetch / memtable_flush / memtable_clear and
lsm.reader_memtable_flush): puts accumulate with the reference's
last-arrival-wins rule across batches (rbtree_arena/src/lib.rs:497-511), gets
consult the memtable before every table (lsm_tree.rs:676-685), and a flush
turns it into the newest table (lsm_tree.rs:850-915).

Oracle: tests/memtable_model.py (batch_model.flush_run over the concatenated
arrivals) for the bytes and counts, and a FRESH Reader over
tables + [model run] for the answers — never the code under test.
"""
import ctypes
import os

import numpy as np
import pytest

import batch_model
import memtable_model
import oracle
from dbeel_amd import engine, lsm
from dbeel_amd.engine import DbeelGpuError, Job, Reader
from dbeel_amd.format import Entry, build_run
from memtable_model import I128_MAX, I128_MIN, Memtable, gen, key_pool

pytestmark = pytest.mark.gpu

INVALID_ARG, ITEM_TOO_LARGE, IO = 1, 3, 7
HIT_FIELDS = ("run", "is_tombstone", "value_offset", "value_len")
ABSENT = [b"\xfe" * 9, b"absent", b"\x00" * 41, b"zz"]


@pytest.fixture(params=["radix", "merge"])
def order(request, monkeypatch):
    """The order stage's environment switch, read by the engine per call."""
    monkeypatch.setenv("DBEEL_BATCH_ORDER", request.param)
    return request.param


def _code(fn, *a, **kw):
    with pytest.raises(DbeelGpuError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _run_bloom(run):
    with Job([run], device=0) as job:
        job.run(True)
        return job.bloom()


# the key pool every generated batch draws from, and the reader the tests
# start from: two small runs over that pool, the older one with a filter
POOL = key_pool(7, 1500)
_BASE = None


def _base():
    """-> (runs, blooms), built once and never changed."""
    global _BASE
    if _BASE is None:
        older = batch_model.flush_run(gen(1, 300, POOL[::3]))
        newer = batch_model.flush_run(gen(2, 200, POOL[1::4]))
        _BASE = ([older, newer], [_run_bloom(older), None])
    return _BASE


def _run_keys(run):
    data, index = run
    rec = np.frombuffer(index, dtype="<u8").reshape(-1, 2)
    out = []
    for off, sizes in rec.tolist():
        ks = sizes & 0xFFFFFFFF
        out.append(bytes(data[off + 8:off + ks]))
    return out


def _assert_raw_equal(got, exp):
    hits, voff, values, _ = got
    ehits, evoff, evalues, _ = exp
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], ehits[f]), f
    assert np.array_equal(voff, evoff)
    assert values.tobytes() == evalues.tobytes()


def _assert_answers(rd, tables, blooms, model, keys):
    """rd (tables + memtable) answers raw-equal to a fresh reader over
    tables + [the model's run]; memtable hits sit at run == len(tables)."""
    mrun = model.run()
    runs = list(tables) + ([mrun] if model.entries else [])
    bl = list(blooms) + ([None] if model.entries else [])
    got = rd.get_raw(keys)
    with Reader(runs, blooms=bl, device=0) as fresh:
        exp = fresh.get_raw(keys)
    _assert_raw_equal(got, exp)
    held = set(model.keys())
    for q, k in enumerate(keys):
        assert (got[0]["run"][q] == len(tables)) == (k in held), k
    # a non-empty memtable counts as one visit to an unfiltered run: the
    # counters are the fresh reader's, where it IS the newest unfiltered run
    for f in ("bloom_probes", "bloom_skips", "searches", "hits",
              "tombstones"):
        assert got[3][f] == exp[3][f], f


def _assert_memtable(rd, model):
    info = rd.memtable_info
    assert info["entries"] == model.entries
    assert info["data_bytes"] == model.data_bytes
    assert rd.memtable_fetch() == model.run()


def _put(rd, model, writes):
    """One put on both sides, stats and state checked against the model."""
    m_before = model.entries
    batch_entries, replaced = model.put(writes)
    st = rd.put(writes)
    assert st["writes_in"] == len(writes)
    assert st["batch_entries"] == batch_entries
    assert st["replaced"] == replaced
    assert st["entries"] == model.entries == m_before + batch_entries - replaced
    assert st["data_bytes"] == model.data_bytes
    assert st["prefix_tied"] == batch_model.prefix_tied(writes)
    _assert_memtable(rd, model)
    return st


# ---- 1. chain parity ----

def test_chain_parity(order):
    tables, blooms = _base()
    base_keys = [k for r in tables for k in _run_keys(r)]
    model = Memtable()
    with Reader(tables, blooms=blooms, device=0) as rd:
        tb = rd.table_bytes
        for j, n in enumerate((1, 2, 63, 64, 65, 257, 1000, 4097)):
            writes = gen(100 + j, n, POOL)
            _put(rd, model, writes)
            assert rd.memtable_info["puts"] == j + 1
            keys = model.keys() + base_keys + ABSENT
            _assert_answers(rd, tables, blooms, model, keys)
        assert rd.n_runs == 2 and rd.table_bytes == tb


def test_empty_memtable_changes_nothing():
    tables, blooms = _base()
    keys = _run_keys(tables[0])[::5] + ABSENT
    with Reader(tables, blooms=blooms, device=0) as rd, \
            Reader(tables, blooms=blooms, device=0) as fresh:
        tb = rd.table_bytes
        exp = fresh.get_raw(keys)
        st = rd.put([])
        assert st["writes_in"] == 0 and st["entries"] == 0
        assert rd.memtable_info == {"entries": 0, "data_bytes": 0,
                                    "reserved_bytes": 0, "puts": 0}
        assert rd.memtable_fetch() == (b"", b"")
        got = rd.get_raw(keys)
        _assert_raw_equal(got, exp)
        assert got[3]["searches"] == exp[3]["searches"]
        # used and emptied again: the same answers and counters
        rd.put(gen(5, 50, POOL))
        rd.memtable_clear()
        got = rd.get_raw(keys)
        _assert_raw_equal(got, exp)
        assert got[3]["searches"] == exp[3]["searches"]
        assert rd.table_bytes == tb == fresh.table_bytes


# ---- 2. last arrival wins across puts ----

def test_last_arrival_wins_across_puts(order):
    live = build_run([Entry(b"k-live", b"base-value", 50),
                      Entry(b"k-other", b"other", 1)])
    dead = build_run([Entry(b"k-dead", b"", 60), Entry(b"k-other", b"top", 2)])
    tables = [live, dead]
    model = Memtable()
    with Reader(tables, device=0) as rd:
        # the earlier put carries the larger timestamp
        _put(rd, model, [(b"key", b"first", 300), (b"k-live", b"x", I128_MAX)])
        _put(rd, model, [(b"key", b"second", 200), (b"k-dead", b"", 9)])
        _put(rd, model, [(b"key", b"third", I128_MIN),
                         (b"k-live", b"", 1),          # tombstone over live
                         (b"k-dead", b"reborn", 0)])   # live over a tombstone
        assert rd.memtable_fetch() == build_run([
            Entry(b"k-dead", b"reborn", 0), Entry(b"k-live", b"", 1),
            Entry(b"key", b"third", I128_MIN)])
        keys = [b"key", b"k-live", b"k-dead", b"k-other", b"nope"]
        hits, _, _, _ = rd.get_raw(keys)
        assert rd.get(keys) == [b"third", b"", b"reborn", b"top", None]
        assert hits["run"].tolist() == [2, 2, 2, 1, -1]
        assert hits["is_tombstone"].tolist() == [0, 1, 0, 0, 0]
        _assert_answers(rd, tables, [None, None], model, keys)


# ---- 3. position classes of B against M ----

def _k(j):
    return b"key-%05d" % j


POSITION_CASES = {
    "b_below_m": ([_k(j) for j in range(100, 140)],
                  [_k(j) for j in range(0, 30)]),
    "b_above_m": ([_k(j) for j in range(0, 30)],
                  [_k(j) for j in range(100, 140)]),
    "identical": ([_k(j) for j in range(70)], [_k(j) for j in range(70)]),
    "interleaved": ([_k(j) for j in range(0, 160, 2)],
                    [_k(j) for j in range(1, 160, 2)]),
    "one_one_equal": ([b"solo"], [b"solo"]),
    "one_one_below": ([b"solo"], [b"rolo"]),
    "one_one_above": ([b"solo"], [b"tolo"]),
    "empty_key_in_m": ([b"", b"b", b"d"], [b"a", b"c"]),
    "empty_key_in_b": ([b"a", b"c"], [b"", b"b", b"d"]),
    "empty_key_in_both": ([b"", b"c"], [b"", b"a"]),
}


@pytest.mark.parametrize("case", sorted(POSITION_CASES))
def test_position_classes(order, case):
    mkeys, bkeys = POSITION_CASES[case]
    tables, blooms = _base()
    model = Memtable()
    # arrival order reversed: the order stage has work to do
    w1 = [(k, b"m-" + k, j) for j, k in enumerate(reversed(mkeys))]
    w2 = [(k, b"" if j % 5 == 4 else b"b-" + k * 2, -j)
          for j, k in enumerate(reversed(bkeys))]
    with Reader(tables, blooms=blooms, device=0) as rd:
        _put(rd, model, w1)
        st = _put(rd, model, w2)
        if case == "identical":
            assert st["replaced"] == len(mkeys) == st["entries"]
        _assert_answers(rd, tables, blooms, model,
                        sorted(set(mkeys + bkeys)) + ABSENT)


def test_values_of_every_copy_class(order):
    """Values of ~100 B, ~1 KiB and ~4 KiB, so the merge's verbatim copy
    takes each of its window geometries over the memtable's buffers, with
    odd sizes and more than one window."""
    rng = np.random.default_rng(55)
    tables, blooms = _base()
    for vlen in (97, 1031, 4099):
        model = Memtable()
        keys = [b"val-%04d" % j for j in range(90)]
        w1 = [(k, memtable_model.rand_bytes(rng, vlen + j % 5), j)
              for j, k in enumerate(keys[:60])]
        w2 = [(k, memtable_model.rand_bytes(rng, vlen - j % 7), -j)
              for j, k in enumerate(keys[30:])]
        with Reader(tables, blooms=blooms, device=0) as rd:
            _put(rd, model, w1)
            assert _put(rd, model, w2)["replaced"] == 30
            _assert_answers(rd, tables, blooms, model, keys + ABSENT)


# ---- 4. prefix ties ----

def test_prefix_ties(order):
    rng = np.random.default_rng(31)
    family = sorted({b"user:000" + memtable_model.rand_bytes(
        rng, rng.integers(0, 33)) for _ in range(300)})
    padding = [b"ab", b"ab\0", b"ab\0\0", b"ab" + b"\0" * 7]
    keys = family + padding
    order_ = rng.permutation(len(keys)).tolist()
    half = len(keys) // 2
    first = [(keys[i], b"one-%d" % i, i) for i in order_[:half + 40]]
    second = [(keys[i], b"" if i % 6 == 0 else b"two-%d" % i, -i)
              for i in order_[half - 40:]]  # 80 overwrites
    tables, blooms = _base()
    model = Memtable()
    with Reader(tables, blooms=blooms, device=0) as rd:
        _put(rd, model, first)
        st = _put(rd, model, second)
        assert st["replaced"] == 80 and st["entries"] == len(keys)
        _assert_answers(rd, tables, blooms, model,
                        keys + [b"user:000", b"ab\0\0\0", b"a"])


# ---- 5. flush ----

def _scan_all(pages):
    datas, indexes, off, total = [], [], 0, 0
    for d, x, n in pages:
        rec = np.frombuffer(x, dtype=engine.INDEX_DTYPE).copy()
        rec["offset"] += off
        datas.append(d)
        indexes.append(rec.tobytes())
        off += len(d)
        total += n
    return b"".join(datas), b"".join(indexes), total


@pytest.mark.parametrize("build_bloom", [False, True], ids=["plain", "bloom"])
def test_flush(order, build_bloom):
    tables, blooms = _base()
    model = Memtable()
    keys = POOL[::2] + ABSENT
    page = (np.empty(1 << 12, dtype=np.uint8),
            np.empty(16 * 16, dtype=np.uint8))
    with Reader(tables, blooms=blooms, device=0) as rd:
        sc = rd.scan_open()
        assert not sc.next(*page)["done"]
        _put(rd, model, gen(41, 700, POOL))
        _put(rd, model, gen(42, 300, POOL))
        # the scan opened before the puts is still valid
        assert sc.next(*page)["n_entries"]
        reserved = rd.memtable_info["reserved_bytes"]
        before = rd.get_raw(keys)
        d, i, bloom = rd.memtable_flush(build_bloom=build_bloom)
        assert (d, i) == model.run()
        assert rd.n_runs == 3
        assert rd.memtable_info == {"entries": 0, "data_bytes": 0,
                                    "reserved_bytes": reserved, "puts": 0}
        assert rd.memtable_fetch() == (b"", b"")
        # identical hits, offsets and value bytes before and after
        _assert_raw_equal(rd.get_raw(keys), before)
        # ... and stale after the flush
        assert _code(sc.next, *page) == INVALID_ARG
        sc.close()
        if build_bloom:
            cd, ci, cb, _ = rd.compact_begin([2], True, bloom=True)
            rd.compact_abort()
            assert (cd, ci) == (d, i)
            assert bloom == cb and bloom[:4] == b"DBLM"
        else:
            assert bloom is None
        all_runs = tables + [model.run()]
        all_blooms = blooms + [bloom]
        with Reader(all_runs, blooms=all_blooms, device=0) as fresh:
            _assert_raw_equal(rd.get_raw(keys), fresh.get_raw(keys))
            assert rd.table_bytes == fresh.table_bytes
        # flushing the now empty memtable: no table, and an open scan stays
        # valid
        sc = rd.scan_open()
        assert rd.memtable_flush(build_bloom=build_bloom) == (b"", b"", None)
        assert rd.memtable_flush(fetch=False) == (None, None, None)
        assert rd.n_runs == 3
        sc.next(*page)
        sc.close()


def test_scan_open_across_puts_sees_the_tables_alone(order):
    tables, blooms = _base()
    model = Memtable()
    with Reader(tables, blooms=blooms, device=0) as rd:
        pages = []
        for p, (d, x, n, _) in enumerate(rd.scan_pages(page_bytes=4096,
                                                        page_entries=64)):
            pages.append((d.tobytes(), x.tobytes(), n))
            if p < 3:
                _put(rd, model, gen(60 + p, 90, POOL))
        assert len(pages) > 3 and model.entries
        assert _scan_all(pages) == engine.scan(tables, device=0)
        assert rd.scan() == engine.scan(tables, device=0)


# ---- 6. limits and interplay ----

def test_reader_at_64_tables(order):
    tiny = [build_run([Entry(b"k%02d" % r, b"v%d" % r, r)]) for r in range(64)]
    model = Memtable()
    writes = [(b"k07", b"", 1), (b"new", b"value", 2), (b"k63", b"over", -3)]
    keys = [b"k%02d" % r for r in range(64)] + [b"new", b"none"]
    with Reader(tiny, device=0) as rd:
        tb = rd.table_bytes
        _put(rd, model, writes)
        _put(rd, model, [(b"new", b"value-2", 0)])
        hits, _, _, _ = rd.get_raw(keys)
        exp_run = [64 if k in (b"k07", b"k63", b"new") else r
                   for r, k in enumerate(keys[:64])] + [64, -1]
        assert hits["run"].tolist() == exp_run
        assert hits["is_tombstone"][7] == 1
        got = rd.get(keys)
        assert got[63] == b"over" and got[64] == b"value-2" and got[5] == b"v5"
        before = rd.get_raw(keys)
        # the flush is refused and keeps the memtable
        assert _code(rd.memtable_flush) == INVALID_ARG
        assert _code(rd.memtable_flush, build_bloom=True, fetch=False) == \
            INVALID_ARG
        assert rd.n_runs == 64 and rd.table_bytes == tb
        _assert_memtable(rd, model)
        _assert_raw_equal(rd.get_raw(keys), before)
        rd.memtable_clear()
        model.clear()
        _assert_memtable(rd, model)
        assert rd.get_raw(keys)[0]["run"].tolist() == list(range(64)) + [-1, -1]


def test_put_between_compact_begin_and_commit(order):
    tables, blooms = _base()
    top = batch_model.flush_run(gen(3, 80, POOL[2::7]))
    model = Memtable()
    keys = POOL[::3] + ABSENT
    with Reader(tables + [top], blooms=blooms + [None], device=0) as rd:
        rd.compact_begin([0, 1], True, fetch=False)
        _put(rd, model, gen(71, 400, POOL))
        rd.compact_commit(0)
        _put(rd, model, gen(72, 100, POOL))
        od, oi, _ = oracle.compact(tables, True)
        _assert_answers(rd, [(od, oi), top], [None, None], model, keys)


def test_tables_added_under_a_memtable(order):
    """insert_run / write_batch at the end while the memtable is not empty:
    the memtable still wins and its reported run moves up."""
    tables, blooms = _base()
    model = Memtable()
    keys = POOL[::3] + ABSENT
    extra = batch_model.flush_run(gen(81, 150, POOL))
    batch = gen(82, 200, POOL)
    with Reader(tables, blooms=blooms, device=0) as rd:
        _put(rd, model, gen(80, 500, POOL))
        rd.insert_run(2, extra)
        _assert_answers(rd, tables + [extra], blooms + [None], model, keys)
        rd.write_batch(batch, fetch=False)
        _assert_answers(rd, tables + [extra, batch_model.flush_run(batch)],
                        blooms + [None, None], model, keys)
        _assert_memtable(rd, model)


def _raw_put(rd, n, ptrs):
    return rd._lib.dbeel_gpu_reader_put(rd._h, n, *ptrs, None)


def test_host_refusals_in_order_leave_the_memtable_untouched():
    """With a live reader, on arrays that only carry offsets: a NULL array,
    2^31 writes, a descending offset, an oversized write — each refused on
    the host with the reader, its memtable and its answers as before. (The
    bound on memtable entries + n_writes shares the 2^31 refusal's code; a
    memtable of 2^31 entries is not built here.)"""
    tables, blooms = _base()
    model = Memtable()
    n, ptrs, keep = engine._write_arrays([(b"k", b"v", 1), (b"a", b"", -1)])
    u64p = ctypes.POINTER(ctypes.c_uint64)
    desc = np.array([1, 0, 0], dtype=np.uint64)
    huge = np.array([0, 1, 1 + 0xFFFFFFFF - 32], dtype=np.uint64)
    keys = POOL[::4]
    with Reader(tables, blooms=blooms, device=0) as rd:
        _put(rd, model, gen(90, 120, POOL))
        before = rd.get_raw(keys)
        info = rd.memtable_info
        err = rd._lib.dbeel_gpu_last_error
        assert _raw_put(rd, n, [None] + ptrs[1:]) == INVALID_ARG
        assert b"null array" in err()
        assert _raw_put(rd, 1 << 31, ptrs) == INVALID_ARG
        assert b"2^31" in err()
        # descending AND oversized: the descending offset is reported
        assert _raw_put(rd, n, [ptrs[0], desc.ctypes.data_as(u64p), ptrs[2],
                                huge.ctypes.data_as(u64p),
                                ptrs[4]]) == INVALID_ARG
        assert b"descend" in err()
        assert _raw_put(rd, n, [ptrs[0], ptrs[1], ptrs[2],
                                huge.ctypes.data_as(u64p),
                                ptrs[4]]) == ITEM_TOO_LARGE
        assert rd.memtable_info == info
        _assert_memtable(rd, model)
        _assert_raw_equal(rd.get_raw(keys), before)
        assert _raw_put(rd, 0, [None] * 5) == 0  # a successful no-op
        assert rd.memtable_info == info
    del keep


# ---- 7. growth ----

def test_growth():
    tables, blooms = _base()
    model = Memtable()
    pool = key_pool(11, 6000)
    reserved, grown = 0, 0
    with Reader(tables, blooms=blooms, device=0) as rd:
        tb = rd.table_bytes
        for j in range(40):
            writes = gen(200 + j, 200, pool)
            model.put(writes)
            st = rd.put(writes)
            assert st["entries"] == model.entries
            now = rd.memtable_info["reserved_bytes"]
            assert now >= reserved
            grown += now > reserved
            reserved = now
        assert grown >= 3 and rd.memtable_info["puts"] == 40
        assert grown < 40  # geometric: most puts allocate nothing
        _assert_memtable(rd, model)
        assert rd.table_bytes == tb
        _assert_answers(rd, tables, blooms, model, pool[::10] + ABSENT)


# ---- 8. file level ----

def _dir_state(d):
    return {f: open(os.path.join(d, f), "rb").read()
            for f in sorted(os.listdir(d))}


def test_lsm_reader_memtable_flush(order, tmp_path):
    d = str(tmp_path)
    tables, _ = _base()
    lsm.write_run_files(d, 0, *tables[0])
    lsm.write_run_files(d, 2, *tables[1])
    model = Memtable()
    keys = POOL[::3] + ABSENT
    rd, idx = lsm.open_reader(d, device=0)
    with rd:
        # an empty memtable writes nothing
        state = _dir_state(d)
        assert lsm.reader_memtable_flush(d, rd, idx, 4) == idx
        assert _dir_state(d) == state and rd.n_runs == 2
        _put(rd, model, gen(95, 500, POOL))
        _put(rd, model, gen(96, 100, POOL))
        before = rd.get_raw(keys)
        # a stale index (below, or equal to, one held) is refused with
        # nothing written
        for stale in (1, 2):
            assert _code(lsm.reader_memtable_flush, d, rd, idx,
                         stale) == INVALID_ARG
        assert _dir_state(d) == state and rd.n_runs == 2
        _assert_memtable(rd, model)
        _assert_raw_equal(rd.get_raw(keys), before)

        idx = lsm.reader_memtable_flush(d, rd, idx, 4)
        assert idx == [0, 2, 4]
        assert lsm.read_run_files(d, 4) == model.run()
        assert not [f for f in os.listdir(d) if f.endswith(".bloom")]
        assert len(os.listdir(d)) == 6 and rd.n_runs == 3
        assert rd.memtable_info["entries"] == 0
        _assert_raw_equal(rd.get_raw(keys), before)
        fresh, fidx = lsm.open_reader(d, device=0)
        with fresh:
            assert fidx == idx
            _assert_raw_equal(rd.get_raw(keys), fresh.get_raw(keys))
            assert rd.table_bytes == fresh.table_bytes


def test_lsm_reader_memtable_flush_io_error_changes_nothing(tmp_path):
    d = str(tmp_path)
    tables, _ = _base()
    lsm.write_run_files(d, 0, *tables[0])
    model = Memtable()
    keys = POOL[::3] + ABSENT
    rd, idx = lsm.open_reader(d, device=0)
    with rd:
        _put(rd, model, gen(97, 300, POOL))
        before = rd.get_raw(keys)
        tb = rd.table_bytes
        info = rd.memtable_info
        gone = os.path.join(d, "no-such-directory")
        assert _code(lsm.reader_memtable_flush, gone, rd, idx, 3) == IO
        assert rd.n_runs == 1 and rd.table_bytes == tb
        assert rd.memtable_info == info
        _assert_memtable(rd, model)
        _assert_raw_equal(rd.get_raw(keys), before)
        assert sorted(os.listdir(d)) == sorted(
            ["%020d.data" % 0, "%020d.index" % 0])


# ---- 9. seeded fuzz ----

@pytest.mark.parametrize("seed", range(30))
def test_fuzz(seed, monkeypatch):
    rng = np.random.default_rng(9000 + seed)
    pool = key_pool(500 + seed, 400, max_klen=24)
    tables = [batch_model.flush_run(gen(seed, 60, pool[::2]))]
    blooms = [None]
    model = Memtable()
    monkeypatch.delenv("DBEEL_BATCH_ORDER", raising=False)
    with Reader(tables, device=0) as rd:
        for step in range(10):
            op = rng.choice(["put", "put", "put", "get", "flush", "clear",
                             "insert"])
            if op == "put":
                n = int(rng.integers(1, 120))
                model.put(w := gen(seed * 100 + step, n, pool, max_vlen=48))
                assert rd.put(w)["entries"] == model.entries
            elif op == "flush":
                bloom = bool(rng.integers(0, 2))
                d, i, b = rd.memtable_flush(build_bloom=bloom)
                assert (d, i) == model.run()
                if model.entries:
                    tables.append((d, i))
                    blooms.append(b)
                model.clear()
            elif op == "clear":
                rd.memtable_clear()
                model.clear()
            elif op == "insert":
                run = batch_model.flush_run(
                    gen(seed * 100 + 50 + step, 40, pool))
                pos = int(rng.integers(0, len(tables) + 1))
                rd.insert_run(pos, run)
                tables.insert(pos, run)
                blooms.insert(pos, None)
            keys = [pool[int(j)] for j in rng.integers(0, len(pool), 64)]
            _assert_answers(rd, tables, blooms, model, keys + ABSENT[:2])
        _assert_memtable(rd, model)
        assert rd.n_runs == len(tables)
