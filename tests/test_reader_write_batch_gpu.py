"""GPU tests of the write batch (engine.Reader.write_batch,
engine.flush_batch, lsm.reader_flush): an unsorted batch of writes with
repeated keys is sorted, deduplicated and encoded on the device straight
into a resident table — the reference's memtable + flush
(rbtree_arena/src/lib.rs:497-511, lsm_tree.rs:850-915, 925-946).

Host model: tests/batch_model.py (last arrival of a key wins whatever the
timestamps, keys ascending bytewise, tombstones kept). Every byte-exact test
runs under both DBEEL_BATCH_ORDER settings: radix sort + settle, and the
single merge sort (the default when the variable is unset).
"""
import ctypes
import os

import numpy as np
import pytest

import batch_model
import oracle
from dbeel_amd import engine, lsm
from dbeel_amd.engine import DbeelGpuError, Reader
from dbeel_amd.format import Entry, build_run

pytestmark = pytest.mark.gpu

INVALID_ARG, IO = 1, 7
HIT_FIELDS = ("run", "is_tombstone", "value_offset", "value_len")
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
# what the reader holds before a batch arrives: one key no batch here writes
BASE_RUN = build_run([Entry(b"\xff" * 48, b"base", 0)])


@pytest.fixture(params=["radix", "merge"])
def order(request, monkeypatch):
    """The order stage's environment switch, read by the engine per call."""
    monkeypatch.setenv("DBEEL_BATCH_ORDER", request.param)
    return request.param


def _code(fn, *a, **kw):
    with pytest.raises(DbeelGpuError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, int(n), dtype=np.uint8))


def _gen(seed, n, n_keys, max_klen=40, max_vlen=64):
    """n writes over about n_keys keys of 0..max_klen B (the empty key
    among them), values 0..max_vlen B with ~15 % tombstones, timestamps
    negative, positive and the i128 extremes."""
    rng = np.random.default_rng(seed)
    pool = {b""} if n_keys > 2 else set()
    while len(pool) < n_keys:
        pool.add(_rand_bytes(rng, rng.integers(0, max_klen + 1)))
    pool = sorted(pool)
    special = [I128_MIN, I128_MAX, -1, 0, 1]
    writes = []
    for i in range(n):
        k = pool[int(rng.integers(0, len(pool)))]
        v = (b"" if rng.random() < 0.15
             else _rand_bytes(rng, rng.integers(0, max_vlen + 1)))
        t = (special[int(rng.integers(0, len(special)))] if i % 7 == 0
             else int(rng.integers(-10**15, 10**15)))
        writes.append((k, v, t))
    return writes


def _assert_raw_equal(got, exp):
    hits, voff, values, _ = got
    ehits, evoff, evalues, _ = exp
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], ehits[f]), f
    assert np.array_equal(voff, evoff)
    assert values.tobytes() == evalues.tobytes()


def _assert_same_as_fresh(live, runs, keys, blooms=None):
    """Answers and table_bytes of the live reader equal a reader reopened
    over the same runs and filters."""
    assert live.n_runs == len(runs)
    with Reader(runs, blooms=blooms, device=0) as fresh:
        _assert_raw_equal(live.get_raw(keys), fresh.get_raw(keys))
        assert live.table_bytes == fresh.table_bytes


def _check_batch(writes, build_bloom=False):
    """write_batch at the end of a reader holding one small run: bytes and
    stats against the model. Returns (data, index, bloom)."""
    md, mi = batch_model.flush_run(writes)
    with Reader([BASE_RUN], device=0) as rd:
        d, i, bloom, st = rd.write_batch(writes, build_bloom=build_bloom)
        assert i == mi
        assert d == md
        assert st["writes_in"] == len(writes)
        assert st["entries_out"] == len(mi) // 16
        assert st["data_bytes_out"] == len(md)
        assert st["prefix_tied"] == batch_model.prefix_tied(writes)
        assert st["d2h_bytes"] >= len(md) + len(mi)
        assert rd.n_runs == 2
        keys = sorted({w[0] for w in writes})[:512]
        _assert_same_as_fresh(rd, [BASE_RUN, (md, mi)], keys,
                              blooms=[None, bloom] if bloom else None)
    return d, i, bloom


# ---- 1. parity ----

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_parity(order, n):
    writes = _gen(1000 + n, n, max(1, (n * 3) // 10))
    d, i, _ = _check_batch(writes)
    fd, fi, fn = engine.flush_batch(writes, device=0)
    assert (fd, fi, fn) == (d, i, len(i) // 16)
    ents = batch_model.flush_entries(writes)
    ed, ei, _ = engine.encode_run(
        [(e.key, e.data, e.timestamp) for e in ents], device=0)
    assert (ed, ei) == (d, i)


def test_parity_with_the_switch_unset(monkeypatch):
    monkeypatch.delenv("DBEEL_BATCH_ORDER", raising=False)
    _check_batch(_gen(4242, 1000, 300))


# ---- 2. last arrival wins ----

def test_last_arrival_beats_timestamp(order):
    writes = [(b"key", b"first", 300), (b"key", b"second", 200),
              (b"key", b"third", 100)]
    d, i, _ = _check_batch(writes)
    assert (d, i) == build_run([Entry(b"key", b"third", 100)])


def test_one_key_4097_times(order):
    writes = [(b"the-one-key", b"v%d" % j, 5000 - j) for j in range(4097)]
    d, i, _ = _check_batch(writes)
    assert (d, i) == build_run([Entry(b"the-one-key", b"v4096", 904)])


@pytest.mark.parametrize("rev", [False, True], ids=["sorted", "reversed"])
def test_presorted_input(order, rev):
    keys = sorted({w[0] for w in _gen(5, 700, 500)}, reverse=rev)
    writes = [(k, b"val-" + k[:4], j - 300) for j, k in enumerate(keys)]
    _check_batch(writes)


# ---- 3. prefix families ----

def test_shared_prefix_batch(order):
    """5,000 writes whose keys all share their first 8 bytes, with
    duplicates: every write is prefix-tied."""
    rng = np.random.default_rng(77)
    writes = [(b"user:000" + b"%06d" % int(rng.integers(0, 3000)),
               _rand_bytes(rng, rng.integers(0, 24)), int(j))
              for j in range(5000)]
    assert batch_model.prefix_tied(writes) == 5000
    d, i, _ = _check_batch(writes)
    assert len(i) // 16 == len({w[0] for w in writes}) < 3000


def test_distinct_prefixes_tie_nothing(order):
    writes = [(int(j * 2654435761 % 2**32).to_bytes(4, "big") + b"-tail-%d" % j,
               b"v", j) for j in range(3000)]
    assert batch_model.prefix_tied(writes) == 0
    _check_batch(writes)


def test_zero_padding_and_empty_key(order):
    keys = [b"ab\0\0", b"ab", b"", b"ab\0", b"ab\0\0\0\0\0\0", b"ab\0\0\0\0\0\0\0",
            b"ab", b"", b"a"]
    writes = [(k, b"v%d" % j, -j) for j, k in enumerate(keys)]
    _check_batch(writes)


def test_keys_equal_through_byte_96(order):
    stem = bytes(range(96))
    keys = [stem + t for t in (b"", b"\0", b"\0\0", b"b", b"a", b"ab", b"\xff",
                               b"a" * 40, b"a" * 39 + b"b")]
    writes = [(k, b"x" * (j % 5), j) for j, k in enumerate(keys * 3)]
    _check_batch(writes)


def test_long_keys_and_values(order):
    """Keys and values past 512 B: wave_copy_bytes loops more than once,
    with every tail length."""
    rng = np.random.default_rng(9)
    writes = [(_rand_bytes(rng, 513 + j * 37), _rand_bytes(rng, 515 + j * 101),
               j) for j in range(12)]
    writes += [(writes[3][0], _rand_bytes(rng, 1029), 1)]
    _check_batch(writes)


def test_value_sizes_around_a_chunk(order):
    writes = [(b"key-%d" % v, b"\xab" * v, v) for v in (0, 1, 7, 8, 9)]
    writes += [(b"k" * kl, b"\xcd" * 9, kl) for kl in (1, 7, 8, 9, 15, 16, 17)]
    _check_batch(writes)


def test_one_70_kib_value(order):
    rng = np.random.default_rng(3)
    writes = _gen(11, 40, 20)
    writes.insert(17, (b"big", _rand_bytes(rng, 70 * 1024), 5))
    _check_batch(writes)


# ---- 4. read path ----

def _old_and_batch():
    """An older run holding some of the batch's keys with HIGHER
    timestamps, and the batch."""
    keys = [b"key-%04d" % j for j in range(40)]
    old = build_run([Entry(k, b"old-" + k, 10**9) for k in keys[:30]])
    writes = []
    for j, k in enumerate(keys[10:]):
        writes.append((k, b"" if j % 4 == 0 else b"new-" + k, j))
    writes.append((keys[12], b"newest", -5))  # rewritten inside the batch
    return keys, old, writes


def test_get_sees_the_batch_first(order):
    keys, old, writes = _old_and_batch()
    last = {k: v for k, v, _ in writes}
    with Reader([old], device=0) as rd:
        rd.write_batch(writes)
        hits, _, _, _ = rd.get_raw(keys)
        got = rd.get(keys)
        for q, k in enumerate(keys):
            if k in last:
                assert got[q] == last[k]
                assert hits["run"][q] == 1
                assert hits["is_tombstone"][q] == (last[k] == b"")
            else:
                assert got[q] == b"old-" + k and hits["run"][q] == 0
        _assert_same_as_fresh(rd, [old, batch_model.flush_run(writes)], keys)


def test_batch_below_the_old_run_loses(order):
    keys, old, writes = _old_and_batch()
    last = {k: v for k, v, _ in writes}
    with Reader([old], device=0) as rd:
        rd.write_batch(writes, pos=0)
        got = rd.get(keys)
        for q, k in enumerate(keys):
            assert got[q] == (b"old-" + k if q < 30 else last[k])
        _assert_same_as_fresh(rd, [batch_model.flush_run(writes), old], keys)


# ---- 5. composition ----

def test_composes_with_compaction_and_scan(order):
    keys, old, writes = _old_and_batch()
    older = build_run([Entry(k, b"older", 5) for k in keys[::3]])
    model = batch_model.flush_run(writes)
    with Reader([older, old], device=0) as rd:
        d, i, bloom, _ = rd.write_batch(writes, build_bloom=True)
        assert (d, i) == model and bloom[:4] == b"DBLM"
        # a single-run rewrite reproduces the three files
        cd, ci, cb, _ = rd.compact_begin([2], True, bloom=True)
        rd.compact_abort()
        assert (cd, ci) == (d, i)
        assert cb == bloom
        # a paged scan over the three tables
        assert rd.scan() == engine.scan([older, old, model], device=0)
        assert rd.scan(start_key=keys[5], end_key=keys[33],
                       page_bytes=512, page_entries=8) == engine.scan(
            [older, old, model], start_key=keys[5], end_key=keys[33], device=0)
        # compacting the new table with the older runs
        for keep in (True, False):
            gd, gi, _, st = rd.compact_begin([0, 1, 2], keep)
            rd.compact_abort()
            od, oi, on = oracle.compact([older, old, model], keep)
            assert (gd, gi, st["entries_out"]) == (od, oi, on)
        _assert_same_as_fresh(rd, [older, old, model], keys,
                              blooms=[None, None, bloom])


# ---- 6. liveness and atomicity ----

def test_open_scan_goes_stale_only_on_a_real_batch(order):
    keys, old, writes = _old_and_batch()
    data = np.empty(1 << 16, dtype=np.uint8)
    index = np.empty(16 * 64, dtype=np.uint8)
    with Reader([old], device=0) as rd:
        tb = rd.table_bytes
        sc = rd.scan_open()
        d, i, b, st = rd.write_batch([])
        assert (d, i, b) == (b"", b"", None)
        assert st["writes_in"] == 0 and st["entries_out"] == 0
        assert rd.n_runs == 1 and rd.table_bytes == tb
        sc.next(data, index)  # still valid
        rd.write_batch(writes)
        assert _code(sc.next, data, index) == INVALID_ARG
        sc.close()


def test_write_batch_under_a_pending_compaction(order):
    keys, old, writes = _old_and_batch()
    older = build_run([Entry(k, b"older", 5) for k in keys[::3]])
    top = build_run([Entry(k, b"top", 7) for k in keys[1::5]])
    with Reader([older, old, top], device=0) as rd:
        rd.compact_begin([0, 1], True, fetch=False)
        rd.write_batch(writes, pos=0, fetch=False)
        assert rd.n_runs == 4
        rd.compact_commit(1)
        od, oi, _ = oracle.compact([older, old], True)
        _assert_same_as_fresh(
            rd, [batch_model.flush_run(writes), (od, oi), top], keys)


def _raw_write_batch(rd, n, ptrs):
    return rd._lib.dbeel_gpu_reader_write_batch(
        rd._h, rd.n_runs, n, *ptrs, 0, None, None, None, None)


def test_failures_leave_the_reader_untouched():
    keys, old, writes = _old_and_batch()
    n, ptrs, keep = engine._write_arrays(writes)
    koff = keep[2].copy()
    koff[5] = koff[6] + 1  # descends
    bad = list(ptrs)
    bad[1] = koff.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    with Reader([old], device=0) as rd:
        before = rd.get_raw(keys)
        tb = rd.table_bytes
        assert _raw_write_batch(rd, n, bad) == INVALID_ARG
        assert _code(rd.write_batch, writes, pos=2) == INVALID_ARG
        assert rd.n_runs == 1 and rd.table_bytes == tb
        _assert_raw_equal(rd.get_raw(keys), before)
        rd.write_batch(writes)  # and the reader still takes a good batch
        assert rd.n_runs == 2

    tiny = [build_run([Entry(b"k%02d" % r, b"v", r)]) for r in range(64)]
    with Reader(tiny, device=0) as rd:
        q = [b"k%02d" % r for r in range(64)] + [w[0] for w in writes]
        before = rd.get_raw(q)
        tb = rd.table_bytes
        assert _code(rd.write_batch, writes) == INVALID_ARG
        rd.write_batch([])  # an empty batch is still a no-op, not an error
        assert rd.n_runs == 64 and rd.table_bytes == tb
        _assert_raw_equal(rd.get_raw(q), before)
    del keep


def test_table_bytes_match_a_reopened_reader(order):
    writes = _gen(21, 900, 250)
    _check_batch(writes, build_bloom=True)  # asserts table_bytes, filter kept
    with Reader([BASE_RUN], device=0) as rd:
        # fetch=False leaves the bytes on the device; the table is the same
        d, i, b, st = rd.write_batch(writes, build_bloom=True, fetch=False)
        assert (d, i, b) == (None, None, None) and st["d2h_bytes"] == 0
        md, mi = batch_model.flush_run(writes)
        cd, ci, cb, _ = rd.compact_begin([1], True, bloom=True)
        rd.compact_abort()
        assert (cd, ci) == (md, mi)
        _assert_same_as_fresh(rd, [BASE_RUN, (md, mi)],
                              sorted({w[0] for w in writes}),
                              blooms=[None, cb])


# ---- 7. file level ----

def _dir_state(d):
    return {f: open(os.path.join(d, f), "rb").read()
            for f in sorted(os.listdir(d))}


def test_lsm_reader_flush(order, tmp_path):
    d = str(tmp_path)
    keys, old, writes = _old_and_batch()
    older = build_run([Entry(k, b"older", 5) for k in keys[::3]])
    lsm.write_run_files(d, 0, *older)
    lsm.write_run_files(d, 2, *old)
    rd, idx = lsm.open_reader(d, device=0)
    with rd:
        idx = lsm.reader_flush(d, rd, idx, 4, writes)
        assert idx == [0, 2, 4]
        assert lsm.read_run_files(d, 4) == batch_model.flush_run(writes)
        mid = [(k, b"mid", 1) for k in reversed(keys[:8])]
        idx = lsm.reader_flush(d, rd, idx, 1, mid)
        assert idx == [0, 1, 2, 4]
        assert lsm.read_run_files(d, 1) == batch_model.flush_run(mid)
        assert not [f for f in os.listdir(d) if f.endswith(".bloom")]
        assert len(os.listdir(d)) == 8
        # an empty memtable flushes nothing
        assert lsm.reader_flush(d, rd, idx, 6, []) == idx
        assert len(os.listdir(d)) == 8 and rd.n_runs == 4

        fresh, fidx = lsm.open_reader(d, device=0)
        with fresh:
            assert fidx == idx
            _assert_raw_equal(rd.get_raw(keys), fresh.get_raw(keys))
            assert rd.table_bytes == fresh.table_bytes

        # a duplicate index is refused with the directory untouched
        state = _dir_state(d)
        before = rd.get_raw(keys)
        assert _code(lsm.reader_flush, d, rd, idx, 2, writes) == INVALID_ARG
        assert _dir_state(d) == state and rd.n_runs == 4
        _assert_raw_equal(rd.get_raw(keys), before)


def test_lsm_reader_flush_io_error_removes_the_table(tmp_path):
    d = str(tmp_path)
    keys, old, writes = _old_and_batch()
    lsm.write_run_files(d, 0, *old)
    rd, idx = lsm.open_reader(d, device=0)
    with rd:
        before = rd.get_raw(keys)
        tb = rd.table_bytes
        gone = os.path.join(d, "no-such-directory")
        assert _code(lsm.reader_flush, gone, rd, idx, 3, writes) == IO
        assert rd.n_runs == 1 and rd.table_bytes == tb
        _assert_raw_equal(rd.get_raw(keys), before)
        assert sorted(os.listdir(d)) == sorted(
            ["%020d.data" % 0, "%020d.index" % 0])
