"""GPU tests of the live resident reader (engine.Reader.insert_run /
compact_begin / compact_commit / compact_abort, lsm.reader_add /
lsm.reader_compact): the shared sstable list of the reference's LSMTree
(flush lsm_tree.rs:901-915, compaction swap lsm_tree.rs:1113-1145).

Host model: the run list itself. Reads follow test_reader_gpu's model (the
HIGHEST position wins, regardless of timestamp); a compaction replaces the
chosen runs by the CPU oracle's output for them. The central assertion:
after any sequence of updates, get_raw on the live reader equals get_raw on
a fresh Reader over the resulting run list, field for field and in value
bytes and offsets.
"""
import os
import shutil

import numpy as np
import pytest

import oracle
from conftest import GOLDEN_CASES, load_golden
from dbeel_amd import lsm
from dbeel_amd.engine import DbeelGpuError, Job, Reader
from dbeel_amd.format import Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs

pytestmark = pytest.mark.gpu

INVALID_ARG, CORRUPT = 1, 2
HIT_FIELDS = ("run", "is_tombstone", "value_offset", "value_len")


def _code(fn, *a, **kw):
    with pytest.raises(DbeelGpuError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _model(runs):
    model = {}
    for r, (d, i) in enumerate(runs):
        for e in parse_run(bytes(d), bytes(i)):
            model[e.key] = (r, e.data)
    return model


def _keys_of(runs):
    return sorted({e.key for d, i in runs
                   for e in parse_run(bytes(d), bytes(i))})


def _absent(n, seed=99, klen=16):
    rng = np.random.default_rng(seed)
    return [b"\xfe" + bytes(rng.integers(0, 256, klen - 1, dtype=np.uint8))
            for _ in range(n)]


def _assert_raw_equal(got, exp):
    hits, voff, values, _ = got
    ehits, evoff, evalues, _ = exp
    for f in HIT_FIELDS:
        assert np.array_equal(hits[f], ehits[f]), f
    assert np.array_equal(voff, evoff)
    assert values.tobytes() == evalues.tobytes()


def _assert_same_as_fresh(live, runs, keys, blooms=None):
    """The central assertion."""
    assert live.n_runs == len(runs)
    with Reader(runs, blooms=blooms, device=0) as fresh:
        _assert_raw_equal(live.get_raw(keys), fresh.get_raw(keys))
        return fresh.table_bytes


def _apply_compact(runs, positions, out_pos, keep):
    """The list edit of compact_commit, with the oracle's output."""
    od, oi, n = oracle.compact([runs[p] for p in positions], keep)
    left = [r for p, r in enumerate(runs) if p not in set(positions)]
    left.insert(out_pos, (od, oi))
    return left, (od, oi, n)


def _mk_run(rng, pool, n, max_val=64, ts_lo=1, ts_hi=10**6):
    """n entries with keys drawn from pool, 0..max_val-B values (0 =
    tombstone), random timestamps."""
    pick = rng.choice(len(pool), size=n, replace=False)
    ents = [Entry(pool[int(j)],
                  bytes(rng.integers(0, 256, int(rng.integers(0, max_val + 1)),
                                     dtype=np.uint8)),
                  int(rng.integers(ts_lo, ts_hi)))
            for j in pick]
    return build_run(sorted(ents, key=lambda e: e.key))


class _Base:
    """Three ~200-entry runs (16-B keys, 0-64-B values) over a shared key
    pool, a fourth to insert, and the query set — built once, read-only."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.pool = [bytes(rng.integers(0, 256, 16, dtype=np.uint8))
                     for _ in range(600)]
        assert len(set(self.pool)) == 600
        self.runs = [_mk_run(rng, self.pool, 200) for _ in range(3)]
        self.extra = _mk_run(rng, self.pool, 200)
        self.queries = self.pool + _absent(50)
        self.rng_seed = 7


@pytest.fixture(scope="module")
def base():
    return _Base()


# ---- 1. insert ----

@pytest.mark.parametrize("pos", [0, 2, 3], ids=["front", "middle", "end"])
def test_insert(base, pos):
    with Reader(base.runs, device=0) as rd:
        rd.insert_run(pos, base.extra)
        runs = list(base.runs)
        runs.insert(pos, base.extra)
        _assert_same_as_fresh(rd, runs, base.queries)
        model = _model(runs)
        exp = [model[k][1] if k in model else None for k in base.queries]
        assert rd.get(base.queries) == exp


def test_insert_position_beats_timestamp():
    low = build_run([Entry(b"k" * 16, b"low-position-new-ts", 5000)])
    high = build_run([Entry(b"k" * 16, b"high-position-old-ts", 10)])
    other = build_run([Entry(b"z" * 16, b"zz", 1)])
    with Reader([low, other], device=0) as rd:
        rd.insert_run(2, high)
        assert rd.get([b"k" * 16]) == [b"high-position-old-ts"]
        _assert_same_as_fresh(rd, [low, other, high], [b"k" * 16, b"z" * 16])
    with Reader([low, other], device=0) as rd:
        # the same run inserted BELOW: the run above it keeps winning
        rd.insert_run(0, high)
        assert rd.get([b"k" * 16]) == [b"low-position-new-ts"]
        _assert_same_as_fresh(rd, [high, low, other], [b"k" * 16])


def test_insert_empty_run(base):
    with Reader(base.runs, device=0) as rd:
        rd.insert_run(1, (b"", b""))
        runs = list(base.runs)
        runs.insert(1, (b"", b""))
        _assert_same_as_fresh(rd, runs, base.queries)


def test_insert_with_filter(base):
    with Job([base.extra], device=0) as job:
        job.run(True)
        bloom = job.bloom()
    with Reader(base.runs, device=0) as rd:
        _, _, _, st = rd.get_raw(base.queries)
        assert st["bloom_probes"] == 0
        rd.insert_run(3, base.extra, bloom=bloom)
        runs = base.runs + [base.extra]
        _assert_same_as_fresh(rd, runs, base.queries,
                              blooms=[None, None, None, bloom])
        _, _, _, st = rd.get_raw(base.queries)
        assert st["bloom_probes"] > 0


# ---- 2. insert failure is atomic ----

def _bad_inputs(base):
    d, i = base.extra
    ents = parse_run(d, i)
    ents[10], ents[11] = ents[11], ents[10]
    good_bloom_hdr = b"XBLM" + bytes(28 + 64)
    return {
        "truncated_index": ((d, i[:-8]), None),
        "swapped_keys": (build_run(ents), None),
        "bad_filter_magic": ((d, i), good_bloom_hdr),
    }


@pytest.mark.parametrize("case", ["truncated_index", "swapped_keys",
                                  "bad_filter_magic"])
def test_insert_failure_is_atomic(base, case):
    run, bloom = _bad_inputs(base)[case]
    with Reader(base.runs, device=0) as rd:
        before = rd.get_raw(base.queries)
        tb = rd.table_bytes
        assert _code(rd.insert_run, 1, run, bloom=bloom) == CORRUPT
        assert rd.n_runs == 3 and rd.table_bytes == tb
        _assert_raw_equal(rd.get_raw(base.queries), before)
        assert _code(rd.insert_run, 4, base.extra) == INVALID_ARG  # pos
        assert rd.n_runs == 3 and rd.table_bytes == tb
        # and the reader still takes a good run
        rd.insert_run(1, base.extra)
        assert rd.n_runs == 4


# ---- 8. 64 -> 1 (and the 65th insert) ----

def test_64_runs_full_then_compact_to_one():
    key = b"the-same-key-16B"
    runs = [build_run([Entry(key, b"v%02d" % r, 1000 - 7 * (r % 5))])
            for r in range(64)]
    with Reader(runs, device=0) as rd:
        tb = rd.table_bytes
        assert _code(rd.insert_run, 0, runs[0]) == INVALID_ARG  # 65th
        assert rd.n_runs == 64 and rd.table_bytes == tb
        assert rd.get([key]) == [b"v63"]
        data, index, _, st = rd.compact(range(64), 0, True)
        od, oi, n = oracle.compact(runs, True)
        assert (data, index) == (od, oi) and n == 1
        assert st["entries_in"] == 64 and st["entries_out"] == 1
        assert rd.n_runs == 1
        _assert_same_as_fresh(rd, [(od, oi)], [key, b"other"])
        rd.insert_run(1, runs[5])
        assert rd.n_runs == 2 and rd.get([key]) == [b"v05"]


# ---- 3. compaction parity over every golden fixture ----

@pytest.fixture(scope="module")
def goldens():
    return {name: load_golden(name) for name in GOLDEN_CASES}


@pytest.mark.parametrize("keep", [0, 1], ids=["drop", "keep"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_compact_golden(goldens, name, keep):
    runs, keep_out, drop_out = goldens[name]
    exp = keep_out if keep else drop_out
    queries = _keys_of(runs) + _absent(20)
    with Reader(runs, device=0) as rd:
        data, index, bloom, st = rd.compact(range(len(runs)), 0, bool(keep))
        assert data == exp[0]
        assert index == exp[1]
        assert bloom is None
        assert st["entries_out"] == len(exp[1]) // 16
        _assert_same_as_fresh(rd, [exp], queries)


# ---- 4. non-contiguous group and placement ----

def _placement_runs():
    k_shared, k_pair = b"shared-key-00016", b"pair-key-0000016"
    rng = np.random.default_rng(41)
    pool = [bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            for _ in range(120)]
    runs = []
    # timestamps opposite to positions: position 0 holds the newest
    for r in range(4):
        ents = parse_run(*_mk_run(rng, pool, 60))
        ents.append(Entry(k_shared, b"shared@%d" % r, 4000 - 1000 * r))
        if r in (0, 2):
            ents.append(Entry(k_pair, b"pair@%d" % r, 4000 - 1000 * r))
        runs.append(build_run(sorted(ents, key=lambda e: e.key)))
    return runs, pool + [k_shared, k_pair] + _absent(10)


@pytest.mark.parametrize("out_pos", [0, 1, 2])
def test_noncontiguous_group_and_placement(out_pos):
    runs, queries = _placement_runs()
    with Reader(runs, device=0) as rd:
        data, index, _, _ = rd.compact([0, 2], out_pos, True)
        new_runs, (od, oi, _) = _apply_compact(runs, [0, 2], out_pos, True)
        assert (data, index) == (od, oi)
        _assert_same_as_fresh(rd, new_runs, queries)
        # the compacted run carries position 0's (newest) value; whether a
        # read sees it depends on where the run was placed
        model = _model(new_runs)
        assert rd.get([b"shared-key-00016", b"pair-key-0000016"]) == [
            model[b"shared-key-00016"][1], b"pair@0"]
        expect_shared = {0: b"shared@3", 1: b"shared@3", 2: b"shared@0"}
        assert model[b"shared-key-00016"][1] == expect_shared[out_pos]


# ---- 5. adopt-kernel edges ----

def test_adopt_key_lengths_sharing_a_prefix():
    stem = b"PREFIX-8"
    keys = [b"", stem[:1], stem[:7], stem, stem + b"\0", stem + b"9",
            stem + b"x" * 32]
    assert sorted(len(k) for k in keys) == [0, 1, 7, 8, 9, 9, 40]
    a = build_run(sorted((Entry(k, b"a:" + k, 10) for k in keys),
                         key=lambda e: e.key))
    b = build_run(sorted((Entry(k, b"b:" + k, 20) for k in keys[::2]),
                         key=lambda e: e.key))
    queries = keys + [stem + b"\0\0", stem[:6], stem + b"x" * 31, b"\0"]
    with Reader([a, b], device=0) as rd:
        data, index, bloom, _ = rd.compact([0, 1], 0, True, bloom=True)
        new_runs, (od, oi, n) = _apply_compact([a, b], [0, 1], 0, True)
        assert (data, index) == (od, oi) and n == len(keys)
        with Job([a, b], device=0) as job:
            job.run(True)
            assert bloom == job.bloom()
        _assert_same_as_fresh(rd, new_runs, queries, blooms=[bloom])
        assert rd.get(keys) == [(b"b:" if k in keys[::2] else b"a:") + k
                                for k in keys]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_adopt_survivor_counts_and_filter(n):
    rng = np.random.default_rng(1000 + n)
    pool = [bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            for _ in range(n)]
    a = _mk_run(rng, pool, n, ts_lo=1, ts_hi=100)
    b = _mk_run(rng, pool, (n + 1) // 2, ts_lo=200, ts_hi=300)
    n_bits = int(9.585 * n) + 64
    absent = _absent(200, seed=n)
    with Reader([a, b], device=0) as rd:
        data, index, bloom, st = rd.compact([0, 1], 0, True, bloom=True)
        od, oi, on = oracle.compact([a, b], True)
        assert (data, index) == (od, oi) and on == n
        assert st["entries_out"] == n
        with Job([a, b], device=0) as job:
            job.run(True)
            assert bloom == job.bloom()
        assert len(bloom) == 32 + (n_bits + 7) // 8
        for k in pool:
            assert lsm.bloom_contains(bloom, k)
        _assert_same_as_fresh(rd, [(od, oi)], pool + absent, blooms=[bloom])
        _, _, _, gst = rd.get_raw(absent)
        assert gst["bloom_probes"] == 200 and gst["bloom_skips"] > 0


# ---- 6. empty output ----

def test_empty_output_stays_as_empty_run(goldens):
    runs, _, drop_out = goldens["all_tombstones"]
    assert drop_out == (b"", b"")
    keys = _keys_of(runs)
    other = build_run([Entry(b"live-key", b"live", 1)])
    with Reader(runs + [other], device=0) as rd:
        data, index, bloom, st = rd.compact(range(len(runs)), 1, False,
                                            bloom=True)
        assert (data, index) == (b"", b"")
        assert st["entries_out"] == 0 and st["data_bytes_out"] == 0
        assert rd.n_runs == 2
        assert rd.get(keys) == [None] * len(keys)
        assert rd.get([b"live-key"]) == [b"live"]
        hits, _, _, _ = rd.get_raw([b"live-key"])
        assert hits["run"][0] == 0  # the empty run sits at position 1
        _assert_same_as_fresh(rd, [other, (b"", b"")], keys + [b"live-key"],
                              blooms=[None, bloom])


# ---- 7. begin / commit / abort protocol ----

def test_begin_commit_abort_protocol(base):
    runs = base.runs + [base.extra]
    n = len(runs)
    with Reader(runs, device=0) as rd:
        before = rd.get_raw(base.queries)
        tb = rd.table_bytes
        for bad in ([2, 1], [1, 1], [], [n]):
            assert _code(rd.compact_begin, bad, True) == INVALID_ARG, bad
        assert _code(rd.compact_commit, 0) == INVALID_ARG  # nothing pending

        rd.compact_begin([1, 2], True)
        assert rd.n_runs == n
        _assert_raw_equal(rd.get_raw(base.queries), before)  # old list
        assert _code(rd.compact_begin, [0], True) == INVALID_ARG  # second
        rd.compact_abort()
        assert rd.table_bytes == tb and rd.n_runs == n
        _assert_raw_equal(rd.get_raw(base.queries), before)
        assert _code(rd.compact_commit, 0) == INVALID_ARG

        rd.compact_begin([1, 2], True)
        _assert_raw_equal(rd.get_raw(base.queries), before)
        assert _code(rd.compact_commit, n - 2 + 1) == INVALID_ARG
        rd.compact_commit(n - 2)  # the pending table survived
        new_runs, _ = _apply_compact(runs, [1, 2], n - 2, True)
        fresh_tb = _assert_same_as_fresh(rd, new_runs, base.queries)
        assert rd.table_bytes == fresh_tb


# ---- 9. stats ----

def test_stats(base):
    runs = base.runs
    od, oi, on = oracle.compact(runs[:2], False)
    with Reader(runs, device=0) as rd:
        _, _, _, st = rd.compact_begin([0, 1], False)
        assert st["pipeline"]["h2d_ms"] == 0
        assert st["entries_in"] == sum(len(i) // 16 for _, i in runs[:2])
        assert st["entries_out"] == on
        assert st["data_bytes_out"] == len(od)
        assert st["d2h_bytes"] == len(od) + len(oi)
        assert st["adopt_ms"] > 0
        rd.compact_abort()
        data, index, bloom, st = rd.compact_begin([0, 1], False, bloom=True,
                                                  fetch=False)
        assert data is None and index is None and bloom is None
        assert st["d2h_bytes"] == 0 and st["d2h_ms"] == 0
        assert st["entries_out"] == on
        rd.compact_commit(0)
        _assert_same_as_fresh(rd, [(od, oi), runs[2]], base.queries)


# ---- 10. directory flow ----

def _dir_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read()
            for n in sorted(os.listdir(d))}


def _assert_live_matches_dir(rd, indices, d, queries):
    fresh, fidx = lsm.open_reader(d, device=0)
    with fresh:
        assert indices == fidx
        assert rd.n_runs == fresh.n_runs
        _assert_raw_equal(rd.get_raw(queries), fresh.get_raw(queries))
        assert rd.table_bytes == fresh.table_bytes


@pytest.fixture(scope="module")
def dir_runs():
    runs = make_runs(4, 2000, 16, 48, overlap_frac=0.5, tombstone_frac=0.2,
                     seed=91)
    runs = [(bytes(d), bytes(i)) for d, i in runs]
    rng = np.random.default_rng(5)
    keys = _keys_of(runs)
    queries = [keys[int(j)] for j in rng.integers(0, len(keys), 800)]
    return runs, queries + _absent(100)


def test_directory_flow(tmp_path, dir_runs):
    runs, queries = dir_runs
    d, ref = str(tmp_path / "live"), str(tmp_path / "ref")
    for idx, (data, index) in zip((0, 2, 4), runs):
        lsm.write_run_files(d, idx, data, index)
    shutil.copytree(d, ref)

    rd, indices = lsm.open_reader(d, device=0)
    with rd:
        assert indices == [0, 2, 4]
        indices = lsm.reader_compact(d, rd, indices, [0, 2], 1, True,
                                     bloom_min_size=1)
        assert indices == [1, 4]
        lsm.compact(ref, [0, 2], 1, keep_tombstones=True, device=0,
                    bloom_min_size=1)
        assert os.path.exists(f"{d}/{1:020d}.bloom")
        assert _dir_bytes(d) == _dir_bytes(ref)
        _assert_live_matches_dir(rd, indices, d, queries)

        for dd in (d, ref):
            lsm.write_run_files(dd, 6, *runs[3])
        indices = lsm.reader_add(d, rd, indices, 6)
        assert indices == [1, 4, 6]
        _assert_live_matches_dir(rd, indices, d, queries)
        assert _code(lsm.reader_add, d, rd, indices, 6) == INVALID_ARG
        assert _code(lsm.reader_compact, d, rd, indices, [1, 5], 3,
                     True) == INVALID_ARG
        assert _code(lsm.reader_compact, d, rd, indices, [1, 4], 6,
                     True) == INVALID_ARG
        _assert_live_matches_dir(rd, indices, d, queries)

        indices = lsm.reader_compact(d, rd, indices, [1, 4, 6], 3, False)
        assert indices == [3]
        lsm.compact(ref, [1, 4, 6], 3, keep_tombstones=False, device=0)
        assert _dir_bytes(d) == _dir_bytes(ref)
        _assert_live_matches_dir(rd, indices, d, queries)
        # tombstones were dropped: the model is the oracle's output
        od, oi, _ = oracle.compact(
            [oracle.compact(runs[:2], True)[:2], runs[2], runs[3]], False)
        assert lsm.read_run_files(d, 3) == (od, oi)


def test_directory_crash_after_journal(tmp_path, dir_runs, monkeypatch):
    runs, queries = dir_runs
    d = str(tmp_path)
    for idx, (data, index) in zip((0, 2, 4), runs):
        lsm.write_run_files(d, idx, data, index)
    rd, indices = lsm.open_reader(d, device=0)
    with rd:
        before = rd.get_raw(queries)
        tb = rd.table_bytes
        monkeypatch.setenv("DBEEL_LSM_CRASH_AFTER_JOURNAL", "1")
        after = lsm.reader_compact(d, rd, indices, [0, 2], 1, True,
                                   bloom_min_size=1)
        monkeypatch.delenv("DBEEL_LSM_CRASH_AFTER_JOURNAL")
        assert after == indices == [0, 2, 4]
        assert os.path.exists(f"{d}/{1:020d}.compact_action")
        assert rd.n_runs == 3 and rd.table_bytes == tb
        _assert_raw_equal(rd.get_raw(queries), before)
    assert lsm.replay(d) == 1
    new_runs, _ = _apply_compact(runs[:3], [0, 1], 0, True)
    fresh, fidx = lsm.open_reader(d, device=0)
    with fresh:
        assert fidx == [1, 4]
        model = _model(new_runs)
        exp = [model[k][1] if k in model else None for k in queries]
        assert fresh.get(queries) == exp


# ---- 11. short soak ----

def test_short_soak(base):
    rng = np.random.default_rng(base.rng_seed)
    runs = list(base.runs)
    with Reader(runs, device=0) as rd:
        for cycle in range(30):
            n = len(runs)
            if n < 2 or (n < 10 and rng.random() < 0.55):
                run = _mk_run(rng, base.pool, 200)
                pos = int(rng.integers(0, n + 1))
                rd.insert_run(pos, run)
                runs.insert(pos, run)
            else:
                k = int(rng.integers(1, n + 1))
                positions = sorted(int(p) for p in
                                   rng.choice(n, size=k, replace=False))
                out_pos = int(rng.integers(0, n - k + 1))
                keep = bool(rng.integers(0, 2))
                data, index, _, _ = rd.compact(positions, out_pos, keep)
                runs, (od, oi, _) = _apply_compact(runs, positions, out_pos,
                                                   keep)
                assert (data, index) == (od, oi), cycle
            model = _model(runs)
            keys = [base.queries[int(j)]
                    for j in rng.integers(0, len(base.queries), 300)]
            exp = [model[k][1] if k in model else None for k in keys]
            assert rd.get(keys) == exp, cycle
        fresh_tb = _assert_same_as_fresh(rd, runs, base.queries)
        assert rd.table_bytes == fresh_tb
