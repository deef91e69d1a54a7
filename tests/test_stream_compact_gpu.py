"""GPU tests of compaction into caller buffers (dbeel_gpu_compact_into,
dbeel_gpu_job_fetch_into, dbeel_lsm_compact_stream): the bytes equal the
oracle's and dbeel_gpu_compact's at every slice count, nothing outside the
caller's arrays is touched, the filter built across slices equals the whole
job's, and the file layer leaves the directory as dbeel_lsm_compact does.

Every input here is well-formed: what the device does with a corrupt run is
dbeel_gpu_job_run's own, unchanged, and covered where it always was."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN_CASES, load_golden
from dbeel_amd import lsm
from dbeel_amd.format import Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs

pytestmark = pytest.mark.gpu

GUARD = 0x5A
PAD = 4096
ITEM_TOO_LARGE = 3


@pytest.fixture(scope="module")
def engine():
    import dbeel_amd

    return dbeel_amd


class Guarded:
    """A caller buffer of exactly `cap` bytes with a guard region either
    side; .arr is what the engine is given."""

    def __init__(self, cap):
        self.cap = cap
        self.whole = np.full(cap + 2 * PAD, GUARD, dtype=np.uint8)
        self.arr = self.whole[PAD:PAD + cap]

    def guards_intact(self):
        return bool((self.whole[:PAD] == GUARD).all()
                    and (self.whole[PAD + self.cap:] == GUARD).all())

    def untouched(self):
        return bool((self.whole == GUARD).all())


def _into(engine, runs, keep, n_slices=0, data_cap=None, index_cap=None,
          **kw):
    """compact_into with caps at the inputs' sums unless given; returns
    (data bytes, index bytes, n, stats, bloom) and checks the guards."""
    if data_cap is None:
        data_cap = sum(len(d) for d, _ in runs)
    if index_cap is None:
        index_cap = sum(len(i) for _, i in runs)
    gd, gi = Guarded(data_cap), Guarded(index_cap)
    dl, il, n, st, bloom = engine.compact_into(
        runs, keep, gd.arr, gi.arr, device=0, n_slices=n_slices, **kw)
    assert gd.guards_intact() and gi.guards_intact()
    assert il == n * 16
    assert st["bytes_out"] == dl + il
    return gd.arr[:dl].tobytes(), gi.arr[:il].tobytes(), n, st, bloom


@pytest.fixture(scope="module")
def base_runs():
    # the 40,000-entry sliced parity test's shape at a tenth
    return make_runs(6, 4_000, 16, 128, overlap_frac=0.6, tombstone_frac=0.1,
                     seed=99)


@pytest.fixture(scope="module")
def base_expected(engine, base_runs):
    """keep -> (oracle result, dbeel_gpu_compact result), computed once."""
    out = {}
    for keep in (True, False):
        o = oracle.compact(base_runs, keep_tombstones=keep)
        g = engine.compact(base_runs, keep_tombstones=keep, device=0)
        assert tuple(g) == tuple(o)
        out[keep] = tuple(bytes(x) if not isinstance(x, int) else x
                          for x in o)
    return out


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "drop"])
@pytest.mark.parametrize("n_slices", [1, 2, 7])
def test_parity_forced_slices(engine, base_runs, base_expected, n_slices,
                              keep):
    od, oi, on = base_expected[keep]
    gd, gi, gn, st, bloom = _into(engine, base_runs, keep, n_slices=n_slices)
    assert gn == on
    assert gi == oi
    assert gd == od
    assert bloom is None
    assert st["slices"] == n_slices
    assert st["bytes_in"] == sum(len(d) + len(i) for d, i in base_runs)


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "drop"])
def test_parity_budget_slices(engine, base_runs, base_expected, keep):
    total = sum(len(d) + len(i) for d, i in base_runs)
    od, oi, on = base_expected[keep]
    gd, gi, gn, st, _ = _into(engine, base_runs, keep,
                              max_resident_bytes=total // 7)
    assert (gn, gi, gd) == (on, oi, od)
    assert st["slices"] in (7, 8)  # ceil(total / (total // 7))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_fixtures_sliced(engine, name):
    """Every golden fixture at 1 and 3 slices: empty views inside slices
    (empty_run, single_run), slices with no survivors and an empty output
    (all_tombstones, dropped)."""
    runs, exp_keep, exp_drop = load_golden(name)
    for keep, exp in ((True, exp_keep), (False, exp_drop)):
        for n_slices in (1, 3):
            gd, gi, gn, st, _ = _into(engine, runs, keep, n_slices=n_slices)
            assert gi == exp[1], (keep, n_slices)
            assert gd == exp[0], (keep, n_slices)
            assert gn == len(exp[1]) // 16
            assert st["slices"] <= n_slices


def _adversarial():
    from adversarial import all_cases

    want = ("window_straddle", "all64_ts_asc", "all64_ts_equal")
    return [c for c in all_cases() if c[0] in want]


@pytest.mark.parametrize("case", _adversarial(), ids=lambda c: c[0])
def test_equal_key_groups_do_not_split(engine, case):
    """64 runs holding the same keys, and duplicates straddling a co-rank
    window, sliced: a pivot never separates two versions of a key."""
    name, runs = case
    for keep in (True, False):
        od, oi, on = oracle.compact(runs, keep_tombstones=keep)
        for n_slices in (2, 5):
            gd, gi, gn, st, _ = _into(engine, runs, keep, n_slices=n_slices)
            assert (gn, gi, gd) == (on, oi, od), (name, keep, n_slices)
            assert st["slices"] == n_slices  # it was sliced


def test_varkey_sliced(engine):
    """cfg5-style ragged msgpack keys: host pivots and bisection follow
    raw-byte key order."""
    from dbeel_amd.genruns import make_runs_varkey

    runs = make_runs_varkey(6, 1_500, value_size=256, overlap_frac=0.4,
                            tombstone_frac=0.1, seed=0xBEEF)
    total = sum(len(d) + len(i) for d, i in runs)
    od, oi, on = oracle.compact(runs, keep_tombstones=False)
    gd, gi, gn, st, _ = _into(engine, runs, False,
                              max_resident_bytes=total // 5)
    assert (gn, gi, gd) == (on, oi, od)
    assert st["slices"] >= 5


def test_large_value_between_pivots(engine):
    """One 200,000-byte value between 40-byte entries, a pivot either side
    of it: the slice holding it is 200 KB of one entry, its neighbours a
    few KB."""
    rng = np.random.default_rng(7)
    ents = []
    for i in range(300):
        val = (bytes(rng.integers(0, 256, 200_000, dtype=np.uint8))
               if i == 150 else b"v%d" % (i % 10))
        ents.append(Entry(b"k%05d" % i, val, i))
    big = build_run(ents)
    assert len(big[0]) == 299 * 40 + 32 + 6 + 200_000
    other = build_run([Entry(b"k%05d" % i, b"w%d" % (i % 10), 1000 + i)
                       for i in range(0, 300, 3)])
    runs = [big, other]
    od, oi, on = oracle.compact(runs, keep_tombstones=True)
    # pivots at entries 100 and 200 of the largest run
    gd, gi, gn, st, _ = _into(engine, runs, True, n_slices=3)
    assert (gn, gi, gd) == (on, oi, od)
    assert st["slices"] == 3


@pytest.mark.parametrize("n_slices", [1, 3])
def test_exact_and_short_caps(engine, base_runs, base_expected, n_slices):
    od, oi, on = base_expected[False]
    # exact caps succeed, guards intact (checked in _into)
    gd, gi, gn, _, _ = _into(engine, base_runs, False, n_slices=n_slices,
                             data_cap=len(od), index_cap=len(oi))
    assert (gn, gi, gd) == (on, oi, od)
    # one byte / one record short: refused with the exact needs
    for dcap, icap in ((len(od) - 1, len(oi)), (len(od), len(oi) - 16)):
        d, i = Guarded(dcap), Guarded(icap)
        with pytest.raises(engine.DbeelGpuError) as ei:
            engine.compact_into(base_runs, False, d.arr, i.arr, device=0,
                                n_slices=n_slices, bloom=True)
        assert ei.value.code == ITEM_TOO_LARGE
        assert ei.value.needed == (len(od), len(oi))
        assert ei.value.stats["slices"] == n_slices  # every slice still ran
        assert d.guards_intact() and i.guards_intact()


def test_pinned_and_pageable_destinations_agree(engine, base_runs,
                                                base_expected):
    od, oi, on = base_expected[True]
    out = {}
    for pinned in (False, True):
        d, i = Guarded(len(od)), Guarded(len(oi))
        if pinned:
            engine.pin_host(d.arr)
            engine.pin_host(i.arr)
        try:
            dl, il, n, _, _ = engine.compact_into(
                base_runs, True, d.arr, i.arr, device=0, n_slices=3)
        finally:
            if pinned:
                engine.unpin_host(d.arr)
                engine.unpin_host(i.arr)
        assert d.guards_intact() and i.guards_intact()
        out[pinned] = (d.arr[:dl].tobytes(), i.arr[:il].tobytes(), n)
    assert out[True] == out[False] == (od, oi, on)


INDEX_REC = np.dtype([("off", "<u8"), ("ks", "<u4"), ("fs", "<u4")])


def test_job_fetch_into(engine, base_runs, base_expected):
    od, oi, on = base_expected[False]
    with engine.Job(base_runs, device=0) as job:
        job.run(False)
        assert job.fetch() == (od, oi, on)
        want_bloom = job.bloom()
        ref = np.frombuffer(oi, dtype=INDEX_REC)
        for base in (0, 12_345, (1 << 32) + 7):
            d, i = Guarded(len(od)), Guarded(len(oi))
            dl, il, ms = job.fetch_into(d.arr, i.arr, index_base=base)
            assert (dl, il) == (len(od), len(oi)) and ms >= 0
            assert d.guards_intact() and i.guards_intact()
            assert d.arr.tobytes() == od
            got = np.frombuffer(i.arr.tobytes(), dtype=INDEX_REC)
            assert (got["off"] == ref["off"] + np.uint64(base)).all()
            assert (got["ks"] == ref["ks"]).all()
            assert (got["fs"] == ref["fs"]).all()
            # the job's own result is as job_run left it
            assert job.fetch() == (od, oi, on)
            assert job.bloom() == want_bloom
        # a short cap writes nothing
        for dcap, icap in ((len(od) - 1, len(oi)), (len(od), len(oi) - 16)):
            d, i = Guarded(dcap), Guarded(icap)
            with pytest.raises(engine.DbeelGpuError) as ei:
                job.fetch_into(d.arr, i.arr, index_base=5)
            assert ei.value.code == ITEM_TOO_LARGE
            assert ei.value.needed == (len(od), len(oi))
            assert d.untouched() and i.untouched()
        assert job.fetch() == (od, oi, on)


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "drop"])
def test_bloom_across_slices(engine, base_runs, base_expected, keep):
    od, oi, on = base_expected[keep]
    with engine.Job(base_runs, device=0) as job:
        job.run(keep)
        want = job.bloom()
    for n_slices in (1, 7):
        gd, gi, gn, _, bloom = _into(engine, base_runs, keep,
                                     n_slices=n_slices, bloom=True)
        assert (gn, gi, gd) == (on, oi, od)
        assert bloom == want, n_slices
    for e in parse_run(od, oi):
        assert lsm.bloom_contains(want, e.key)
    assert _into(engine, base_runs, keep, n_slices=7, bloom=False)[4] is None


def test_bloom_of_an_empty_output(engine):
    runs, _, exp_drop = load_golden("all_tombstones")
    assert exp_drop[1] == b""
    with engine.Job(runs, device=0) as job:
        job.run(False)
        want = job.bloom()
    assert _into(engine, runs, False, n_slices=3, bloom=True)[4] == want


def _dir_state(d):
    return {n: open(os.path.join(d, n), "rb").read()
            for n in sorted(os.listdir(d))}


def _two_dirs(tmp_path, runs, indices):
    dirs = []
    for name in ("whole", "stream"):
        d = str(tmp_path / name)
        for idx, (data, index) in zip(indices, runs):
            lsm.write_run_files(d, idx, bytes(data), bytes(index))
        dirs.append(d)
    return dirs


@pytest.mark.parametrize("bloom_min", [1, 1 << 30], ids=["bloom", "nobloom"])
def test_lsm_compact_stream_matches_compact(tmp_path, base_runs, bloom_min):
    runs = base_runs[:4]
    total = sum(len(d) + len(i) for d, i in runs)
    whole, stream = _two_dirs(tmp_path, runs, [0, 2, 4, 6])
    n1 = lsm.compact(whole, [0, 2, 4, 6], 7, keep_tombstones=False, device=0,
                     bloom_min_size=bloom_min)
    n2 = lsm.compact_stream(stream, [0, 2, 4, 6], 7, keep_tombstones=False,
                            device=0, max_resident_bytes=total // 4,
                            bloom_min_size=bloom_min)
    assert n1 == n2
    a, b = _dir_state(whole), _dir_state(stream)
    assert list(a) == list(b)
    assert a == b
    assert (f"{7:020d}.bloom" in b) == (bloom_min == 1)


def test_lsm_compact_stream_crash_and_replay(tmp_path, base_runs):
    runs = base_runs[:3]
    total = sum(len(d) + len(i) for d, i in runs)
    whole, stream = _two_dirs(tmp_path, runs, [0, 2, 4])
    os.environ["DBEEL_LSM_CRASH_AFTER_JOURNAL"] = "1"
    try:
        lsm.compact(whole, [0, 2, 4], 5, keep_tombstones=True, device=0,
                    bloom_min_size=1)
        lsm.compact_stream(stream, [0, 2, 4], 5, keep_tombstones=True,
                           device=0, max_resident_bytes=total // 3,
                           bloom_min_size=1)
    finally:
        del os.environ["DBEEL_LSM_CRASH_AFTER_JOURNAL"]
    # stopped after the journal: staging files, journal and inputs present.
    # The journals name their own directories, so compare names and the
    # staged bytes, not the journal's.
    a, b = _dir_state(whole), _dir_state(stream)
    assert list(a) == list(b)
    assert f"{5:020d}.compact_action" in b and f"{0:020d}.data" in b
    for n in a:
        if not n.endswith(".compact_action"):
            assert a[n] == b[n], n
    assert lsm.replay(whole) == 1 and lsm.replay(stream) == 1
    a, b = _dir_state(whole), _dir_state(stream)
    assert a == b
    assert sorted(a) == [f"{5:020d}.{e}" for e in ("bloom", "data", "index")]
