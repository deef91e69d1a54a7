"""Survivor offsets by rank tile (k_rankreduce tile sums, k_tilebase,
k_emit_tile) against the oracle and against the two per-entry scan forms.

A tile is 2048 consecutive ranks. The cases sit where the tile path can go
wrong and the per-entry scans cannot: totals on both sides of a tile edge,
a whole tile without a survivor (its base equals the next one's), no
survivor at all, waves whose ranks straddle tiles and whose lanes straddle
run seams, the rank base jumping between the jobs of a batch, the sums
re-zeroed from step to step, and both sides of the size limit up to which
the emit kernel fills the copy's window map itself.

Every case is compared byte-for-byte with the C oracle, and the same job is
run with DBEEL_SCAN_MODE unset (tiles), "rocprim" (one packed per-entry
scan) and "two" (two scans): all three must agree in data, index and count.
"""
import functools
import struct

import numpy as np
import pytest

import oracle
from dbeel_amd.format import Entry, build_run

TILE = 2048
MODES = [None, "rocprim", "two"]


def _key(i, klen=16):
    return struct.pack(">Q", i + 1) + bytes([i % 251]) * (klen - 8)


def _val(i, n=24):
    return bytes([(i * 7) % 255 + 1]) * n


@functools.lru_cache(maxsize=None)
def edge_runs(total):
    """Two runs, `total` entries in all, distinct keys interleaved, every
    fifth a tombstone."""
    ents = [Entry(_key(i), b"" if i % 5 == 4 else _val(i, 8 + i % 40), i)
            for i in range(total)]
    return (build_run(ents[0::2]), build_run(ents[1::2]))


@functools.lru_cache(maxsize=None)
def dead_tile_runs():
    """Ranks 1000 .. 1000 + 2 * TILE + 500 are tombstones: with
    keep_tombstones=False at least one whole tile has no survivor."""
    n = 1000 + 2 * TILE + 500 + 1000
    dead = range(1000, 1000 + 2 * TILE + 500)
    ents = [Entry(_key(i), b"" if i in dead else _val(i), i)
            for i in range(n)]
    return (build_run(ents[0::2]), build_run(ents[1::2]))


@functools.lru_cache(maxsize=None)
def no_survivor_runs():
    """Every key in both runs; the newer copy is always a tombstone."""
    n = TILE + 300
    return (build_run([Entry(_key(i), _val(i), 1) for i in range(n)]),
            build_run([Entry(_key(i), b"", 2) for i in range(n)]))


@functools.lru_cache(maxsize=None)
def eight_runs():
    """8 runs x 600 entries drawn round-robin from one key range, with
    some keys repeated in the next run: 600 is no multiple of 64, so run
    seams fall inside waves, and consecutive entries of a run lie 8 ranks
    apart, so every wave's ranks span several tiles' worth of lanes."""
    runs = []
    for r in range(8):
        ents = []
        for i in range(600):
            k = i * 8 + r
            if i % 9 == 0 and r:
                k -= 1  # also in run r - 1: superseded there
            ents.append(Entry(_key(k), b"" if (i + r) % 6 == 0 else
                              _val(k, 16 + (k % 64)), r))
        runs.append(build_run(sorted(ents, key=lambda e: e.key)))
    return tuple(runs)


@functools.lru_cache(maxsize=None)
def big_value_runs(vlen):
    """40 entries with vlen-byte values over two runs, small ones and a
    tombstone between them."""
    ents = []
    for i in range(60):
        if i % 3 == 2:
            ents.append(Entry(_key(i), b"" if i % 2 else _val(i, 10), i))
        else:
            ents.append(Entry(_key(i), bytes([i + 1]) * vlen, i))
    return (build_run(ents[0::2]), build_run(ents[1::2]))


# 100 KiB values: the average entry is in the > 2 KiB class, whose copy
# windows are 16 KiB, so every big entry is larger than a window and the
# window map comes from k_winmap.
# 16 KiB - 48 B values with 16-B keys: full_size = 16 + 16336 + 32 = 16384,
# exactly one window of that class; the emit kernel fills the map.
CASES = {
    "edge-1": functools.partial(edge_runs, 1),
    "edge-2047": functools.partial(edge_runs, TILE - 1),
    "edge-2048": functools.partial(edge_runs, TILE),
    "edge-2049": functools.partial(edge_runs, TILE + 1),
    "edge-4097": functools.partial(edge_runs, 2 * TILE + 1),
    "dead-tile": dead_tile_runs,
    "no-survivor": no_survivor_runs,
    "eight-runs": eight_runs,
    "values-100KiB": functools.partial(big_value_runs, 100 * 1024),
    "values-one-window": functools.partial(big_value_runs, 16384 - 48),
}


@functools.lru_cache(maxsize=None)
def expected(name, keep):
    return oracle.compact(list(CASES[name]()), keep_tombstones=keep)


def test_case_shapes():
    for total in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        runs = edge_runs(total)
        assert sum(len(ix) // 16 for _, ix in runs) == total
    assert expected("no-survivor", False) == (b"", b"", 0)
    assert expected("no-survivor", True)[2] == TILE + 300
    # dropped tombstones leave exactly the 2000 live entries
    assert expected("dead-tile", False)[2] == 2000
    ix = np.frombuffer(big_value_runs(16384 - 48)[0][1],
                       dtype=np.dtype([("off", "<u8"), ("ks", "<u4"),
                                       ("fs", "<u4")]))
    assert ix["fs"].max() == 16384
    data = sum(len(d) for d, _ in big_value_runs(16384 - 48))
    assert data // 60 > 2048  # the 16 KiB window class
    assert sum(len(d) for d, _ in big_value_runs(100 * 1024)) // 60 > 2048
    assert 0 < expected("eight-runs", False)[2] < 4800


@pytest.fixture(scope="module")
def engine():
    import dbeel_amd

    return dbeel_amd


def _compact(engine, monkeypatch, mode, runs, keep):
    if mode is None:
        monkeypatch.delenv("DBEEL_SCAN_MODE", raising=False)
    else:
        monkeypatch.setenv("DBEEL_SCAN_MODE", mode)
    return engine.compact(list(runs), keep_tombstones=keep, device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_three_modes_match_oracle(engine, monkeypatch, name, keep):
    want = expected(name, keep)
    for mode in MODES:
        got = _compact(engine, monkeypatch, mode, CASES[name](), keep)
        assert got[2] == want[2], mode
        assert got[1] == want[1], mode
        assert got[0] == want[0], mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_batch_jobs_of_different_sizes(monkeypatch, mode):
    """The second job's ranks start at the first job's entry count, in the
    middle of a tile; fetch_job slices the result there."""
    from dbeel_amd.engine import BatchJob

    if mode is None:
        monkeypatch.delenv("DBEEL_SCAN_MODE", raising=False)
    else:
        monkeypatch.setenv("DBEEL_SCAN_MODE", mode)
    jobs = [list(edge_runs(TILE + 700)), list(eight_runs()),
            list(edge_runs(333))]
    with BatchJob(jobs, device=0) as bj:
        for keep in (True, False):
            bj.run(keep)
            for j, runs in enumerate(jobs):
                assert bj.fetch_job(j) == oracle.compact(
                    runs, keep_tombstones=keep), (j, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dead-tile", "edge-4097",
                                  "values-100KiB"])
def test_same_job_alternating_keep(engine, monkeypatch, name):
    """The tile sums and the k_winmap flag are zeroed for every step:
    nothing of the step before is left in them."""
    monkeypatch.delenv("DBEEL_SCAN_MODE", raising=False)
    with engine.Job(list(CASES[name]()), device=0) as job:
        for keep in (True, False, True):
            dl, ne, _ = job.run(keep)
            got = job.fetch()
            assert (dl, ne) == (len(got[0]), got[2])
            assert got == expected(name, keep)
