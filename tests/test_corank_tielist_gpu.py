"""The block-wide tie list of k_corank.

A window's prefix-tied pairs are noted by every thread's scout, collected
into one list in LDS, settled by the whole block and handed back to the
threads that noted them. What can go wrong there and not in the walk: the
list is not rebuilt for the next window a block takes, a full list (1024
pairs) is followed by a sparse or an empty one, a pair sits at the very
first or the very last position of a window.

DBEEL_CORANK_GRID caps the number of corank blocks, so with 1 or 2 blocks
every block works through several of the three 2048-position windows the
inputs of test_corank_ties_gpu span. Every result is compared
byte-for-byte with the C oracle, for both keep_tombstones settings and both
block sizes.
"""
import functools

import numpy as np
import pytest

import oracle
import pymerge
from dbeel_amd.format import Entry, build_run
from test_corank_ties_gpu import (CASES, N_PER_RUN, _rand_keys, _val,
                                  density_runs, expected)

LIST_CASES = sorted(n for n in CASES
                    if n.startswith(("density-", "family-")))


@functools.lru_cache(maxsize=None)
def tied_free_tied_runs():
    """Three runs over keys A < C (every key of A below every key of C):
    run 0 = A, run 1 = A + C, run 2 = C. Pair (0, 1) is nothing but ties
    through A, so its first window fills the list (1024 pairs); pair
    (0, 2) shares no key, its windows have empty lists; pair (1, 2) starts
    tie-free (A alone) and ends on C, again nothing but ties. One block
    taking all windows in order goes full, empty, full."""
    rng = np.random.default_rng(4242)
    pool = _rand_keys(rng, 2 * N_PER_RUN, 32)
    A, C = pool[:N_PER_RUN], pool[N_PER_RUN:]
    r0 = [Entry(k, _val(rng), 100) for k in A]
    r1 = [Entry(k, b"" if i % 7 == 0 else _val(rng), 200)
          for i, k in enumerate(A + C)]
    r2 = [Entry(k, _val(rng), 150 if i % 2 else 250)
          for i, k in enumerate(C)]
    return (build_run(r0), build_run(r1), build_run(r2))


def _edge_runs(where):
    """Two runs of 1024 + 1024 distinct keys, one 2048-position window,
    with exactly one key present in both: the smallest of all (the pair
    takes positions 0 and 1) or the largest (positions 2046 and 2047)."""
    rng = np.random.default_rng(99 if where == "first" else 98)
    pool = _rand_keys(rng, 2047, 24)
    tie = pool[0] if where == "first" else pool[-1]
    rest = pool[1:] if where == "first" else pool[:-1]
    k0 = sorted(rest[0::2] + [tie])
    k1 = sorted(rest[1::2] + [tie])
    assert len(k0) == len(k1) == 1024
    return (build_run([Entry(k, _val(rng), 1) for k in k0]),
            build_run([Entry(k, _val(rng), 2) for k in k1]))


@functools.lru_cache(maxsize=None)
def edge_first_runs():
    return _edge_runs("first")


@functools.lru_cache(maxsize=None)
def edge_last_runs():
    return _edge_runs("last")


EXTRA = {
    "tied-free-tied": tied_free_tied_runs,
    "edge-first": edge_first_runs,
    "edge-last": edge_last_runs,
}


@functools.lru_cache(maxsize=None)
def expected_extra(name, keep):
    return oracle.compact(list(EXTRA[name]()), keep_tombstones=keep)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(EXTRA))
def test_oracle_matches_pymerge(name, keep):
    od, oi, on = expected_extra(name, keep)
    pd, pi = pymerge.merge(list(EXTRA[name]()), keep)
    assert (od, oi, on) == (pd, pi, len(pi) // 16)


def test_case_shapes():
    # j=1 shares every key: 3000 pairs over three windows, the first two
    # windows hold 1024 each, which is the list's capacity
    assert expected("density-j1-k32-lead0", True)[2] == N_PER_RUN
    assert len(density_runs(1, 32, 0)[0][1]) // 16 == N_PER_RUN
    for name in ("edge-first", "edge-last"):
        assert expected_extra(name, True)[2] == 2047
    # 2 * N distinct keys, each of them in two of the three runs
    assert expected_extra("tied-free-tied", True)[2] == 2 * N_PER_RUN


@pytest.fixture(scope="module")
def engine():
    import dbeel_amd

    return dbeel_amd


@pytest.fixture(params=["256", "512"])
def corank_block(request, monkeypatch):
    monkeypatch.setenv("DBEEL_CORANK_BLOCK", request.param)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("grid", ["1", "2"])
@pytest.mark.parametrize("name", LIST_CASES)
def test_windows_back_to_back(engine, corank_block, monkeypatch, name, grid,
                              keep):
    monkeypatch.setenv("DBEEL_CORANK_GRID", grid)
    got = engine.compact(list(CASES[name]()), keep_tombstones=keep, device=0)
    od, oi, on = expected(name, keep)
    assert got[2] == on
    assert got[1] == oi
    assert got[0] == od


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("grid", [None, "1"])
@pytest.mark.parametrize("name", sorted(EXTRA))
def test_full_empty_and_edge_lists(engine, corank_block, monkeypatch, name,
                                   grid, keep):
    if grid:
        monkeypatch.setenv("DBEEL_CORANK_GRID", grid)
    got = engine.compact(list(EXTRA[name]()), keep_tombstones=keep, device=0)
    od, oi, on = expected_extra(name, keep)
    assert got[2] == on
    assert got[1] == oi
    assert got[0] == od
