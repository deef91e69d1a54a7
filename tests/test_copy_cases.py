"""The copy cases are what they claim (CPU only).

tests/copy_cases.py lays its inputs out so that the expected outputs drive
every path of the verbatim copy at every compiled window size. Here the
census of the C oracle's outputs is held against that list, condition by
condition and window size by window size; the oracle is pinned on the same
inputs by the independent Python merge; and the census itself is checked on
small hand-made indexes.
"""
import functools
import struct

import numpy as np
import pytest

import oracle
import pymerge
from copy_cases import (CASES, FILL_SWITCH, GRID, GRID_STRIDE_CASES, WINDOWS,
                        census, explain_diff, window_map)
from dbeel_amd.format import INDEX_DTYPE, parse_run

ALL_PHASES = set(range(1, 16))


@functools.lru_cache(maxsize=None)
def expected(name, keep):
    return oracle.compact(list(CASES[name]()), keep_tombstones=keep)


@functools.lru_cache(maxsize=None)
def _census(name, keep, win):
    return census(expected(name, keep)[1], win, GRID)


def _all(keep, win):
    return {name: _census(name, keep, win) for name in CASES}


def _union(cs, field):
    out = set()
    for c in cs.values():
        out |= c[field]
    return out


def _index(sizes):
    off, recs = 0, []
    for s in sizes:
        recs.append(struct.pack("<QII", off, 8, s))
        off += s
    return b"".join(recs)


# ---- the census on indexes small enough to check by hand ----

def test_census_by_hand():
    # 100 entries of 100 bytes, windows of 8192: entry 81 lies across the
    # edge (8100 .. 8200), so window 0 stages entries 0 .. 81 and the final
    # window 81 .. 99
    c = census(_index([100] * 100), 8192, 64)
    assert (c["total"], c["n_windows"], c["tail"]) == (10000, 2, 1808)
    offs = np.arange(100, dtype=np.int64) * 100
    win_p0, cnt, interior = window_map(offs, 10000, 8192)
    assert win_p0.tolist() == [0, 81]
    assert cnt.tolist() == [82, 19]
    assert interior.tolist() == [True, False]
    assert c["cnt_values"] == {82, 19} and c["bisect"] and not c["sweep"]
    # ends k*100: every multiple of 4 that is no multiple of 16
    assert c["interior_phases"] == {4, 8, 12} == c["final_phases"]
    assert c["edge_offsets"] == {8}  # the boundary at 8200 = 8192 + 8
    assert c["max_span"] == 2
    assert not c["sweep_to_bisect"] and not c["bisect_to_sweep"]


def test_census_edges_spans_and_fills():
    # boundary exactly on the edge, and an entry that starts there: the
    # kernel's win_p0 of window 1 is that entry, and window 0 counts it
    c = census(_index([8192, 40]), 8192, 64)
    assert c["edge_offsets"] == {0}
    assert sorted(c["cnt_values"]) == [1, 2]
    # 15 short of the edge, then 1 past the next one
    c = census(_index([8192 - 15, 8192 + 16, 100]), 8192, 64)
    assert c["edge_offsets"] == {-15, 1}
    assert c["interior_phases"] == {1}          # 8177 % 16; 16385 is final
    assert c["final_phases"] == {1}
    # one entry over three windows and a bit, then 300 entries of 40 bytes:
    # sweep-filled window after a bisect-filled one
    c = census(_index([3 * 8192 + 100] + [40] * 300), 8192, 2)
    assert c["max_span"] == 4 and c["span_then_dense"]
    assert c["sweep"] and c["bisect"]
    # windows 0..2 hold 1 (2 for the kernel) entries, window 3 and 4 many:
    # block 1 of a grid of 2 sees windows 1 and 3 -> bisect then sweep
    assert c["bisect_to_sweep"] and not c["sweep_to_bisect"]
    assert max(c["cnt_values"]) >= FILL_SWITCH
    # no entries at all
    assert census(b"", 8192, 64)["n_windows"] == 0


def test_explain_diff_names_the_place():
    sizes = [100] * 100
    index = _index(sizes)
    want = bytes(range(250)) * 40
    assert explain_diff(want, want, index, 8192) == "no difference"
    got = bytearray(want)
    got[8195] ^= 0xFF   # granule 8192..8207 holds the boundary at 8200
    text = explain_diff(got, want, index, 8192)
    for part in ("first differing byte 8195", "window 1 of 2",
                 "final partial", "cnt 19 -> bisect", "granule 0 at byte 8192",
                 "c1 = 8", "owning entry 81 [8100, 8200)"):
        assert part in text, (part, text)
    assert "lengths got 9999" in explain_diff(want[:-1], want, index, 8192)


# ---- the inputs ----

@pytest.mark.parametrize("name", sorted(CASES))
def test_runs_are_sorted_and_entries_at_least_32(name):
    runs = CASES[name]()
    assert sum(len(d) + len(i) for d, i in runs) <= 8 << 20, "about 8 MB"
    for data, index in runs:
        rec = np.frombuffer(index, dtype=INDEX_DTYPE)
        assert (rec["full_size"] >= 32).all()
        keys = [e.key for e in parse_run(data, index)]
        assert all(x < y for x, y in zip(keys, keys[1:])), name


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_pymerge(name, keep):
    od, oi, on = expected(name, keep)
    pd, pi = pymerge.merge(list(CASES[name]()), keep)
    assert oi == pi
    assert od == pd
    assert on == len(pi) // 16


def test_unaligned_table_ends():
    """Compacted as a reader's resident tables, these runs make a granule
    that straddles the end of a table's last entry read past the table."""
    for name in GRID_STRIDE_CASES:
        tails = [len(d) % 16 for d, _ in CASES[name]()]
        assert any(tails), (name, tails)


# ---- the census conditions, per window size ----
# keep=True holds every condition. With tombstones dropped the outputs of
# all cases but "tombstones" and "single" are the same bytes, so everything
# but the tombstone density and the single entry holds there too.

@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_interior_phases(win, keep):
    got = _union(_all(keep, win), "interior_phases")
    assert got == ALL_PHASES, f"interior phases missing at {win}: " \
        f"{sorted(ALL_PHASES - got)}"
    assert got & set(range(1, 8)), f"blend branch c1 < 8 at {win}"
    assert got & set(range(9, 16)), f"blend branch c1 > 8 at {win}"
    assert 8 in got, f"blend special case c1 == 8 at {win}"


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_final_window_phases(win, keep):
    for name in GRID_STRIDE_CASES:  # each of them alone, in ONE final window
        got = _census(name, keep, win)["final_phases"]
        assert got == ALL_PHASES, f"final-window phases missing at {win} " \
            f"in {name}: {sorted(ALL_PHASES - got)}"


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_output_ends(win, keep):
    cs = _all(keep, win)
    tails = {name: c["tail"] for name, c in cs.items() if c["n"]}
    assert any(1 <= t <= 15 for t in tails.values()), \
        f"short final window (total % win in 1..15) at {win}: {tails}"
    assert {tails["short-tail-1"], tails["short-tail-15"]} == {1, 15}
    exact = [n for n, t in tails.items() if t == 0]
    assert exact, f"exact multiple (total % win == 0) at {win}: {tails}"
    assert any(cs[n]["n_windows"] > 1 for n in exact), \
        f"exact multiple of more than one window at {win}"


def test_single_entry():
    od, oi, on = expected("single", True)
    assert (len(od), len(oi), on) == (32, 16, 1), "single 32-byte entry"
    assert expected("single", False) == (b"", b"", 0)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_fill_switch(win, keep):
    cs = _all(keep, win)
    cnts = _union(cs, "cnt_values")
    assert FILL_SWITCH - 1 in cnts, f"cnt == 127 (last bisect) at {win}"
    assert FILL_SWITCH in cnts, f"cnt == 128 (first sweep) at {win}"
    assert any(c["sweep"] and c["bisect"] for c in cs.values()), \
        f"both fill paths in one output at {win}"
    assert 1 in cnts, f"window covered by one entry (cnt == 1) at {win}"


@pytest.mark.parametrize("win", WINDOWS)
def test_densest_window(win):
    c = _census("tombstones", True, win)
    assert c["max_cnt"] >= win // 34, \
        f"densest window (cnt >= win/34) at {win}: {c['max_cnt']}"
    assert c["max_cnt"] <= win // 32 + 4, "within the kernel's SPAN"
    # the case is what it says: those windows hold kept tombstones of 33/34 B
    od, oi, on = expected("tombstones", True)
    sizes = np.frombuffer(oi, dtype=INDEX_DTYPE)["full_size"]
    assert ((sizes == 33) | (sizes == 34)).sum() == 24 * 257
    assert on - expected("tombstones", False)[2] == 24 * 257


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_boundaries_at_window_edges(win, keep):
    got = _union(_all(keep, win), "edge_offsets")
    for lo, hi, what in ((-15, -1, "before the edge (last granule of a "
                          "window straddles)"),
                         (0, 0, "exactly on the edge"),
                         (1, 15, "past the edge (first granule of the next "
                          "window straddles, entry 0 starts before wstart)")):
        missing = sorted(set(range(lo, hi + 1)) - got)
        assert not missing, f"entry boundary {what} at {win}: {missing}"


@pytest.mark.parametrize("keep", [True, False])
def test_spanning_entries(keep):
    c = _census("mixed", keep, 65536)
    assert c["max_span"] >= 3, "an entry over >= 3 windows of 64 KiB"
    sizes = np.frombuffer(expected("mixed", keep)[1],
                          dtype=INDEX_DTYPE)["full_size"]
    assert sizes.max() >= 200_000
    for win in WINDOWS:
        assert _census("mixed", keep, win)["span_then_dense"], \
            f"dense run of <= 40-byte entries after a spanning entry at {win}"


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_grid_stride(win, keep):
    for name in GRID_STRIDE_CASES:
        c = _census(name, keep, win)
        assert c["n_windows"] > GRID, \
            f"more than {GRID} windows at {win} in {name}: {c['n_windows']}"
        # the engine sizes its grid from the input bytes: no fewer windows
        in_bytes = sum(len(d) for d, _ in CASES[name]())
        assert -(-in_bytes // win) >= GRID
    c = _census("mixed", keep, win)
    assert c["sweep_to_bisect"], \
        f"one block goes sweep -> bisect at {win}, grid {GRID}"
    assert c["bisect_to_sweep"], \
        f"one block goes bisect -> sweep at {win}, grid {GRID}"
