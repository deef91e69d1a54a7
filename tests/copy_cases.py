"""Directed inputs for the verbatim copy (k_winmap + k_copy) and a census
of the copy paths an output drives.

The copy kernel (dbeel_amd/csrc/dbeel_gpu.hip) cuts the OUTPUT into windows
of 8, 16, 32 or 64 KiB, stages the entries that intersect a window, fills a
granule -> entry map by one of two strategies (an entry sweep when the window
holds 128 entries or more, a per-granule bisection below that), and moves
16-byte granules: whole ones straight, a granule with an entry boundary in it
by a blend whose arithmetic depends on the phase c1 = entry_end % 16, and the
granules of the final partial window by byte loops. Which of those paths run
depends only on the output's offsets, so the cases here are laid out by
output offset: every entry carries a key that sorts in construction order
(one section byte, then a counter), and the merge merely has to reassemble
the list from three runs that also hold superseded older versions.

census() derives, exactly as the kernel does, what an expected output index
drives at one window size and grid; tests/test_copy_cases.py asserts the
conditions the case set exists for, per window size. explain_diff() names
the place of a mismatch in those terms.

Used by:
  - tests/test_copy_cases.py (CPU: census conditions, oracle vs pymerge)
A GPU module that runs these cases through every caller of launch_copy
under every geometry variant is what they are for; see DESIGN.md, "Copy
test coverage", for why the suite does not hold one yet.
"""
from __future__ import annotations

import functools

import numpy as np

from dbeel_amd.format import INDEX_DTYPE, Entry, build_run

WINDOWS = (8192, 16384, 32768, 65536)  # k_copy's compiled window sizes
FILL_SWITCH = 128                      # cnt >= 128: entry sweep, else bisect
BIG = 65536
N_RUNS = 3


# ------------------------------------------------------------------ census

def _index_arrays(index_bytes):
    rec = np.frombuffer(bytes(index_bytes), dtype=INDEX_DTYPE)
    offs = rec["offset"].astype(np.int64)
    sizes = rec["full_size"].astype(np.int64)
    return offs, sizes


def window_map(offs, total, win):
    """(win_p0, cnt, interior) per window, as k_winmap / k_copy derive them."""
    n = len(offs)
    n_windows = -(-total // win)
    starts = np.arange(n_windows, dtype=np.int64) * win
    win_p0 = np.searchsorted(offs, starts, side="right") - 1
    p_end = np.empty(n_windows, dtype=np.int64)
    p_end[:-1] = np.minimum(win_p0[1:] + 1, n)
    p_end[-1] = n
    cnt = p_end - win_p0
    interior = starts + win <= total
    return win_p0, cnt, interior


def census(index_bytes, win, grid):
    """Which copy paths an output with this index drives at window size win,
    launched with `grid` blocks. Returns a dict; every quantity is derived as
    the kernel derives it (see the module docstring)."""
    offs, sizes = _index_arrays(index_bytes)
    n = len(offs)
    out = {
        "win": win, "grid": grid, "n": n, "total": 0, "n_windows": 0,
        "tail": 0, "interior_phases": set(), "final_phases": set(),
        "cnt_values": set(), "max_cnt": 0, "sweep": False, "bisect": False,
        "edge_offsets": set(), "max_span": 0, "span_then_dense": False,
        "sweep_to_bisect": False, "bisect_to_sweep": False,
    }
    if not n:
        return out
    ends = offs + sizes
    total = int(ends[-1])
    win_p0, cnt, interior = window_map(offs, total, win)
    n_windows = len(cnt)
    out.update(total=total, n_windows=n_windows, tail=total % win,
               cnt_values=set(cnt.tolist()), max_cnt=int(cnt.max()))
    sweep = cnt >= FILL_SWITCH
    out["sweep"] = bool(sweep.any())
    out["bisect"] = bool((~sweep).any())

    # a granule with an entry boundary strictly inside it: phase = the bytes
    # of the ending entry in that granule
    inner = ends[:-1]
    phase = inner % 16
    strad = phase != 0
    gwin = (inner - phase) // win
    in_interior = interior[gwin]
    out["interior_phases"] = set(phase[strad & in_interior].tolist())
    out["final_phases"] = set(phase[strad & ~in_interior].tolist())

    # entry boundaries within 15 bytes of the edge between two windows
    r = inner % win
    after = r <= 15           # 0 .. +15 past the edge below
    before = r >= win - 15    # -15 .. -1 short of the edge above, which the
    #                           next entry (>= 32 bytes) always crosses
    out["edge_offsets"] = (set(r[after].tolist())
                           | set((r[before] - win).tolist()))

    first_w = offs // win
    last_w = (ends - 1) // win
    span = last_w - first_w + 1
    out["max_span"] = int(span.max())
    # an entry over >= 3 windows whose end is followed, in the window where
    # it ends, by nothing but entries of at most 40 bytes, enough of them
    # for the sweep fill
    for p in np.flatnonzero(span >= 3).tolist():
        w = int(ends[p] // win)
        if w >= n_windows or not sweep[w]:
            continue
        lo, hi = p + 1, int(win_p0[w] + cnt[w])
        if hi > lo and int(sizes[lo:hi].max()) <= 40:
            out["span_then_dense"] = True
            break

    # one block's consecutive grid-stride iterations: b, b + grid, ...
    if grid and n_windows > grid:
        a, b = sweep[:-grid], sweep[grid:]
        out["sweep_to_bisect"] = bool((a & ~b).any())
        out["bisect_to_sweep"] = bool((~a & b).any())
    return out


def explain_diff(got, want, index, win):
    """Where got first differs from want (both data bytes; index = the
    EXPECTED index bytes), in the copy kernel's terms at window size win."""
    got, want = bytes(got), bytes(want)
    if got == want:
        return "no difference"
    a = np.frombuffer(got, dtype=np.uint8)
    b = np.frombuffer(want, dtype=np.uint8)
    m = min(len(a), len(b))
    ne = np.flatnonzero(a[:m] != b[:m])
    head = f"lengths got {len(a)} want {len(b)}; "
    if not len(ne):
        return head + f"equal over the common {m} bytes"
    pos = int(ne[0])
    offs, sizes = _index_arrays(index)
    total = int(offs[-1] + sizes[-1])
    win_p0, cnt, interior = window_map(offs, total, win)
    w = pos // win
    gpos = pos - pos % 16
    p = int(np.searchsorted(offs, pos, side="right") - 1)
    pg = int(np.searchsorted(offs, gpos, side="right") - 1)
    e_end = int(offs[pg] + sizes[pg])
    c1 = e_end - gpos if e_end < min(gpos + 16, total) else 0
    return head + (
        f"first differing byte {pos} (got {a[pos]:#04x} want {b[pos]:#04x}), "
        f"{len(ne)} differ; win {win}: window {w} of {len(cnt)} "
        f"({'interior' if interior[w] else 'final partial'}, "
        f"cnt {int(cnt[w])} -> {'sweep' if cnt[w] >= FILL_SWITCH else 'bisect'}"
        f" fill, p0 {int(win_p0[w])}), granule {(pos % win) // 16} at byte "
        f"{gpos} (byte {pos - gpos} of it), straddle phase c1 = {c1}; owning "
        f"entry {p} [{int(offs[p])}, {int(offs[p] + sizes[p])}), byte "
        f"{pos - int(offs[p])} of it")


# ------------------------------------------------------------------ layout

class _Layout:
    """Entries in output order. Keys are one section byte then a big-endian
    counter, so construction order is key order; off tracks the output
    offset the next entry will have."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.entries = []
        self.off = 0
        self.sec = 0
        self.ctr = 0

    def section(self):
        self.sec += 1
        self.ctr = 0
        assert self.sec < 256

    def add_key(self, key, vlen):
        self.entries.append(Entry(key, self._val(vlen), 1000 + len(self.entries)))
        self.off += 32 + len(key) + vlen

    def add(self, size):
        """One entry of exactly `size` bytes: a 4-byte key and a value of at
        least one byte (an empty value would be a tombstone)."""
        assert size >= 37, size
        self.ctr += 1
        self.add_key(bytes([self.sec]) + self.ctr.to_bytes(3, "big"), size - 36)

    def _val(self, n):
        # non-zero bytes: an empty value alone is a tombstone
        return bytes(self.rng.integers(1, 256, int(n), dtype=np.uint8))

    def end_at(self, target):
        """Add entries so that the last one ends exactly at output offset
        target (at least 36 bytes ahead)."""
        gap = target - self.off
        assert gap >= 37, gap
        if gap > 3000 and self.ctr % 2:
            # every other time as many mid-sized entries, not one large one
            while target - self.off > 1200:
                self.add(300 + int(self.rng.integers(0, 200)))
            gap = target - self.off
        self.add(gap)
        assert self.off == target


def _tombstones(L, n_first):
    """The densest legal stretch: tombstones with 1- and 2-byte keys (33 and
    34 bytes), n_first x 257 of them. Kept only with keep_tombstones."""
    for _ in range(n_first):
        L.section()
        L.entries.append(Entry(bytes([L.sec]), b"", 1000 + len(L.entries)))
        L.off += 33
        for x in range(256):
            L.entries.append(Entry(bytes([L.sec, x]), b"",
                                   1000 + len(L.entries)))
            L.off += 34


def _phase_sweep(L, n):
    """Small entries whose sizes walk every residue mod 16 (values of
    1 + (37 i) % 97 bytes): every straddle phase, in sweep-filled windows."""
    L.section()
    for i in range(n):
        L.add(37 + (37 * i) % 97)


def _fill_switch(L, win, n_windows):
    """Entries of about win / 126.5 bytes: consecutive windows of size win
    hold 127 or 128 entries as the kernel counts them, either side of the
    fill switch."""
    L.section()
    target = win * 2 / 253.0
    start = L.off
    k = 0
    while L.off - start < n_windows * win:
        k += 1
        L.add(int(round(k * target)) - int(round((k - 1) * target)))


def _edges(L, offsets):
    """One entry boundary at every given offset from a 64 KiB window edge,
    which is an edge of every smaller window size too."""
    L.section()
    for d in offsets:
        edge = (L.off // BIG + 1) * BIG
        if edge + d - L.off < 37:
            edge += BIG
        L.end_at(edge + d)


def _giants(L, n, vlen, run_len):
    """Values of vlen bytes (>= 3 windows of 64 KiB each), each followed by
    run_len entries of 40 bytes."""
    L.section()
    for i in range(n):
        L.add(36 + vlen + 17 * i)
        for _ in range(run_len):
            L.add(40)


def _random(L, n, lo, hi, klen_hi=4):
    L.section()
    for _ in range(n):
        L.ctr += 1
        key = (bytes([L.sec]) + L.ctr.to_bytes(3, "big")
               + b"k" * int(L.rng.integers(0, klen_hi - 3)))
        L.add_key(key, int(L.rng.integers(lo, hi + 1)))


def _tail(L, rem, phases=False):
    """Close the output so that total % 64 KiB == rem, hence total % win ==
    rem % win for every window size. With phases, the last 33 entries are
    37 bytes each (rem >= 2048): their ends walk every residue mod 16
    inside the final window of every window size."""
    small = 33 * 37 if phases else 0
    assert not phases or 2048 <= rem < 8192
    goal = (L.off // BIG + 1) * BIG + rem
    if goal - small - L.off < 37:
        goal += BIG
    L.section()
    L.end_at(goal - small)
    for _ in range(33 if phases else 0):
        L.add(37)
    assert L.off == goal


def _split(L, seed):
    """The layout's entries dealt over N_RUNS runs, plus superseded older
    versions (other sizes, lower timestamps) in other runs: the merged
    output is exactly the layout (tombstones subject to keep_tombstones)."""
    rng = np.random.default_rng(seed)
    per = [[] for _ in range(N_RUNS)]
    for i, e in enumerate(L.entries):
        r = int(rng.integers(0, N_RUNS))
        per[r].append(e)
        if i % 16 == 3 and len(e.data) < 4096:
            old = bytes(rng.integers(0, 256, int(rng.integers(0, 90)),
                                     dtype=np.uint8))
            per[(r + 1) % N_RUNS].append(Entry(e.key, old, e.timestamp - 500))
    runs = []
    for ents in per:
        ents.sort(key=lambda e: e.key)
        keys = [e.key for e in ents]
        assert all(x < y for x, y in zip(keys, keys[1:]))
        runs.append(build_run(ents))
    return tuple(runs)


# ------------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def case_mixed():
    """Sweep-filled windows first, then windows covered by a few large
    entries, then small entries again, over more than 64 windows of 64 KiB:
    with a grid of 64 one block goes from either fill to the other. Holds
    the phase walk, the fill-switch sections of all four window sizes, and
    values over three windows followed by runs of 40-byte entries."""
    L = _Layout(0xC0B1)
    _phase_sweep(L, 3000)
    _random(L, 1700, 600, 2000, klen_hi=40)
    for win in WINDOWS:
        _fill_switch(L, win, 6)
    _phase_sweep(L, 6000)
    _giants(L, 4, 200_000, 1700)
    _phase_sweep(L, 3000)
    _tail(L, 3000, phases=True)
    return _split(L, 1)


@functools.lru_cache(maxsize=None)
def case_edges():
    """An entry boundary at every offset -15 .. +15 from a window edge, the
    windows between them covered by one large or many mid-sized entries,
    then random small values; over more than 64 windows of 64 KiB."""
    L = _Layout(0xED6E)
    _random(L, 2500, 1, 200)
    _edges(L, range(-15, 16))
    _random(L, 6000, 1, 1200, klen_hi=24)
    _edges(L, (15, -1, 0, 1, -15, 8, -8))
    _phase_sweep(L, 2500)
    _tail(L, 2500, phases=True)
    return _split(L, 2)


@functools.lru_cache(maxsize=None)
def case_tombstones():
    """24 x 257 tombstones of 33 and 34 bytes between two stretches of small
    values: kept, they fill windows to within a few entries of the staging
    capacity; dropped, the stretches meet."""
    L = _Layout(0x70B5)
    _random(L, 300, 1, 60)
    _tombstones(L, 24)
    _random(L, 300, 1, 60)
    return _split(L, 3)


@functools.lru_cache(maxsize=None)
def case_exact(n_big):
    """Odd-sized entries ending exactly on a 64 KiB edge: no partial window
    at any window size."""
    L = _Layout(0xE8AC + n_big)
    _random(L, 150 * n_big, 1, 700, klen_hi=12)
    _tail(L, 0)
    return _split(L, 4)


@functools.lru_cache(maxsize=None)
def case_short_tail(rem):
    """A final window of rem (1 .. 15) bytes at every window size: the last
    granule of the output is the tail of an entry that began in the window
    before."""
    L = _Layout(0x7A11 + rem)
    _random(L, 200, 1, 500, klen_hi=12)
    _tail(L, rem)
    return _split(L, 5)


@functools.lru_cache(maxsize=None)
def case_single():
    """One 32-byte entry: empty key, empty value (kept tombstones only)."""
    return (build_run([Entry(b"", b"", 7)]),)


CASES = {
    "mixed": case_mixed,
    "edges": case_edges,
    "tombstones": case_tombstones,
    "exact-1": functools.partial(case_exact, 1),
    "exact-3": functools.partial(case_exact, 3),
    "short-tail-1": functools.partial(case_short_tail, 1),
    "short-tail-15": functools.partial(case_short_tail, 15),
    "single": case_single,
}
GRID_STRIDE_CASES = ("mixed", "edges")  # more than 64 windows of 64 KiB
GRID = 64                               # the smallest DBEEL_COPY_GRID taken
