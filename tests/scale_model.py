"""Vectorised host models for the tests that drive the kernels past the
launch-grid cap (test_grid_cap_gpu.py). numpy only, never the code under
test; the per-entry Python models of the other modules (parse_run,
batch_model, pymm3, snapshot_model) take many seconds at half a million
entries, these take a fraction of one. test_scale_model.py ties each of them
to the slow model it restates.

Everything here is for FIXED-WIDTH keys: a key set is a (n, K) uint8 matrix,
compared as numpy "S<K>" scalars, whose order among equal-width values is
the byte-lexicographic order of the reference's Vec<u8>. Ragged keys are
outside these models; the tests that need them run at sizes where the slow
models are quick enough.

A set of entries is an `Entries`: keys (n, K) u8, vlen (n,) i64 with every
non-zero length equal to V, vals (n, V) u8 (rows of tombstones ignored) and
ts (n, 16) u8, the i128 timestamp's little-endian bytes.
"""
from dataclasses import dataclass

import numpy as np

from dbeel_amd.engine import HIT_DTYPE
from dbeel_amd.format import INDEX_DTYPE, build_run_fixed_key

BLOCK = 256
WAVE = 64


# ---------------------------------------------------------------- the cap
def first_strided(grid_for, lanes_per_item: int = 1) -> int:
    """The number of items the capped grid covers in ONE trip of the
    grid-stride loop: items with an index >= it are reached only by a later
    trip. Found from the engine's own grid function: one less than the
    smallest n with grid_for(n * lanes, BLOCK) * BLOCK < n * lanes."""
    def over(n):
        return grid_for(n * lanes_per_item, BLOCK) * BLOCK < n * lanes_per_item

    lo, hi = 1, 1 << 40
    assert over(hi), "no cap below 2^40 items"
    while lo < hi:
        mid = (lo + hi) // 2
        if over(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo - 1


def sizes(grid_for):
    """-> (T, W, N_T, N_W): the thread-per-item and wave-per-item caps and
    the sizes the tests use. N_T ends a second trip inside a block; N_W
    gives the wave kernels a third trip."""
    t = first_strided(grid_for, 1)
    w = first_strided(grid_for, WAVE)
    return t, w, t + 2 * BLOCK + 37, 2 * w + 5


# ------------------------------------------------------------------- keys
def skeys(keys) -> np.ndarray:
    """(n, K) u8 -> (n,) S<K>."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    return keys.view(f"S{keys.shape[1]}").reshape(-1)


def key_list(keys):
    """(n, K) u8 -> list of K-byte bytes, for the engine's list arguments."""
    blob = np.ascontiguousarray(keys, dtype=np.uint8).tobytes()
    k = keys.shape[1]
    return [blob[i:i + k] for i in range(0, len(blob), k)]


def gather(data, off, length) -> np.ndarray:
    """concat(data[off[i] : off[i] + length[i]])."""
    off = np.asarray(off, dtype=np.int64)
    length = np.asarray(length, dtype=np.int64)
    total = int(length.sum())
    if not total:
        return np.zeros(0, dtype=np.uint8)
    starts = np.cumsum(length) - length
    idx = np.arange(total, dtype=np.int64) + np.repeat(off - starts, length)
    return data[idx]


def offsets_of(length) -> np.ndarray:
    out = np.zeros(len(length) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(length, dtype=np.uint64), out=out[1:])
    return out


@dataclass
class Entries:
    keys: np.ndarray
    vlen: np.ndarray
    vals: np.ndarray
    ts: np.ndarray

    def __len__(self):
        return self.keys.shape[0]

    def take(self, idx):
        return Entries(self.keys[idx], self.vlen[idx], self.vals[idx],
                       self.ts[idx])

    @staticmethod
    def concat(parts):
        return Entries(*(np.concatenate([getattr(p, f) for p in parts])
                         for f in ("keys", "vlen", "vals", "ts")))

    def writes(self):
        """The engine's write list: (key, value, timestamp int)."""
        ks = key_list(self.keys)
        v = self.vals.shape[1]
        vb = np.ascontiguousarray(self.vals).tobytes()
        tb = np.ascontiguousarray(self.ts).tobytes()
        vl = self.vlen.tolist()
        return [(ks[i], vb[i * v:i * v + vl[i]],
                 int.from_bytes(tb[16 * i:16 * i + 16], "little", signed=True))
                for i in range(len(ks))]


def ts_bytes(lo, hi=None) -> np.ndarray:
    """u64 low halves (and optional i64 high halves) -> (n, 16) u8."""
    lo = np.asarray(lo, dtype="<u8")
    out = np.zeros((lo.size, 16), dtype=np.uint8)
    out[:, :8] = lo.view(np.uint8).reshape(-1, 8)
    if hi is not None:
        out[:, 8:] = np.asarray(hi, dtype="<i8").view(np.uint8).reshape(-1, 8)
    return out


def encode_run(e: Entries):
    """Entries already in key order, unique -> (data u8, index u8): the run
    file through build_run_fixed_key, the timestamps' high halves written in
    afterwards (the builder knows only the low ones)."""
    lo = np.ascontiguousarray(e.ts[:, :8]).view("<u8").reshape(-1)
    data, index = build_run_fixed_key(
        e.keys, e.vlen.astype(np.uint64),
        e.vals[e.vlen != 0].reshape(-1), lo)
    hi = e.ts[:, 8:]
    if hi.any():
        rec = index.view(INDEX_DTYPE)
        pos = (rec["offset"] + rec["full_size"] - 8).astype(np.int64)
        data = data.copy()
        data[pos[:, None] + np.arange(8)] = hi
    return data, index


class Table:
    """A run file of K-byte keys decoded from its index array and key
    matrix: off / full per entry, keys (n, K), voff / vlen of the value
    bytes, ts (n, 16)."""

    def __init__(self, data, index, K: int):
        self.data = (data if isinstance(data, np.ndarray)
                     else np.frombuffer(bytes(data), dtype=np.uint8))
        rec = (index if isinstance(index, np.ndarray)
               else np.frombuffer(bytes(index), dtype=np.uint8)
               ).view(INDEX_DTYPE)
        assert np.all(rec["key_size"] == 8 + K), "fixed-width keys only"
        self.K = K
        self.n = rec.size
        self.off = rec["offset"].astype(np.int64)
        self.full = rec["full_size"].astype(np.int64)
        self.voff = self.off + 16 + K
        self.vlen = self.full - 32 - K
        if self.n:
            self.keys = self.data[(self.off + 8)[:, None] + np.arange(K)]
            self.ts = self.data[(self.off + self.full - 16)[:, None]
                                + np.arange(16)]
        else:
            self.keys = np.zeros((0, K), dtype=np.uint8)
            self.ts = np.zeros((0, 16), dtype=np.uint8)
        self.skeys = skeys(self.keys)

    def entries(self) -> Entries:
        v = int(self.vlen.max()) if self.n else 0
        vals = np.zeros((self.n, v), dtype=np.uint8)
        nz = np.flatnonzero(self.vlen)
        assert np.all(self.vlen[nz] == v)
        if nz.size:
            vals[nz] = self.data[self.voff[nz][:, None] + np.arange(v)]
        return Entries(self.keys, self.vlen.copy(), vals, self.ts)


# ------------------------------------------------------------- read model
class ReadModel:
    """key -> (highest run index, value offset, value length, tombstone, 16
    timestamp bytes) over runs [(data, index), ...] of K-byte keys; mem_run,
    a non-empty memtable's run file, is consulted first and reported at run
    == len(runs) (LSMTree::get_entry, lsm_tree.rs:674-723)."""

    def __init__(self, runs, K: int, mem_run=None):
        self.n_runs = len(runs)
        tabs = [Table(d, i, K) for d, i in runs]
        if mem_run is not None and len(mem_run[1]):
            tabs.append(Table(mem_run[0], mem_run[1], K))
        self.tabs = tabs
        lens = [t.data.size for t in tabs]
        base = np.cumsum([0] + lens)[:-1]
        self.blob = (np.concatenate([t.data for t in tabs]) if tabs
                     else np.zeros(0, dtype=np.uint8))
        keys = np.concatenate([t.skeys for t in tabs])
        run = np.concatenate([np.full(t.n, r, dtype=np.int32)
                              for r, t in enumerate(tabs)])
        order = np.lexsort((run, keys))  # by key, then run
        ks = keys[order]
        last = np.ones(ks.size, dtype=bool)
        last[:-1] = ks[1:] != ks[:-1]    # the highest run of each key
        sel = order[last]
        self.keys = keys[sel]
        self.run = run[sel]
        self.voff = np.concatenate([t.voff for t in tabs])[sel]
        self.vlen = np.concatenate([t.vlen for t in tabs])[sel]
        self.ts = np.concatenate([t.ts for t in tabs])[sel]
        self._gvoff = self.voff + base[self.run]  # into self.blob

    def find(self, q):
        """q (n, K) u8 -> (found bool, position in the model's arrays)."""
        qs = skeys(q)
        pos = np.minimum(np.searchsorted(self.keys, qs), self.keys.size - 1)
        return self.keys[pos] == qs, pos

    def hits(self, q) -> np.ndarray:
        found, pos = self.find(q)
        h = np.zeros(len(q), dtype=HIT_DTYPE)
        h["run"] = np.where(found, self.run[pos], -1)
        h["value_offset"] = np.where(found, self.voff[pos], 0)
        h["value_len"] = np.where(found, self.vlen[pos], 0)
        h["is_tombstone"] = found & (self.vlen[pos] == 0)
        return h

    def values(self, q):
        """-> (value_offsets u64[n+1], values u8 packed in query order)."""
        found, pos = self.find(q)
        length = np.where(found, self.vlen[pos], 0)
        return offsets_of(length), gather(self.blob, self._gvoff[pos], length)

    def records(self, q):
        """get_entries' records `data_len | data | timestamp`, which lie
        contiguous in the run: -> (record_offsets u64[n+1], records u8)."""
        found, pos = self.find(q)
        length = np.where(found, self.vlen[pos] + 24, 0)
        return (offsets_of(length),
                gather(self.blob, self._gvoff[pos] - 8, length))

    def timestamps(self, q):
        """-> (found, ts (n, 16) u8, zero where absent)."""
        found, pos = self.find(q)
        return found, np.where(found[:, None], self.ts[pos], 0).astype(
            np.uint8)


def paging(offsets, cap: int) -> dict:
    """get_entries_model.paging over an offset array."""
    n = len(offsets) - 1
    n_done = int(np.searchsorted(offsets, cap, side="right")) - 1
    return {"n_done": n_done, "records_len": int(offsets[n_done]),
            "records_total": int(offsets[n]),
            "needed": int(offsets[n_done + 1] - offsets[n_done])
            if n_done < n else 0}


# ------------------------------------------------------------ merge model
def merge_expect(answers):
    """merge_model.expect over arrays. answers: per candidate — the sources
    in order, the local reader LAST — its get_entries answer to the same
    queries as (record_offsets u64[n+1], records u8). The winner of a query
    has the greatest i128 timestamp, the highest candidate among equals
    (tasks/db_server.rs:338-363). -> (hits MERGE_HIT_DTYPE, record_offsets,
    the winners' records)."""
    from dbeel_amd.engine import MERGE_HIT_DTYPE

    n = len(answers[0][0]) - 1
    have = np.zeros(n, dtype=bool)
    best_hi = np.zeros(n, dtype=np.int64)
    best_lo = np.zeros(n, dtype=np.uint64)
    winner = np.full(n, -1, dtype=np.int32)
    founds, his, los = [], [], []
    for c, (off, rec) in enumerate(answers):
        off = np.asarray(off, dtype=np.uint64).astype(np.int64)
        rec = _u8(rec)
        found = off[1:] > off[:-1]
        at = np.where(found, off[1:] - 16, 0)
        ts = (rec[at[:, None] + np.arange(16)] if rec.size
              else np.zeros((n, 16), dtype=np.uint8))
        lo = np.ascontiguousarray(ts[:, :8]).view("<u8").reshape(-1)
        hi = np.ascontiguousarray(ts[:, 8:]).view("<i8").reshape(-1)
        ge = (hi > best_hi) | ((hi == best_hi) & (lo >= best_lo))
        take = found & (~have | ge)
        winner[take] = c
        best_hi = np.where(take, hi, best_hi)
        best_lo = np.where(take, lo, best_lo)
        have |= found
        founds.append(found), his.append(hi), los.append(lo)
    stale = np.zeros(n, dtype=np.uint64)
    for c in range(len(answers)):
        older = (his[c] < best_hi) | ((his[c] == best_hi)
                                      & (los[c] < best_lo))
        stale |= np.where(have & (~founds[c] | older), np.uint64(1 << c),
                          np.uint64(0))
    length = np.zeros(n, dtype=np.int64)
    src_off = np.zeros(n, dtype=np.int64)
    base = 0
    blobs = []
    for c, (off, rec) in enumerate(answers):
        off = np.asarray(off, dtype=np.uint64).astype(np.int64)
        w = winner == c
        length[w] = (off[1:] - off[:-1])[w]
        src_off[w] = off[:-1][w] + base
        blobs.append(_u8(rec))
        base += blobs[-1].size
    hits = np.zeros(n, dtype=MERGE_HIT_DTYPE)
    hits["source"] = winner
    hits["is_tombstone"] = have & (length == 24)
    hits["value_len"] = np.maximum(length - 24, 0)
    hits["stale_mask"] = stale
    return hits, offsets_of(length), gather(np.concatenate(blobs), src_off,
                                            length)


# ------------------------------------------------------------ flush model
def last_arrivals(keys) -> np.ndarray:
    """Arrival indices of the survivors of a write batch, in key order: a
    stable sort by key keeps arrival order inside a key, and the last
    arrival of each key wins (rbtree set(), rbtree_arena/src/lib.rs:497)."""
    ks = skeys(keys)
    order = np.argsort(ks, kind="stable")
    s = ks[order]
    last = np.ones(s.size, dtype=bool)
    last[:-1] = s[1:] != s[:-1]
    return order[last]


def flush_model(arrivals: Entries):
    """-> (survivors Entries in key order, (data, index) of the flushed
    run)."""
    surv = arrivals.take(last_arrivals(arrivals.keys))
    return surv, encode_run(surv)


def prefix_tied(keys) -> int:
    """batch_model.prefix_tied for keys of at least 8 bytes."""
    p = np.ascontiguousarray(keys[:, :8]).view(">u8").reshape(-1)
    _, counts = np.unique(p, return_counts=True)
    return int(counts[counts > 1].sum())


# ---------------------------------------------------------------- murmur3
def _rotl32(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def murmur3_32(keys, seed: int = 0) -> np.ndarray:
    """MurmurHash3 x86_32 of every row of a (n, K) u8 matrix -> u32."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    n, K = keys.shape
    c1, c2 = np.uint32(0xCC9E2D51), np.uint32(0x1B873593)
    h = np.full(n, seed, dtype=np.uint32)
    nb = K // 4
    if nb:
        blocks = np.ascontiguousarray(keys[:, :4 * nb]).view("<u4")
        for i in range(nb):
            k = blocks[:, i] * c1
            k = _rotl32(k, 15) * c2
            h = _rotl32(h ^ k, 13) * np.uint32(5) + np.uint32(0xE6546B64)
    tail = K - 4 * nb
    if tail:
        k = np.zeros(n, dtype=np.uint32)
        for j in range(tail - 1, -1, -1):
            k = (k << np.uint32(8)) | keys[:, 4 * nb + j].astype(np.uint32)
        h = h ^ (_rotl32(k * c1, 15) * c2)
    h = h ^ np.uint32(K)
    h = (h ^ (h >> np.uint32(16))) * np.uint32(0x85EBCA6B)
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def between(h, start: int, end: int):
    """pymm3.between_cmp over an array (tasks/migration.rs:54-60)."""
    s, e = np.uint32(start), np.uint32(end)
    if end < start:
        return (h < s) | (h >= e)
    return (h >= s) & (h < e)


def first_range(h, ranges) -> np.ndarray:
    """Index of the first range holding each hash, -1 = none."""
    rid = np.full(h.size, -1, dtype=np.int64)
    for j in range(len(ranges) - 1, -1, -1):
        rid = np.where(between(h, *ranges[j]), j, rid)
    return rid


# ------------------------------------------------------------- scan model
def scan_model(tabs, start_key=None, end_key=None, ranges=None,
               newest_only=False):
    """engine.scan / the snapshot scan over segments tabs (Tables, in yield
    order; the memtable's run last): -> (data u8, index u8, range ids u32,
    shadowed). Filters as pymm3.scan_model; newest_only as snapshot_model:
    an entry is dropped when a later segment holds its key, and `shadowed`
    counts the entries that passed the filters and were dropped for it.
    start_key / end_key are K-byte keys."""
    datas, fulls, rids = [], [], []
    shadowed = 0
    for s, t in enumerate(tabs):
        lo, hi = 0, t.n
        if start_key is not None:
            lo = int(np.searchsorted(
                t.skeys, np.array([start_key], dtype=t.skeys.dtype))[0])
        if end_key is not None:
            hi = int(np.searchsorted(
                t.skeys, np.array([end_key], dtype=t.skeys.dtype))[0])
        mask = np.zeros(t.n, dtype=bool)
        mask[lo:max(lo, hi)] = True
        rid = np.zeros(t.n, dtype=np.int64)
        if ranges:
            rid = first_range(murmur3_32(t.keys), ranges)
            mask &= rid >= 0
        if newest_only and s + 1 < len(tabs):
            later = np.concatenate([u.skeys for u in tabs[s + 1:]])
            shadow = np.isin(t.skeys, later)
            shadowed += int((mask & shadow).sum())
            mask &= ~shadow
        datas.append(gather(t.data, t.off[mask], t.full[mask]))
        fulls.append(t.full[mask])
        rids.append(rid[mask])
    full = np.concatenate(fulls) if fulls else np.zeros(0, dtype=np.int64)
    idx = np.zeros(full.size, dtype=INDEX_DTYPE)
    idx["offset"] = offsets_of(full)[:-1]
    idx["key_size"] = 8 + (tabs[0].K if tabs else 0)
    idx["full_size"] = full
    return (np.concatenate(datas) if datas else np.zeros(0, dtype=np.uint8),
            idx.view(np.uint8).reshape(-1),
            np.concatenate(rids).astype(np.uint32) if rids
            else np.zeros(0, dtype=np.uint32), shadowed)


# ------------------------------------------------------------ comparisons
def _u8(x) -> np.ndarray:
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(x), dtype=np.uint8)


def mismatch_bytes(got, exp):
    """None when two byte strings / arrays are equal in length and in every
    byte; otherwise a description naming the first differing byte."""
    g, e = _u8(got), _u8(exp)
    if g.size != e.size:
        return f"length {g.size} != expected {e.size}"
    bad = np.flatnonzero(g != e)
    if bad.size:
        i = int(bad[0])
        return (f"{bad.size} bytes differ, first at {i}: "
                f"{int(g[i]):#04x} != expected {int(e[i]):#04x}")
    return None


def mismatch_fields(got, exp, fields=None):
    """None when two arrays (structured: field by field) agree in shape and
    in every element; otherwise the field and the first differing index."""
    if got.shape != exp.shape:
        return f"shape {got.shape} != expected {exp.shape}"
    names = fields or got.dtype.names or (None,)
    for f in names:
        g, e = (got, exp) if f is None else (got[f], exp[f])
        bad = np.flatnonzero(g != e)
        if bad.size:
            i = int(bad[0])
            return (f"{f or 'array'}: {bad.size} differ, first at {i}: "
                    f"{g[i]} != expected {e[i]}")
    return None


def mismatch_guard(buf, used: int, guard: int):
    """None when every byte of buf from `used` on still holds the guard."""
    tail = _u8(buf)[used:]
    bad = np.flatnonzero(tail != guard)
    if bad.size:
        return f"{bad.size} bytes past {used} written, first at " \
               f"{used + int(bad[0])}"
    return None


def assert_bytes(got, exp, what=""):
    m = mismatch_bytes(got, exp)
    assert m is None, f"{what}: {m}"


def assert_fields(got, exp, what="", fields=None):
    m = mismatch_fields(got, exp, fields)
    assert m is None, f"{what}: {m}"


def assert_guard(buf, used, guard, what=""):
    m = mismatch_guard(buf, used, guard)
    assert m is None, f"{what}: {m}"


# -------------------------------------------------------------- generator
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def make_keys(rng, n: int, pool: int) -> np.ndarray:
    """n distinct 16-byte keys, not sorted: the first 8 bytes drawn from
    `pool` random values (so most keys share their 8-byte prefix with
    another), the second 8 a bijection of the row number (so every key is
    unique)."""
    keys = np.empty((n, 16), dtype=np.uint8)
    prefixes = rng.integers(0, 2**63, size=pool, dtype=np.uint64)
    keys[:, :8] = prefixes[rng.integers(0, pool, size=n)].astype(
        ">u8").view(np.uint8).reshape(n, 8)
    base = rng.integers(0, 2**63, dtype=np.uint64)
    keys[:, 8:] = ((np.arange(n, dtype=np.uint64) + base) * GOLDEN).astype(
        ">u8").view(np.uint8).reshape(n, 8)
    return keys


def make_entries(rng, keys, tombstone_frac: float, ts_base: int,
                 V: int = 8) -> Entries:
    """Entries over keys (any order): values of V bytes, none of them zero,
    a fraction tombstones, timestamps ts_base + a random 40-bit amount."""
    n = keys.shape[0]
    vlen = np.where(rng.random(n) < tombstone_frac, 0, V).astype(np.int64)
    vals = rng.integers(1, 256, size=(n, V), dtype=np.uint8)
    ts = ts_bytes(np.uint64(ts_base)
                  + rng.integers(0, 1 << 40, size=n, dtype=np.uint64))
    return Entries(keys, vlen, vals, ts)


def sorted_entries(e: Entries) -> Entries:
    return e.take(np.argsort(skeys(e.keys), kind="stable"))


def make_remote(rng, held: Entries, n: int, ts_base: int) -> Entries:
    """Another replica's table of n entries in key order: three quarters of
    its keys are drawn from `held` (unique keys), every eighth of those with
    the holder's own timestamp (a tie), the others with ts_base + a random
    40-bit amount; one quarter are keys of its own. A tenth tombstones."""
    k = 3 * n // 4
    pick = rng.permutation(len(held))[:k]
    own = make_keys(rng, n - k, max(1, (n - k) // 3))
    e = make_entries(rng, np.concatenate([held.keys[pick], own]), 0.10,
                     ts_base)
    tie = np.arange(0, k, 8)
    e.ts[tie] = held.ts[pick[tie]]
    return sorted_entries(e)


def make_pair(n: int, seed: int):
    """The two tables of the grid-cap tests: Entries A and B of n entries
    each in key order, about half of B's keys also in A, about a tenth
    tombstones, 8-byte values, 16-byte keys with a prefix pool of n // 3.
    -> (A, B, absent keys (n // 4, 16))."""
    rng = np.random.default_rng(seed)
    half = n // 2
    pool = make_keys(rng, 2 * n - half + n // 4, max(1, n // 3))
    a_keys = pool[:n]
    shared = a_keys[rng.permutation(n)[:half]]
    b_keys = np.concatenate([shared, pool[n:2 * n - half]])
    absent = pool[2 * n - half:]
    A = sorted_entries(make_entries(rng, a_keys, 0.10, 1 << 41))
    B = sorted_entries(make_entries(rng, b_keys, 0.10, 1 << 42))
    return A, B, absent
