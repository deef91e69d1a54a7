"""Host model of the reader's resident memtable, for the memtable tests.

The memtable after puts W1 ... Wk is the reference's rbtree after the same
set() calls (rbtree_arena/src/lib.rs:497-511): batch_model.flush_run over the
concatenated arrivals. The oracle for gets is a FRESH Reader over
tables + [that run], never the code under test.
"""
import numpy as np

import batch_model

I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1


def rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, int(n), dtype=np.uint8))


def key_pool(seed, n_keys, max_klen=40):
    """n_keys distinct keys of 0..max_klen B, the empty key among them."""
    rng = np.random.default_rng(seed)
    pool = {b""}
    while len(pool) < n_keys:
        pool.add(rand_bytes(rng, rng.integers(0, max_klen + 1)))
    return sorted(pool)


def gen(seed, n, pool, max_vlen=64):
    """n writes drawn from pool: values 0..max_vlen B with ~15 % tombstones,
    timestamps negative, positive and the i128 extremes (the mix of the
    write-batch tests' generator)."""
    rng = np.random.default_rng(seed)
    special = [I128_MIN, I128_MAX, -1, 0, 1]
    writes = []
    for i in range(n):
        k = pool[int(rng.integers(0, len(pool)))]
        v = (b"" if rng.random() < 0.15
             else rand_bytes(rng, rng.integers(0, max_vlen + 1)))
        t = (special[int(rng.integers(0, len(special)))] if i % 7 == 0
             else int(rng.integers(-10**15, 10**15)))
        writes.append((k, v, t))
    return writes


class Memtable:
    """The arrivals since the last flush or clear."""

    def __init__(self):
        self.arrivals = []

    def put(self, writes):
        """-> (batch_entries, replaced): distinct keys in this batch, and how
        many of them the memtable already held."""
        writes = list(writes)
        held = {w[0] for w in self.arrivals}
        batch = {w[0] for w in writes}
        self.arrivals += writes
        return len(batch), len(batch & held)

    def run(self):
        """-> (data, index) of the memtable as a flushed run; (b"", b"")
        when it is empty."""
        if not self.arrivals:
            return b"", b""
        return batch_model.flush_run(self.arrivals)

    @property
    def entries(self):
        return len({w[0] for w in self.arrivals})

    @property
    def data_bytes(self):
        return len(self.run()[0])

    def keys(self):
        return sorted({w[0] for w in self.arrivals})

    def clear(self):
        self.arrivals = []


def self_check():
    m = Memtable()
    assert m.run() == (b"", b"") and m.entries == 0
    assert m.put([(b"b", b"1", 9), (b"a", b"2", 1), (b"b", b"3", 0)]) == (2, 0)
    assert m.put([(b"a", b"", -5), (b"c", b"4", 2)]) == (2, 1)
    assert m.run() == batch_model.flush_run(
        [(b"a", b"", -5), (b"b", b"3", 0), (b"c", b"4", 2)])
    assert m.entries == 3
    m.clear()
    assert m.entries == 0
