"""Host model of the reference's memtable + flush, for the write-batch tests.

The memtable is a RedBlackTree<Vec<u8>, EntryValue> whose set() replaces the
value of an equal key whatever the timestamps are
(rbtree_arena/src/lib.rs:497-511); flush iterates it in key order into
EntryWriter (lsm_tree.rs:882-889, 925-946). Python's bytes order is the
byte-lexicographic order of Vec<u8> (a proper prefix first, b"" smallest).
"""
from collections import Counter

from dbeel_amd.format import Entry, build_run


def flush_entries(writes):
    """writes = iterable of (key, value, timestamp) in arrival order ->
    the flushed run's entries: one per key, ascending, last arrival wins."""
    d = {}
    for k, v, t in writes:
        d[bytes(k)] = (bytes(v), int(t))
    return [Entry(k, *d[k]) for k in sorted(d)]


def flush_run(writes):
    """-> (data_bytes, index_bytes) of the flushed run."""
    return build_run(flush_entries(writes))


def prefix_tied(writes):
    """Writes whose zero-padded 8-byte key prefix equals another write's."""
    c = Counter(bytes(k[:8]).ljust(8, b"\0") for k, _, _ in writes)
    return sum(v for v in c.values() if v > 1)


def self_check():
    """The reference's own rbtree case (rbtree_arena/src/lib.rs tests):
    set("B","are"), set("A","B"), set("A","Trees") iterates as A -> Trees,
    B -> are."""
    got = flush_entries([(b"B", b"are", 3), (b"A", b"B", 2),
                         (b"A", b"Trees", 1)])
    assert [(e.key, e.data, e.timestamp) for e in got] == [
        (b"A", b"Trees", 1), (b"B", b"are", 3)]
    # order: proper prefix first, the empty key smallest, zero bytes count
    keys = [b"ab\0\0", b"ab", b"", b"ab\0", b"b", b"ab\0\0\0\0\0\0\0"]
    got = [e.key for e in flush_entries((k, b"v", 0) for k in keys)]
    assert got == [b"", b"ab", b"ab\0", b"ab\0\0", b"ab\0\0\0\0\0\0\0", b"b"]
    # the zero-padded prefix ties b"ab" with b"ab\0..." but not with b"b"
    assert prefix_tied((k, b"", 0) for k in keys) == 4
    assert prefix_tied([(b"k", b"", 0)]) == 0
