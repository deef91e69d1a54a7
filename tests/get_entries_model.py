"""Host model of dbeel_gpu_reader_get_entries, for its tests. Pure Python,
never the code under test.

The read path is the reference's get_entry (lsm_tree.rs:674-723): the
memtable first (last arrival wins, rbtree_arena/src/lib.rs:497-511), then the
runs newest index first, the first key match winning whatever the timestamps.
The record of a found key, a tombstone included, is the stored
`data_len | data | timestamp` — the entry's encoding without its
`key_len | key` head — and record_offsets is the exclusive prefix sum of the
record sizes over all queries. A page delivers the longest prefix of queries
whose records fit the cap.
"""
import numpy as np

from dbeel_amd.format import Entry, encode_entry, parse_run

ITEM_TOO_LARGE = 3


def record_of(e: Entry) -> bytes:
    return encode_entry(e)[8 + len(e.key):]


def paging(offsets, cap):
    """The paging rule on an offset list (n + 1 ascending values, the first
    0): -> (rc, page dict). n_done is the largest d with offsets[d] <= cap;
    a first record over the cap is ITEM_TOO_LARGE."""
    n = len(offsets) - 1
    assert n >= 0 and offsets[0] == 0
    n_done = max(d for d in range(n + 1) if offsets[d] <= cap)
    page = {
        "n_done": n_done,
        "records_len": offsets[n_done],
        "records_total": offsets[n],
        "needed": offsets[n_done + 1] - offsets[n_done] if n_done < n else 0,
    }
    return (ITEM_TOO_LARGE if n and n_done == 0 else 0), page


class Model:
    """key -> (run, offset of the value bytes in that run's data, Entry) over
    runs [(data, index), ...] and, optionally, a memtable_model.Memtable
    (reported at run == len(runs), offsets into its flushed run's data)."""

    def __init__(self, runs, memtable=None):
        self.n_runs = len(runs)
        self.where = {}
        tables = [(bytes(d), bytes(i)) for d, i in runs]
        if memtable is not None and memtable.arrivals:
            tables.append(memtable.run())
        for r, (d, i) in enumerate(tables):  # the highest index wins
            off = 0
            for e in parse_run(d, i):
                self.where[e.key] = (r, off + 16 + len(e.key), e)
                off += 32 + len(e.key) + len(e.data)

    def expect(self, keys, cap=None):
        """-> (hits as a list of (run, is_tombstone, value_offset, value_len),
        offsets list, the records of ALL queries as one bytes, rc, page).
        cap None = everything fits. The delivered bytes are
        records[:page["records_len"]]."""
        hits, offsets, recs = [], [0], []
        for k in keys:
            if k in self.where:
                r, voff, e = self.where[k]
                hits.append((r, int(not e.data), voff, len(e.data)))
                recs.append(record_of(e))
            else:
                hits.append((-1, 0, 0, 0))
                recs.append(b"")
            offsets.append(offsets[-1] + len(recs[-1]))
        rc, page = paging(offsets, offsets[-1] if cap is None else cap)
        return hits, offsets, b"".join(recs), rc, page

    def entries(self, keys):
        """Reader.get_entries' answer: None | (data, timestamp)."""
        return [(self.where[k][2].data, self.where[k][2].timestamp)
                if k in self.where else None for k in keys]


def hits_array(hits, dtype):
    return np.array(hits, dtype=dtype) if hits else np.zeros(0, dtype=dtype)


def self_check():
    e = Entry(b"key", b"value", -2)
    assert record_of(e) == ((5).to_bytes(8, "little") + b"value"
                            + (-2).to_bytes(16, "little", signed=True))
    assert len(record_of(Entry(b"k", b"", 7))) == 24
    assert paging([0], 0) == (0, {"n_done": 0, "records_len": 0,
                                  "records_total": 0, "needed": 0})
