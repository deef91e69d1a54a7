"""Host model of put_entries / scan_apply, for the migration tests.

A page is what a paged scan yields: entries in the run entry format plus
their 16-byte index records, in arrival order. Applying it is the
reference's migration loop (tasks/migration.rs:62-131): per entry the first
matching range's action, Set into another tree (set_with_timestamp,
shards.rs:768 — a set replaces whatever the timestamps are) or
tree.delete(key) on the own tree. The oracle is always
batch_model.flush_run over the arrivals (through memtable_model.Memtable)
plus a fresh Reader, never the path under test.
"""
import numpy as np

import batch_model
import memtable_model
from dbeel_amd.format import INDEX_DTYPE, Entry, build_run, decode_entry

PUT, DELETE = "put", "delete"


def decode_page(data, index):
    """-> [(key, value, ts), ...] in page order."""
    data = bytes(data)
    recs = np.frombuffer(bytes(index), dtype=INDEX_DTYPE)
    out = []
    for off, _ks, fs in recs:
        e = decode_entry(data[int(off):int(off) + int(fs)])
        out.append((e.key, e.data, e.timestamp))
    return out


def encode_page(writes):
    """(key, value, ts) in arrival order -> (data u8, index u8) numpy arrays:
    a page as scan_next writes it (offsets from 0, no sorting, no dedup)."""
    d, x = build_run(Entry(k, v, t) for k, v, t in writes)
    return (np.frombuffer(d or b"\0", dtype=np.uint8)[:len(d)].copy(),
            np.frombuffer(x, dtype=np.uint8).copy())


def selected(page, range_ids, take):
    """The page's writes the mask lets through, in page order."""
    if range_ids is None:
        return list(page)
    return [w for w, r in zip(page, range_ids) if take[int(r)]]


def apply(mem, page, range_ids=None, take=None, mode=PUT, delete_ts=None):
    """Feeds a memtable_model.Memtable with the selected writes (DELETE: a
    tombstone with delete_ts per selected entry). -> (batch_entries,
    replaced), or None when nothing was selected (no put happened)."""
    sel = selected(page, range_ids, take)
    if mode == DELETE:
        sel = [(k, b"", int(delete_ts)) for k, _, _ in sel]
    if not sel:
        return None
    return mem.put(sel)


def migrate(src_model_pages, actions, delete_ts=None):
    """src_model_pages: [(page, range_ids), ...] as the scan yields them;
    actions[id] = ("skip",) | ("put", name) | ("delete", name). -> {name:
    Memtable} after every page went through every action."""
    mems = {}
    for a in actions:
        if a[0] != "skip":
            mems.setdefault(a[1], memtable_model.Memtable())
    for page, rids in src_model_pages:
        seen = []
        for a in actions:
            if a[0] == "skip" or (a[0], a[1]) in seen:
                continue
            seen.append((a[0], a[1]))
            take = [1 if b[0] == a[0] and b[1:] == a[1:] else 0
                    for b in actions]
            apply(mems[a[1]], page,
                  rids if rids is not None else None, take, a[0], delete_ts)
    return mems


def self_check():
    page = [(b"b", b"1", 9), (b"a", b"2", 1), (b"b", b"3", 0), (b"c", b"", 4)]
    d, x = encode_page(page)
    assert decode_page(d, x) == page
    assert len(x) == 16 * len(page)
    m = memtable_model.Memtable()
    assert apply(m, page) == (3, 0)
    assert m.run() == batch_model.flush_run(
        [(b"a", b"2", 1), (b"b", b"3", 0), (b"c", b"", 4)])
    # the mask: ids {0, 2} of 4
    rids = [0, 1, 2, 3]
    m = memtable_model.Memtable()
    assert apply(m, page, rids, [1, 0, 1, 0]) == (1, 0)
    assert m.arrivals == [(b"b", b"1", 9), (b"b", b"3", 0)]
    assert apply(m, page, rids, [0, 0, 0, 0]) is None
    # DELETE: one tombstone per distinct selected key, with delete_ts
    m = memtable_model.Memtable()
    assert apply(m, page, mode=DELETE, delete_ts=-7) == (3, 0)
    assert m.run() == batch_model.flush_run(
        [(k, b"", -7) for k in (b"a", b"b", b"c")])
    mems = migrate([(page, rids)], [("put", "A"), ("delete", "S"), ("skip",),
                                    ("put", "A")], delete_ts=5)
    assert mems["A"].arrivals == [(b"b", b"1", 9), (b"c", b"", 4)]
    assert mems["S"].arrivals == [(b"a", b"", 5)]
