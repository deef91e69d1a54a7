"""Host model of the snapshot scan (dbeel_gpu_reader_scan_snapshot), for the
snapshot tests.

The snapshot's segments are the tables in list order and then — with the
memtable flag and a non-empty memtable — the memtable as one more run (from
Reader.memtable_fetch, or memtable_model / batch_model over the arrivals).
The plain result is pymm3.scan_model over those segments. newest_only drops
an entry of segment s whose key a LATER segment holds, whatever the filters
keep of that later entry (an equal key has an equal hash and the same place
relative to the key range, so this equals filtering first and keeping, per
key, the entry of the highest segment).
"""
import struct

from dbeel_amd.format import encode_entry, parse_run
from pymm3 import between_cmp, murmur3_32, scan_model


def segments(runs, mem_run=None):
    """runs + [memtable run], the memtable left out when absent or empty."""
    segs = [(bytes(d), bytes(i)) for d, i in runs]
    if mem_run is not None and len(mem_run[1]):
        segs.append((bytes(mem_run[0]), bytes(mem_run[1])))
    return segs


def snapshot_entries(segs, start_key=None, end_key=None, hash_ranges=None,
                     newest_only=False):
    """-> [(segment, Entry)] in yield order."""
    parsed = [parse_run(d, i) for d, i in segs]
    later = [set() for _ in segs]  # keys held by segments after s
    acc = set()
    for s in range(len(segs) - 1, -1, -1):
        later[s] = set(acc)
        acc |= {e.key for e in parsed[s]}
    out = []
    for s, entries in enumerate(parsed):
        for e in entries:
            if start_key is not None and e.key < start_key:
                continue
            if end_key is not None and e.key >= end_key:
                continue
            if hash_ranges:
                h = murmur3_32(e.key, 0)
                if not any(between_cmp(h, a, b) for a, b in hash_ranges):
                    continue
            if newest_only and e.key in later[s]:
                continue
            out.append((s, e))
    return out


def snapshot_model(segs, start_key=None, end_key=None, hash_ranges=None,
                   newest_only=False):
    """-> (data_bytes, index_bytes, n), scan_model's shape."""
    if not newest_only:
        return scan_model(segs, start_key, end_key, hash_ranges)
    data, index = [], []
    off = 0
    for _, e in snapshot_entries(segs, start_key, end_key, hash_ranges, True):
        raw = encode_entry(e)
        index.append(struct.pack("<QII", off, 8 + len(e.key), len(raw)))
        data.append(raw)
        off += len(raw)
    return b"".join(data), b"".join(index), len(index)


def shadowed_count(segs, start_key=None, end_key=None, hash_ranges=None):
    """Entries newest_only drops: info.shadowed after a finished scan."""
    return (len(snapshot_entries(segs, start_key, end_key, hash_ranges))
            - len(snapshot_entries(segs, start_key, end_key, hash_ranges,
                                   True)))


def first_range_ids(model, ranges):
    """u32 list: the first range matching each entry of a model result."""
    d, i, _ = model
    out = []
    for e in parse_run(d, i):
        h = murmur3_32(e.key, 0)
        out.append(next(j for j, (a, b) in enumerate(ranges)
                        if between_cmp(h, a, b)))
    return out


def self_check():
    from dbeel_amd.format import Entry, build_run

    segs = [
        build_run([Entry(b"a", b"0", 1), Entry(b"b", b"0", 1),
                   Entry(b"c", b"0", 9)]),
        build_run([Entry(b"b", b"", 2), Entry(b"d", b"1", 2)]),
        build_run([Entry(b"a", b"2", 0), Entry(b"d", b"", 3)]),
    ]
    plain = snapshot_entries(segs)
    assert len(plain) == 7
    got = snapshot_entries(segs, newest_only=True)
    keys = [e.key for _, e in got]
    assert len(keys) == len(set(keys))  # unique
    top = {}
    for s, e in plain:
        top[e.key] = (s, e)  # yield order: the highest segment comes last
    assert sorted(keys) == sorted(top)
    for s, e in got:
        assert top[e.key] == (s, e)
    # a tombstone shadows and is emitted; an earlier repeat does not shadow
    assert [(s, e.key, e.data) for s, e in got] == [
        (0, b"c", b"0"), (1, b"b", b""), (2, b"a", b"2"), (2, b"d", b"")]
    assert shadowed_count(segs) == 3
    d, i, n = snapshot_model(segs, newest_only=True)
    assert n == 4 and [e.key for e in parse_run(d, i)] == [
        b"c", b"b", b"a", b"d"]
    assert snapshot_model(segs) == scan_model(segs)
