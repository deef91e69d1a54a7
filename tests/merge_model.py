"""Host model of dbeel_gpu_reader_get_merged, for its tests. Pure Python,
never the code under test.

The replicated read of the reference (tasks/db_server.rs:338-363) collects
the remote replicas' Option<EntryValue> answers, pushes the local one last,
drops the absent ones (flatten), takes max_by_key(timestamp) — which returns
the LAST maximum — and only then tests for a tombstone. A candidate here is a
get_entries_model.Model (a reader) or a raw (record_offsets, records) answer
pair; the local model is the last candidate. Records are get_entries'
`data_len | data | timestamp`, and the page is get_entries_model.paging on the
winners' record sizes.
"""
import get_entries_model as gem

I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1


def ts_of(rec: bytes) -> int:
    return int.from_bytes(rec[-16:], "little", signed=True)


def rust_max_by_key(items, key):
    """Iterator::max_by_key restated literally: a fold that keeps the later
    element unless the earlier one compares Greater."""
    it = iter(items)
    try:
        best = next(it)
    except StopIteration:
        return None
    for x in it:
        if not key(best) > key(x):
            best = x
    return best


def pick(timestamps):
    """timestamps: per candidate an int, or None when absent.
    -> (winner index or -1, stale mask)."""
    present = [(c, t) for c, t in enumerate(timestamps) if t is not None]
    if not present:
        return -1, 0
    top = max(t for _, t in present)
    winner = max(c for c, t in present if t == top)
    stale = 0
    for c, t in enumerate(timestamps):
        if t is None or t < top:
            stale |= 1 << c
    return winner, stale


def answers_of(model, keys):
    """A replica's get_entries answer to keys, from its model:
    (offsets list, records bytes)."""
    _, offsets, records, _, _ = model.expect(keys)
    return offsets, records


def candidate_records(keys, local, sources):
    """Per candidate (sources in order, then local) the list of records, one
    per key, b"" = absent."""
    out = []
    for s in list(sources) + [local]:
        if isinstance(s, gem.Model):
            off, rec = answers_of(s, keys)
        else:
            off, rec = [int(x) for x in s[0]], bytes(s[1])
        assert len(off) == len(keys) + 1
        out.append([rec[off[q]:off[q + 1]] for q in range(len(keys))])
    return out


def expect(keys, local, sources, cap=None):
    """-> (hits as a list of (source, is_tombstone, value_len, stale_mask),
    offsets list, the winners' records of ALL queries as one bytes, rc,
    page). cap None = everything fits; the delivered bytes are
    records[:page["records_len"]]."""
    cands = candidate_records(keys, local, sources)
    hits, offsets, recs = [], [0], []
    for q in range(len(keys)):
        col = [c[q] for c in cands]
        w, stale = pick([ts_of(r) if r else None for r in col])
        rec = col[w] if w >= 0 else b""
        hits.append((w, int(len(rec) == 24), max(len(rec) - 24, 0), stale))
        recs.append(rec)
        offsets.append(offsets[-1] + len(rec))
    rc, page = gem.paging(offsets, offsets[-1] if cap is None else cap)
    return hits, offsets, b"".join(recs), rc, page


def merged(keys, local, sources):
    """Reader.get_merged's answer: None | (data, timestamp, source)."""
    hits, off, rec, _, _ = expect(keys, local, sources)
    return [None if h[0] < 0 else
            (rec[off[q] + 8:off[q + 1] - 16],
             ts_of(rec[off[q]:off[q + 1]]), h[0])
            for q, h in enumerate(hits)]


def replicated(keys, local, sources):
    """Reader.get_replicated's answer: a winning tombstone is None."""
    return [None if m is None or not m[0] else m[0]
            for m in merged(keys, local, sources)]


def self_check():
    gem.self_check()
    # the tie rule against max_by_key's last-maximum behaviour, over every
    # pattern of three timestamps drawn from {absent, 1, 2} plus a 4-way tie
    vals = (None, 1, 2)
    pats = [(a, b, c) for a in vals for b in vals for c in vals]
    pats.append((5, 5, 5, 5))
    for ts in pats:
        present = [(c, t) for c, t in enumerate(ts) if t is not None]
        ref = rust_max_by_key(present, key=lambda ct: ct[1])
        assert pick(ts)[0] == (ref[0] if ref else -1), ts
    assert rust_max_by_key([("a", 1), ("b", 1)], key=lambda x: x[1])[0] == "b"
    assert pick((7, 7, 3, None)) == (1, 0b1100)
    assert pick((None, None)) == (-1, 0)
    # i128 order through the record encoding
    order = [I128_MIN, -1, 0, 1 << 63, 1 << 64, I128_MAX]
    enc = [gem.record_of(gem.Entry(b"k", b"v", t)) for t in order]
    assert [ts_of(r) for r in enc] == order
    for i in range(len(order) - 1):
        assert ts_of(enc[i]) < ts_of(enc[i + 1])
        assert pick((ts_of(enc[i + 1]), ts_of(enc[i])))[0] == 0
        assert pick((ts_of(enc[i]), ts_of(enc[i + 1])))[0] == 1
    # local (last) beats an equal-timestamp remote; nobody is stale
    from dbeel_amd.format import build_run
    run = lambda *e: build_run([gem.Entry(*x) for x in e])
    local = gem.Model([run((b"k", b"local", 9))])
    remote = gem.Model([run((b"k", b"remote", 9))])
    hits, off, rec, rc, _ = expect([b"k"], local, [remote])
    assert hits == [(1, 0, 5, 0)] and rec[8:13] == b"local" and rc == 0
    # a tombstone newer than a value wins, and the value's holder is stale
    dead = gem.Model([run((b"k", b"", 10))])
    hits, off, rec, _, _ = expect([b"k", b"x"], local, [dead])
    assert hits == [(0, 1, 0, 0b10), (-1, 0, 0, 0)] and len(rec) == 24
    assert merged([b"k", b"x"], local, [dead]) == [(b"", 10, 0), None]
    assert replicated([b"k", b"x"], local, [dead]) == [None, None]
    # an older tombstone loses
    assert replicated([b"k"], local, [gem.Model([run((b"k", b"", 8))])]) == \
        [b"local"]
