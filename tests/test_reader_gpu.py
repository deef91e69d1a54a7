"""GPU tests of the resident table reader (engine.Reader,
include/dbeel_gpu.h): batched get with the on-device bloom prefilter, the
prefix-accelerated search and the device value gather.

The host model is the reference read path (LSMTree::get over sstables,
lsm_tree.rs:692-696): the match in the HIGHEST run index wins, regardless
of timestamp; b"" = deleted (tombstone), None = absent.
"""
import os
import struct

import numpy as np
import pytest

from dbeel_amd import lsm
from dbeel_amd.engine import (
    DbeelGpuError,
    Job,
    Reader,
    lookup,
    lookup_raw,
)
from dbeel_amd.format import Entry, build_run, parse_run
from dbeel_amd.genruns import make_runs

pytestmark = pytest.mark.gpu


def _model(runs):
    """key -> (run, data): highest run index wins."""
    model = {}
    for r, (d, i) in enumerate(runs):
        for e in parse_run(bytes(d), bytes(i)):
            model[e.key] = (r, e.data)  # later runs overwrite earlier ones
    return model


def _expect(model, keys):
    return [model[k][1] if k in model else None for k in keys]


def _run(entries):
    entries = sorted(entries, key=lambda e: e.key)
    assert len({e.key for e in entries}) == len(entries)
    return build_run(entries)


def _check_get(reader, model, keys):
    assert reader.get(keys) == _expect(model, keys)


def _run_bloom(run):
    """The filter of one run, built by the engine (every key, tombstones
    included)."""
    with Job([run], device=0) as job:
        job.run(True)
        return job.bloom()


def _zero_bloom(n_bits=4096, k=7, seed=0xDBEE1):
    """Valid header, all-zero bitmap: answers "absent" for every key."""
    return (b"DBLM" + struct.pack("<IIIQQ", 1, k, 0, n_bits, seed)
            + bytes((n_bits + 7) // 8))


class _Parity:
    """test_batched_lookup's inputs, shared (read-only) by the tests that
    need them; the old-path results are computed once."""

    def __init__(self):
        runs = make_runs(4, 3000, 16, 64, overlap_frac=0.5,
                         tombstone_frac=0.15, seed=55)
        self.runs = [(bytes(d), bytes(i)) for d, i in runs]
        self.model = _model(self.runs)
        rng = np.random.default_rng(3)
        present = list(self.model.keys())
        self.present = [present[int(rng.integers(0, len(present)))]
                        for _ in range(500)]
        self.absent = [bytes(rng.integers(0, 256, 16, dtype=np.uint8))
                       for _ in range(100)]
        assert not any(k in self.model for k in self.absent)
        self.queries = self.present + self.absent
        self.blooms = [_run_bloom(r) for r in self.runs]


@pytest.fixture(scope="module")
def parity():
    return _Parity()


def test_parity_with_lookup(parity):
    p = parity
    exp = _expect(p.model, p.queries)
    old_hits = lookup_raw(p.runs, p.queries, device=0)
    with Reader(p.runs, device=0) as rd:
        assert rd.get(p.queries) == exp
        hits, voff, values, stats = rd.get_raw(p.queries)
    assert lookup(p.runs, p.queries, device=0) == exp
    # field for field the old call's records
    assert hits.dtype == old_hits.dtype
    for f in ("run", "is_tombstone", "value_offset", "value_len"):
        assert np.array_equal(hits[f], old_hits[f]), f
    # packed values, in query order
    assert values.tobytes() == b"".join(v or b"" for v in exp)
    assert voff[0] == 0 and voff[-1] == len(values)
    assert np.all(np.diff(voff.astype(np.int64)) >= 0)
    assert np.array_equal(np.diff(voff), hits["value_len"])
    n_found = sum(v is not None for v in exp)
    n_tomb = sum(v == b"" for v in exp)
    assert stats["hits"] == n_found and stats["tombstones"] == n_tomb
    assert stats["bloom_probes"] == 0 and stats["bloom_skips"] == 0


def test_reuse_grows_and_shrinks_scratch(parity):
    p = parity
    rng = np.random.default_rng(11)
    pool = p.queries
    sizes = [0, 1, 63, 64, 65, 257, 5000]
    with Reader(p.runs, device=0) as rd:
        for n in sizes + sizes[::-1]:
            # drawn with replacement: duplicates included
            keys = [pool[int(j)] for j in rng.integers(0, len(pool), n)]
            hits, voff, values, _ = rd.get_raw(keys)
            assert len(hits) == n and len(voff) == n + 1
            _check_get(rd, p.model, keys)


def test_read_path_order():
    """Run index beats timestamp, and a newer tombstone hides the value."""
    old = _run([Entry(b"same-key", b"old-value", 1000),
                Entry(b"deleted", b"still-here", 1000),
                Entry(b"only-old", b"o", 5)])
    new = _run([Entry(b"same-key", b"new-value", 10),  # OLDER timestamp
                Entry(b"deleted", b"", 2000)])
    with Reader([old, new], device=0) as rd:
        got = rd.get([b"same-key", b"deleted", b"only-old", b"nowhere"])
    assert got == [b"new-value", b"", b"o", None]


def test_bloom_real_filters(parity):
    p = parity
    n_runs = len(p.runs)
    exp = _expect(p.model, p.queries)
    with Reader(p.runs, blooms=p.blooms, device=0) as rd:
        hits, voff, values, st = rd.get_raw(p.queries)
        assert st["searches"] + st["bloom_skips"] == st["bloom_probes"]
        with Reader(p.runs, device=0) as plain:
            h0, v0, b0, _ = plain.get_raw(p.queries)
        assert np.array_equal(hits, h0)
        assert np.array_equal(voff, v0) and np.array_equal(values, b0)
        assert rd.get(p.queries) == exp

        # absent keys visit every run; the device decision per (key, run)
        # is dbeel_bloom_contains'
        _, _, _, st = rd.get_raw(p.absent)
        host_skips = sum(not lsm.bloom_contains(b, k)
                         for k in p.absent for b in p.blooms)
        assert st["bloom_probes"] == 100 * n_runs
        assert st["bloom_skips"] == host_skips
        assert st["searches"] + st["bloom_skips"] == st["bloom_probes"]
        assert st["hits"] == 0

        # keys of the newest run, live and tombstoned: one probe each, no
        # false negative, found at once
        newest = parse_run(*p.runs[-1])
        live = [e.key for e in newest if e.data][:150]
        dead = [e.key for e in newest if not e.data][:150]
        assert live and dead
        keys = live + dead
        h, _, _, st = rd.get_raw(keys)
        assert st["bloom_probes"] == len(keys) and st["bloom_skips"] == 0
        assert st["searches"] + st["bloom_skips"] == st["bloom_probes"]
        assert np.all(h["run"] == n_runs - 1)
        assert st["tombstones"] == len(dead)

    # mixed: one run without a filter is always searched
    mixed = list(p.blooms)
    mixed[1] = None
    with Reader(p.runs, blooms=mixed, device=0) as rd:
        assert rd.get(p.queries) == exp
        _, _, _, st = rd.get_raw(p.absent)
        assert st["bloom_probes"] == 100 * (n_runs - 1)
        assert st["searches"] == (st["bloom_probes"] - st["bloom_skips"]
                                  + 100)


def test_bloom_gates_the_search():
    """An all-zero filter on the newest run hides it completely: the
    filter, not the search, decides whether a run is visited."""
    older = _run([Entry(b"both-%03d" % i, b"older-%d" % i, 10)
                  for i in range(50)])
    newest = _run([Entry(b"both-%03d" % i, b"newest-%d" % i, 20)
                   for i in range(50)]
                  + [Entry(b"only-%03d" % i, b"x" * (i + 1), 20)
                     for i in range(50)])
    both = [b"both-%03d" % i for i in range(50)]
    only = [b"only-%03d" % i for i in range(50)]
    with Reader([older, newest], blooms=[None, _zero_bloom()],
                device=0) as rd:
        hits, _, _, st = rd.get_raw(only + both)
        assert rd.get(only) == [None] * 50
        assert rd.get(both) == [b"older-%d" % i for i in range(50)]
    assert st["bloom_probes"] == 100 and st["bloom_skips"] == 100
    assert st["searches"] == 100  # run 0 only
    # sanity: without the filter the newest run answers
    with Reader([older, newest], device=0) as rd:
        assert rd.get(both[:3] + only[:1]) == [
            b"newest-0", b"newest-1", b"newest-2", b"x"]


def test_shared_prefixes():
    """Keys sharing their first 8 bytes (one equal-prefix range spanning a
    whole run), a family tied through 40 bytes with strict prefixes, and
    keys shorter than 8 bytes whose trailing zeros collide with the prefix
    array's zero padding."""
    stem = b"PREFIX__"
    tie = stem + bytes(range(100, 132))  # 40 bytes
    assert len(tie) == 40
    family = [tie[:n] for n in range(8, 41)]              # strict prefixes
    family += [tie + bytes([7] * n) for n in range(1, 9)]  # 41..48 bytes
    family += [tie[:39] + b"\x00", tie[:20] + b"\x00", tie + b"\x00"]
    shorts = [b"ab", b"ab\x00", b"ab\x00\x00", b"", b"\x00", b"ab\x01"]
    runs = []
    for r in range(3):
        ents = {}
        for i in range(2500):
            # neighbouring counters; every third key is in two runs
            k = stem + struct.pack(">I", 3 * i + (r if i % 3 else 0))
            ents[k] = Entry(k, b"r%d-%d" % (r, i), 100 + r)
        for j, k in enumerate(family):
            if (j + r) % 3 != 0:
                ents[k] = Entry(k, b"" if j % 5 == 0 else b"fam%d-%d" % (r, j),
                                50)
        for j, k in enumerate(shorts):
            if (j + r) % 2 == 0:
                ents[k] = Entry(k, b"short%d-%d" % (r, j), 60)
        runs.append(_run(list(ents.values())))
    model = _model(runs)
    queries = []
    for k in model:
        queries += [k, k + b"\x00"]
        if k:
            queries.append(k[:-1])
            if k[-1] < 255:
                queries.append(k[:-1] + bytes([k[-1] + 1]))
            if k[-1] > 0:
                queries.append(k[:-1] + bytes([k[-1] - 1]))
    with Reader(runs, device=0) as rd:
        _check_get(rd, model, queries)
    assert lookup(runs, shorts, device=0) == _expect(model, shorts)


GATHER_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 1023, 4096, 70_000]


def test_gather_edges():
    """Every value length at the first and the last entry of a run and at
    the last entry of the last run (the end of the slab's data), next to
    empty and 1-byte neighbours."""
    rng = np.random.default_rng(77)

    def val(n):
        return bytes(rng.integers(1, 256, n, dtype=np.uint8))

    # all lengths back to back in one run, twice, in opposite orders
    asc = _run([Entry(b"asc-%02d" % j, val(n), 1)
                for j, n in enumerate(GATHER_LENS) if n])
    desc = _run([Entry(b"dsc-%02d" % j, val(n), 1)
                 for j, n in enumerate(reversed(GATHER_LENS)) if n])
    model = _model([asc, desc])
    keys = sorted(model) + sorted(model, reverse=True)
    with Reader([asc, desc], device=0) as rd:
        _check_get(rd, model, keys)

    for n in GATHER_LENS:
        first = _run([Entry(b"a-first", val(n), 1),
                      Entry(b"m-mid", b"x", 1),
                      Entry(b"z-last", val(n), 1)])
        last = _run([Entry(b"b-tomb", b"", 2),
                     Entry(b"y-slab-end", val(n), 2)])
        model = _model([first, last])
        keys = [b"a-first", b"b-tomb", b"z-last", b"y-slab-end", b"m-mid",
                b"absent", b"y-slab-end", b"a-first"]
        with Reader([first, last], device=0) as rd:
            hits, voff, values, _ = rd.get_raw(keys)
            exp = _expect(model, keys)
            assert values.tobytes() == b"".join(v or b"" for v in exp), n
            assert rd.get(keys) == exp, n


def test_shapes_empty_and_single_entry_runs():
    a = _run([Entry(b"k%03d" % i, b"a%d" % i, 1) for i in range(100)])
    empty = (b"", b"")
    c = _run([Entry(b"k%03d" % i, b"c%d" % i, 1) for i in range(50, 150)])
    runs = [a, empty, c, empty]
    model = _model(runs)
    keys = sorted(model) + [b"k", b"k999", b""]
    with Reader(runs, device=0) as rd:
        _check_get(rd, model, keys)

    singles = [_run([Entry(b"s%d" % (r % 3), b"v%d" % r, r)])
               for r in range(5)]
    model = _model(singles)
    with Reader(singles, device=0) as rd:
        _check_get(rd, model, [b"s0", b"s1", b"s2", b"s3", b"s", b"s00"])


def test_shapes_64_runs_identical_keys():
    runs = [_run([Entry(k, b"" if (r + j) % 7 == 0 else b"%d-%d" % (r, j),
                        1000 - r)
                  for j, k in enumerate((b"alpha", b"beta", b"gamma"))])
            for r in range(64)]
    model = _model(runs)
    with Reader(runs, device=0) as rd:
        _check_get(rd, model, [b"alpha", b"beta", b"gamma", b"delta"])
        hits, _, _, _ = rd.get_raw([b"alpha", b"beta", b"gamma"])
    assert np.all(hits["run"] == 63)


def _adversarial_cases():
    from adversarial import all_cases

    return all_cases()


@pytest.mark.parametrize("case", _adversarial_cases(), ids=lambda c: c[0])
def test_adversarial_cases(case):
    _, runs = case
    model = _model(runs)
    keys = list(model)
    with Reader(runs, device=0) as rd:
        _check_get(rd, model, keys)


def _corrupt_runs():
    good = _run([Entry(b"key-%03d" % i, b"value-%d" % i, 1)
                 for i in range(200)])
    data, index = good
    # an index record pointing past data_len
    recs = bytearray(index)
    struct.pack_into("<Q", recs, 16 * 120, len(data) - 8)
    past = (data, bytes(recs))
    far = bytearray(index)
    struct.pack_into("<Q", far, 16 * 199, 2**64 - 16)  # off+size wraps
    wrap = (data, bytes(far))
    # a zeroed data region
    zeroed = bytearray(data)
    zeroed[1000:2000] = bytes(1000)
    zero = (bytes(zeroed), index)
    # two swapped entries: well-formed, but not ascending
    ents = parse_run(data, index)
    ents[70], ents[71] = ents[71], ents[70]
    unsorted = build_run(ents)
    dup = build_run(parse_run(data, index)[:10]
                    + parse_run(data, index)[9:20])  # equal neighbours
    return [("past_data_len", past), ("offset_wraps", wrap),
            ("zeroed_data", zero), ("swapped_entries", unsorted),
            ("duplicate_key", dup)]


@pytest.mark.parametrize("case", _corrupt_runs(), ids=lambda c: c[0])
def test_corrupt_inputs_rejected(case):
    good = _run([Entry(b"a", b"b", 1)])
    with pytest.raises(DbeelGpuError) as ei:
        Reader([good, case[1], good], device=0)
    assert ei.value.code == 2  # CORRUPT


def test_footprint(parity):
    p = parity
    input_bytes = sum(len(d) + len(i) for d, i in p.runs)
    entries = sum(len(i) // 16 for _, i in p.runs)
    bloom_bytes = sum(len(b) for b in p.blooms)
    with Reader(p.runs, blooms=p.blooms, device=0) as rd:
        tb = rd.table_bytes
        rd.get(p.queries)
        assert rd.table_bytes == tb  # scratch is not table
    assert tb >= input_bytes + 8 * entries
    assert tb <= input_bytes + 8 * entries + bloom_bytes + (1 << 20)


def test_directory_reader(tmp_path):
    d = str(tmp_path)
    runs = make_runs(3, 2000, 16, 48, overlap_frac=0.5, tombstone_frac=0.2,
                     seed=91)
    for idx, (data, index) in zip((0, 2, 4), runs):
        lsm.write_run_files(d, idx, bytes(data), bytes(index))
    lsm.compact(d, [0, 2], 1, keep_tombstones=True, device=0,
                bloom_min_size=1)
    assert os.path.exists(f"{d}/{1:020d}.bloom")
    before = sorted(os.listdir(d))

    rd, indices = lsm.open_reader(d, device=0)
    with rd:
        assert indices == [1, 4]
        assert indices == sorted(indices)
        live = [lsm.read_run_files(d, i) for i in indices]
        model = _model(live)
        rng = np.random.default_rng(5)
        keys = list(model)[::3] + [
            bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            for _ in range(100)]
        _check_get(rd, model, keys)
        hits, _, _, st = rd.get_raw(keys)
        # only sstable 1 has a filter
        assert 0 < st["bloom_probes"] <= len(keys)
        assert {indices[r] for r in hits["run"] if r >= 0} <= {1, 4}
    assert sorted(os.listdir(d)) == before  # opening never mutates

    # a leftover journal: refuse, with the IO code
    open(f"{d}/{7:020d}.compact_action", "wb").write(b"\0" * 16)
    with pytest.raises(DbeelGpuError) as ei:
        lsm.open_reader(d, device=0)
    assert ei.value.code == 7
