"""The three users of the engine's shared in-run search agree with each
other and with the Python model on one tiny table set: k_lookup
(engine.lookup), k_reader_search (Reader.get) and k_reader_scan_bounds
(Reader.scan's key bounds), with dbeel_gpu_scan (engine.scan, a plain
per-entry key compare) as the independent yardstick for the bounds.

The tables hold what the search has to get right beyond the 8-byte prefix
bisection: keys that differ only in zero padding, keys that share all 8
prefix bytes, every key length around the prefix width, an empty and a
single-entry run, and one key present in every non-empty run.
"""
import pytest

from dbeel_amd.engine import Reader, lookup, scan
from dbeel_amd.format import Entry, build_run
from pymm3 import scan_model

pytestmark = pytest.mark.gpu

SHARED = b"shared-key"


def _run(pairs, ts):
    return build_run([Entry(k, v, ts) for k, v in sorted(pairs)])


def _runs():
    padding = [(b"ab", b"p0"), (b"ab\0", b"p1"), (b"ab\0\0", b"p2")]
    same_prefix = [(b"prefix88" + bytes([c]), b"s%d" % c)
                   for c in (0, 1, 7, 8, 64, 128, 254, 255)]
    lengths = [(bytes(range(65, 65 + n)), b"len%d" % n) for n in range(18)]
    return [
        _run(padding + [(SHARED, b"oldest")], 1),
        _run(same_prefix + [(SHARED, b"older")], 2),
        _run(lengths + [(SHARED, b"old")], 3),
        (b"", b""),
        _run([(SHARED, b"")], 5),  # the newest copy is a tombstone
    ]


def _queries(keys):
    qs = set(keys)
    for k in keys:
        qs.add(k + b"\0")
        qs.add(k + b"\xff")
        if k and k[-1] > 0:
            qs.add(k[:-1] + bytes([k[-1] - 1]))
        if k and k[-1] < 255:
            qs.add(k[:-1] + bytes([k[-1] + 1]))
    return sorted(qs)


class _Shared:
    def __init__(self):
        from dbeel_amd.format import parse_run

        self.runs = _runs()
        self.newest = {}  # key -> value in the highest run that holds it
        for d, i in self.runs:
            for e in parse_run(d, i):
                self.newest[e.key] = e.data
        self.queries = _queries(sorted(self.newest))
        self.reader = Reader(self.runs, device=0)


@pytest.fixture(scope="module")
def shared():
    s = _Shared()
    yield s
    s.reader.close()


def test_tables_hold_the_cases(shared):
    s = shared
    total = sum(len(i) // 16 for _, i in s.runs)
    assert total <= 300
    assert [len(i) // 16 for _, i in s.runs][3:] == [0, 1]
    assert {b"ab", b"ab\0", b"ab\0\0"} <= set(s.newest)
    assert sum(k.startswith(b"prefix88") and len(k) == 9
               for k in s.newest) == 8
    assert {len(k) for k in s.newest} >= set(range(18))
    # every query class is present: hits, and misses on either side
    assert any(q not in s.newest for q in s.queries)
    assert all(k in s.queries for k in s.newest)


def test_lookup_and_get_agree(shared):
    s = shared
    model = [s.newest.get(q) for q in s.queries]
    assert model[s.queries.index(SHARED)] == b""  # tombstone, not absent
    assert model[s.queries.index(b"")] == b"len0"
    assert lookup(s.runs, s.queries, device=0) == model
    assert s.reader.get(s.queries) == model


@pytest.mark.parametrize("bound", ["start_key", "end_key"])
def test_scan_bounds_agree(shared, bound):
    s = shared
    for q in s.queries:
        kw = {bound: q}
        want = scan_model(s.runs, **kw)
        assert scan(s.runs, device=0, **kw) == want, (bound, q)
        assert s.reader.scan(**kw) == want, (bound, q)
