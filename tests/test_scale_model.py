"""CPU self-tests of the vectorised models (scale_model, bloom_model) that
test_grid_cap_gpu.py compares the engine with: each agrees with the slow
per-entry model it restates, the sizes lie past the engine's grid cap, and
every comparison helper sees damage confined to the items that only a later
trip of a grid-stride loop reaches.
"""
import os

import numpy as np
import pytest

import batch_model
import bloom_model
import get_entries_model as gem
import pymm3
import scale_model as sm
import snapshot_model
from conftest import REPO_ROOT
from dbeel_amd import lsm
from dbeel_amd.engine import HIT_DTYPE, grid_for
from dbeel_amd.format import Entry, build_run, parse_run


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(os.path.join(REPO_ROOT, "dbeel_amd",
                                       "libdbeel_gpu.so")):
        import __graft_entry__

        __graft_entry__.build()


@pytest.fixture(scope="module")
def small():
    """Two small tables of the grid-cap tests' shape, with their slow
    models."""
    A, B, absent = sm.make_pair(3000, seed=5)
    runs = [sm.encode_run(A), sm.encode_run(B)]
    runs_b = [(d.tobytes(), i.tobytes()) for d, i in runs]
    return A, B, absent, runs, runs_b


# ------------------------------------------------------------------ sizes
def test_sizes_exceed_the_cap():
    T, W, N_T, N_W = sm.sizes(grid_for)
    assert grid_for(T, 256) * 256 >= T          # one trip covers T items
    assert grid_for(T + 1, 256) * 256 < T + 1   # and not one more
    assert grid_for(W * 64, 256) * 256 >= W * 64
    assert grid_for((W + 1) * 64, 256) * 256 < (W + 1) * 64
    assert N_T == T + 2 * 256 + 37 and N_T > T + 256
    assert (N_T - T) % 256 != 0                 # ends inside a block
    assert N_W == 2 * W + 5 and N_W > 2 * W     # a third trip


def test_grid_for_never_zero_and_monotone():
    T, W, N_T, _ = sm.sizes(grid_for)
    ns = sorted(set([0, 1, 2, 255, 256, 257, T - 1, T, T + 1, N_T, 2 * T,
                     1 << 31, 1 << 40]
                    + list(range(0, 4 * T, 4099))))
    for block in (64, 256, 512, 1024):
        grids = [grid_for(n, block) for n in ns]
        assert min(grids) >= 1
        assert grids == sorted(grids)
        assert all(g * block >= min(n, g * block) for g, n in zip(grids, ns))
    assert grid_for(1, 256) == 1 and grid_for(257, 256) == 2


# ------------------------------------------------------------- the models
def test_make_pair_shape(small):
    A, B, absent, runs, _ = small
    n = len(A)
    assert len(B) == n
    for e in (A, B):
        ks = sm.skeys(e.keys)
        assert np.all(ks[1:] > ks[:-1])         # sorted, unique
        assert 0.05 < np.mean(e.vlen == 0) < 0.15
        assert np.all(e.vals != 0)
        p = np.ascontiguousarray(e.keys[:, :8]).view(">u8").reshape(-1)
        tied = np.zeros(n, dtype=bool)
        tied[1:] |= p[1:] == p[:-1]
        tied[:-1] |= p[1:] == p[:-1]
        assert tied.mean() > 0.5    # share their prefix with a neighbour
    both = np.isin(sm.skeys(B.keys), sm.skeys(A.keys)).mean()
    assert 0.45 < both < 0.55
    assert not np.isin(sm.skeys(absent), sm.skeys(A.keys)).any()
    assert not np.isin(sm.skeys(absent), sm.skeys(B.keys)).any()


def test_encode_run_and_table_roundtrip(small):
    A, _, _, runs, runs_b = small
    ents = parse_run(*runs_b[0])
    assert build_run(ents) == runs_b[0]
    w = A.writes()
    assert [(e.key, e.data, e.timestamp) for e in ents] == w
    t = sm.Table(*runs[0], 16)
    back = t.entries()
    assert np.array_equal(back.keys, A.keys)
    assert np.array_equal(back.vlen, A.vlen)
    assert np.array_equal(back.ts, A.ts)
    assert np.array_equal(back.vals[A.vlen != 0], A.vals[A.vlen != 0])
    # negative and wide timestamps go through the high half
    e = A.take(np.arange(50))
    hi = np.array([-1, 0, 1, -(1 << 63), (1 << 63) - 1] * 10, dtype=np.int64)
    e.ts = sm.ts_bytes(np.arange(50, dtype=np.uint64) * 977, hi)
    d, x = sm.encode_run(e)
    assert (d.tobytes(), x.tobytes()) == build_run(
        Entry(k, v, t) for k, v, t in e.writes())
    assert any(t < 0 for _, _, t in e.writes())


def test_read_model_agrees_with_parse_run(small):
    A, B, absent, runs, runs_b = small
    slow = gem.Model(runs_b)
    fast = sm.ReadModel(runs, 16)
    rng = np.random.default_rng(1)
    q = np.concatenate([A.keys, B.keys, absent, A.keys[:100]])
    q = q[rng.permutation(len(q))]
    keys = sm.key_list(q)
    hits, offsets, records, _, _ = slow.expect(keys)
    assert sm.mismatch_fields(fast.hits(q),
                              gem.hits_array(hits, HIT_DTYPE)) is None
    roff, rec = fast.records(q)
    assert roff.tolist() == offsets and rec.tobytes() == records
    voff, vals = fast.values(q)
    exp_vals = [slow.where[k][2].data if k in slow.where else b""
                for k in keys]
    assert vals.tobytes() == b"".join(exp_vals)
    assert voff.tolist() == np.cumsum([0] + [len(v) for v in exp_vals]
                                      ).tolist()
    found, ts = fast.timestamps(q)
    for i in range(0, len(keys), 37):
        k = keys[i]
        assert bool(found[i]) == (k in slow.where)
        if found[i]:
            assert int.from_bytes(ts[i].tobytes(), "little", signed=True) \
                == slow.where[k][2].timestamp
    # the highest run wins: every shared key answers from run 1
    shared = np.isin(sm.skeys(A.keys), sm.skeys(B.keys))
    assert shared.any() and np.all(fast.hits(A.keys[shared])["run"] == 1)
    # a memtable run is consulted first and reported at n_runs
    mem = sm.ReadModel(runs[:1], 16, mem_run=runs[1])
    assert np.all(mem.hits(B.keys)["run"] == 1) and mem.n_runs == 1
    # paging on an offset array
    for cap in (0, 23, 24, 1000, int(roff[-1]) - 1, int(roff[-1])):
        assert sm.paging(roff, cap) == gem.paging(offsets, cap)[1], cap


def test_flush_model_agrees_with_batch_model(small):
    A, B, _, _, _ = small
    rng = np.random.default_rng(2)
    arr = sm.Entries.concat([A, B, A.take(np.arange(0, len(A), 5)),
                             B.take(np.arange(0, len(B), 7))])
    arr = arr.take(rng.permutation(len(arr)))
    arr.ts = sm.ts_bytes(rng.integers(0, 1 << 60, len(arr), dtype=np.uint64))
    writes = arr.writes()
    surv, (d, x) = sm.flush_model(arr)
    assert (d.tobytes(), x.tobytes()) == batch_model.flush_run(writes)
    assert len(surv) < len(arr)
    assert sm.prefix_tied(arr.keys) == batch_model.prefix_tied(writes)
    assert 0 < sm.prefix_tied(A.keys) < len(A)


def test_murmur3_agrees_with_pymm3_and_published_vectors():
    from test_scan_host import VECTORS

    for key, seed, want in VECTORS:
        m = np.frombuffer(key, dtype=np.uint8).reshape(1, len(key))
        assert int(sm.murmur3_32(m, seed)[0]) == want, key
    rng = np.random.default_rng(3)
    for K in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33):
        m = rng.integers(0, 256, size=(200, K), dtype=np.uint8)
        got = sm.murmur3_32(m)
        assert got.dtype == np.uint32
        assert got.tolist() == [pymm3.murmur3_32(k) for k in sm.key_list(m)]
    h = np.array([0, 5, 10, 2**32 - 1], dtype=np.uint32)
    for s, e in ((5, 10), (10, 5), (0, 0), (7, 7), (0, 2**32 - 1)):
        assert sm.between(h, s, e).tolist() == [
            pymm3.between_cmp(int(v), s, e) for v in h]


def test_scan_model_agrees_with_snapshot_model(small):
    A, B, _, runs, runs_b = small
    tabs = [sm.Table(d, i, 16) for d, i in runs]
    ks = sm.skeys(A.keys)
    start, end = bytes(A.keys[len(A) // 10]), bytes(A.keys[-len(A) // 10])
    ranges = [(0x10000000, 0x50000000), (0xF0000000, 0x20000000)]
    narrow = [(0x10000000, 0x50000000), (0x90000000, 0xA0000000)]
    for kw in (dict(), dict(start_key=start, end_key=end),
               dict(hash_ranges=ranges), dict(hash_ranges=narrow),
               dict(start_key=start, end_key=end, hash_ranges=narrow)):
        for newest in (False, True):
            want = snapshot_model.snapshot_model(runs_b, newest_only=newest,
                                                 **kw)
            r = kw.get("hash_ranges")
            d, x, rid, shadowed = sm.scan_model(
                tabs, kw.get("start_key"), kw.get("end_key"), r, newest)
            assert (d.tobytes(), x.tobytes(), len(x) // 16) == want, kw
            if r:
                assert rid.tolist() == snapshot_model.first_range_ids(want, r)
            if newest:
                assert shadowed == snapshot_model.shadowed_count(runs_b, **kw)
                assert shadowed > 0
    assert len(ks)


def test_merge_expect_agrees_with_merge_model(small):
    import merge_model
    from dbeel_amd.engine import MERGE_HIT_DTYPE

    A, B, absent, runs, runs_b = small
    rng = np.random.default_rng(8)
    C = sm.make_remote(rng, B, 2500, 1 << 42)
    D = sm.make_remote(rng, A, 2500, 1 << 41)
    # i128 order: a few wide and negative timestamps on the remote side
    D.ts[::11] = sm.ts_bytes(D.ts[::11, :8].copy().view("<u8").reshape(-1),
                             np.resize(np.array([-1, 1, -(1 << 62)]),
                                       len(D.ts[::11])))
    rc, rd_ = sm.encode_run(C), sm.encode_run(D)
    q = np.concatenate([A.keys, B.keys, C.keys, D.keys, absent])
    q = q[rng.permutation(len(q))]
    keys = sm.key_list(q)
    local = gem.Model(runs_b)
    src0 = gem.Model([(rc[0].tobytes(), rc[1].tobytes())])
    off1, rec1 = merge_model.answers_of(
        gem.Model([(rd_[0].tobytes(), rd_[1].tobytes())]), keys)
    hits, offsets, records, _, _ = merge_model.expect(
        keys, local, [src0, (off1, rec1)])
    fast = [sm.ReadModel([rc], 16).records(q),
            sm.ReadModel([rd_], 16).records(q),
            sm.ReadModel(runs, 16).records(q)]
    assert fast[1][0].tolist() == off1 and fast[1][1].tobytes() == rec1
    got_hits, got_off, got_rec = sm.merge_expect(fast)
    assert sm.mismatch_fields(
        got_hits, gem.hits_array(hits, MERGE_HIT_DTYPE)) is None
    assert got_off.tolist() == offsets and got_rec.tobytes() == records
    # every outcome occurs: each candidate wins, ties, tombstones both ways
    assert set(got_hits["source"].tolist()) == {-1, 0, 1, 2}
    assert got_hits["is_tombstone"].sum() > 0
    assert len(set(got_hits["stale_mask"].tolist())) >= 6


# ------------------------------------------------------------- the filter
def test_bloom_model_against_the_c_checker(small):
    A, _, absent, _, _ = small
    f = bloom_model.build(A.keys)
    n_bits = bloom_model.n_bits_for(len(A))
    assert len(f) == 32 + (n_bits + 7) // 8
    assert f[:32] == bloom_model.header(n_bits)
    assert n_bits == int(9.585 * len(A)) + 64
    for k in sm.key_list(A.keys):
        assert lsm.bloom_contains(f, k)
    assert bloom_model.maybe(f, A.keys).all()
    rng = np.random.default_rng(4)
    other = rng.integers(0, 256, size=(10_000, 16), dtype=np.uint8)
    assert not np.isin(sm.skeys(other), sm.skeys(A.keys)).any()
    predicted = bloom_model.maybe(f, other)
    got = [lsm.bloom_contains(f, k) for k in sm.key_list(other)]
    assert got == predicted.tolist()
    assert 0 < predicted.sum() < 500  # about 1 % false positives
    # other key widths, and a filter sized for more keys than it holds
    for K in (1, 7, 33):
        m = np.unique(rng.integers(0, 256, size=(300, K), dtype=np.uint8),
                      axis=0)
        g = bloom_model.build(m, n=1000)
        assert all(lsm.bloom_contains(g, k) for k in sm.key_list(m))
        probe = rng.integers(0, 256, size=(500, K), dtype=np.uint8)
        assert [lsm.bloom_contains(g, k) for k in sm.key_list(probe)] \
            == bloom_model.maybe(g, probe).tolist()
    # the empty filter is sized as for one key and holds no bit
    e = bloom_model.build(np.zeros((0, 16), dtype=np.uint8))
    assert len(e) == 32 + (73 + 7) // 8 and not any(e[32:])


# ------------------------------------------- the comparisons see the tail
@pytest.fixture(scope="module")
def tail():
    """A correct expected answer of N_T items, and where its tail begins."""
    T, W, N_T, N_W = sm.sizes(grid_for)
    rng = np.random.default_rng(6)
    hits = np.zeros(N_T, dtype=HIT_DTYPE)
    hits["run"] = rng.integers(0, 2, N_T)
    hits["value_offset"] = rng.integers(1, 1 << 30, N_T)
    hits["value_len"] = 8
    offsets = sm.offsets_of(hits["value_len"])
    values = rng.integers(1, 256, size=8 * N_T, dtype=np.uint8)
    return T, W, N_T, N_W, hits, offsets, values


def test_mismatch_fields_sees_the_tail(tail):
    T, W, N_T, _, hits, offsets, _ = tail
    assert sm.mismatch_fields(hits.copy(), hits) is None
    assert sm.mismatch_fields(offsets.copy(), offsets) is None
    for at in (T, T + 256, N_T - 1, W):
        for f in HIT_DTYPE.names:
            bad = hits.copy()
            bad[f][at] = 0 if hits[f][at] else 1
            m = sm.mismatch_fields(bad, hits)
            assert m is not None and f in m and f"first at {at}" in m
        bad = hits.copy()
        bad[at:] = np.zeros(1, dtype=HIT_DTYPE)   # a tail never written
        assert sm.mismatch_fields(bad, hits) is not None
        shifted = offsets.copy()
        shifted[at] += 1                          # one offset off by one
        assert f"first at {at}" in sm.mismatch_fields(shifted, offsets)
    assert sm.mismatch_fields(hits[:-1], hits) is not None
    with pytest.raises(AssertionError):
        bad = hits.copy()
        bad["run"][N_T - 1] ^= 1
        sm.assert_fields(bad, hits, "hits")


def test_mismatch_bytes_sees_the_tail(tail):
    T, W, N_T, _, _, _, values = tail
    assert sm.mismatch_bytes(values.copy(), values) is None
    assert sm.mismatch_bytes(values.tobytes(), values) is None
    for item in (T, N_T - 1, W):
        bad = values.copy()
        bad[8 * item:] = 0                        # zeroed from item on
        assert f"first at {8 * item}" in sm.mismatch_bytes(bad, values)
        bad = values.copy()
        bad[8 * item + 7] ^= 0x80                 # one bit of one value
        assert f"first at {8 * item + 7}" in sm.mismatch_bytes(bad, values)
    assert sm.mismatch_bytes(values[:-1], values) is not None
    with pytest.raises(AssertionError):
        sm.assert_bytes(values[:-1], values, "values")


def test_mismatch_bytes_sees_one_filter_bit(tail):
    T, _, N_T, _, _, _, _ = tail
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 256, size=(N_T, 16), dtype=np.uint8)
    good = bloom_model.build(keys)
    n_bits = bloom_model.n_bits_for(N_T)
    # the bits of a key that only the second trip reaches
    bits = bloom_model.bit_positions(keys[T + 300:T + 301], n_bits)[0]
    bitmap = np.frombuffer(good, dtype=np.uint8, offset=32)
    b = int(bits[3])
    assert bitmap[b >> 3] >> (b & 7) & 1
    cleared = bytearray(good)
    cleared[32 + (b >> 3)] &= ~(1 << (b & 7)) & 0xFF
    assert sm.mismatch_bytes(bytes(cleared), good) is not None
    zero = int(np.flatnonzero(np.unpackbits(bitmap, bitorder="little")[
        :n_bits] == 0)[-1])                       # an unset bit, far in
    extra = bytearray(good)
    extra[32 + (zero >> 3)] |= 1 << (zero & 7)
    m = sm.mismatch_bytes(bytes(extra), good)
    assert m is not None and f"first at {32 + (zero >> 3)}" in m
    # the behavioural check alone would have let the extra bit through
    assert bloom_model.maybe(bytes(extra), keys[T:]).all()


def test_mismatch_guard_sees_a_write_past_the_end(tail):
    _, _, N_T, _, _, _, values = tail
    buf = np.full(values.size + 64, 0xA5, dtype=np.uint8)
    buf[:values.size] = values
    assert sm.mismatch_guard(buf, values.size, 0xA5) is None
    for at in (values.size, values.size + 63):
        bad = buf.copy()
        bad[at] = 0
        assert f"first at {at}" in sm.mismatch_guard(bad, values.size, 0xA5)
    with pytest.raises(AssertionError):
        bad = buf.copy()
        bad[-1] = 0
        sm.assert_guard(bad, values.size, 0xA5, "values")
