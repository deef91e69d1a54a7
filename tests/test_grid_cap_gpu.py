"""GPU tests past the launch-grid cap.

Every launch outside the copy and co-rank kernels takes its grid from
pick_grid (exported as dbeel_gpu_grid_for), which caps it; past the cap a
grid-stride loop covers the rest. A thread-per-item kernel takes a second
trip round that loop from T items on, a wave-per-item kernel from W items
on. The reader, write, memtable, scan, encode and filter kernels are driven
here at N_T = T + 2 * 256 + 37 items (a second trip that ends inside a
block) and N_W = 2 * W + 5 (a third trip of the wave kernels), T and W read
from the engine, and every output is compared exactly — every field of
every item, every byte — with the vectorised host models of scale_model.py
and bloom_model.py, which test_scale_model.py ties to the slow per-entry
models. The device-built "DBLM" filters are compared byte for byte.

The rule of every case: the items only a later trip reaches have expected
outputs that differ from zero and from the guard byte (present keys with
values, survivors, selected entries), asserted on the expectation before the
engine is called; caller-owned buffers are pre-filled with a guard byte and
must still hold it past the reported lengths.
"""
import ctypes
from functools import cached_property

import numpy as np
import pytest

import batch_model
import bloom_model
import get_entries_model as gem
import migrate_model
import scale_model as sm
from dbeel_amd import engine
from dbeel_amd.engine import (
    HIT_DTYPE,
    MERGE_HIT_DTYPE,
    CompactResult,
    Job,
    Reader,
    grid_for,
    lookup_raw,
)
from dbeel_amd.format import INDEX_DTYPE, Entry, build_run

pytestmark = pytest.mark.gpu

K = 16
GUARD = 0xA5
HASH_3 = [(0, 0x55555555), (0x55555555, 0xAAAAAAAA), (0xAAAAAAAA, 0xFFFFFFFF)]
TINY = build_run([Entry(b"\xff" * 40, b"base", 0)])


def guarded(n, dtype=np.uint8):
    """n elements of dtype, every byte the guard."""
    return np.full(int(n) * np.dtype(dtype).itemsize, GUARD,
                   dtype=np.uint8).view(dtype)


class World:
    """Everything the cases share, built once and never changed: the two
    tables, their read model, the queries and the expectations."""

    def __init__(self):
        self.T, self.W, self.N_T, self.N_W = sm.sizes(grid_for)
        self.A, self.B, self.absent = sm.make_pair(self.N_T, seed=0xCA9)
        self.runs = [sm.encode_run(self.A), sm.encode_run(self.B)]
        self.model = sm.ReadModel(self.runs, K)

    # -- queries: every kind in the head, present values in the tail
    @cached_property
    def q(self):
        rng = np.random.default_rng(11)
        pool = np.concatenate([self.A.keys, self.B.keys, self.absent])
        n_head = self.T - 1000
        head = pool[rng.integers(0, len(pool), n_head)]  # with replacement
        live = np.flatnonzero(self.model.vlen != 0)
        tail = self.model.keys[live[rng.integers(
            0, live.size, self.N_T - n_head)]].view(np.uint8).reshape(-1, K)
        return np.concatenate([head, tail])

    @cached_property
    def q_list(self):
        return sm.key_list(self.q)

    @cached_property
    def hits(self):
        h = self.model.hits(self.q)
        T, W = self.T, self.W
        assert len(h) == self.N_T > T
        # every kind of answer occurs ...
        in_a = np.isin(sm.skeys(self.q), sm.skeys(self.A.keys))
        assert (h["run"] == -1).sum() > 1000
        assert ((h["run"] == 0) & (h["is_tombstone"] == 0)).sum() > 1000
        assert ((h["run"] == 1) & ~in_a).sum() > 1000       # B only
        assert ((h["run"] == 1) & in_a).sum() > 1000        # both: B wins
        assert h["is_tombstone"].sum() > 1000
        assert np.unique(sm.skeys(self.q)).size < self.N_T  # duplicates
        # ... and what only a later trip reaches is a value, from both runs
        assert np.all(h["value_len"][T:] == 8) and np.all(h["run"][T:] >= 0)
        assert {0, 1} <= set(h["run"][T:].tolist())
        assert np.all(h["value_offset"][T:] > 0)
        assert (h["value_len"][W:] > 0).mean() > 0.5
        return h

    @cached_property
    def values(self):
        return self.model.values(self.q)

    @cached_property
    def records(self):
        return self.model.records(self.q)

    @cached_property
    def blooms(self):
        return [bloom_model.build(self.A.keys), bloom_model.build(self.B.keys)]

    @cached_property
    def tabs(self):
        return self.model.tabs

    # -- the write batch: shuffled, a fifth of the keys written 2..4 times
    @cached_property
    def batch(self):
        rng = np.random.default_rng(12)
        u = int(self.N_T / 1.4)
        keys = sm.make_keys(rng, u, max(1, u // 8))
        lone = rng.random(u) < 0.8   # most get a prefix nobody else has
        keys[lone, :8] = rng.integers(0, 256, size=(int(lone.sum()), 8),
                                      dtype=np.uint8)
        rep = rng.permutation(u)[:u // 5]
        extra = np.repeat(rep, rng.integers(1, 4, rep.size))
        extra = extra[:self.N_T - u]
        pad = self.N_T - u - extra.size
        idx = np.concatenate([np.arange(u), extra, rep[:pad]])
        idx = idx[rng.permutation(idx.size)]  # repeats land far apart
        e = sm.make_entries(rng, keys[idx], 0.10, 0)
        e.ts = sm.ts_bytes(rng.integers(0, 1 << 63, len(e), dtype=np.uint64),
                           rng.integers(-2, 3, len(e)))
        assert len(e) == self.N_T
        return e

    @cached_property
    def batch_writes(self):
        return self.batch.writes()

    @cached_property
    def batch_expect(self):
        surv, (d, x) = sm.flush_model(self.batch)
        tied = sm.prefix_tied(self.batch.keys)
        assert 0.4 < tied / self.N_T < 0.7 and tied > self.T // 2
        assert len(surv) < 0.8 * self.N_T
        # the arrivals of the second trip matter: some of them survive
        last = sm.last_arrivals(self.batch.keys)
        assert (last >= self.T).sum() > 100
        assert np.any(surv.vlen[-1000:] != 0) and len(surv) > self.W
        return surv, d, x, tied

    # -- the memtable's arrivals: N_T distinct keys, then N_W half new
    @cached_property
    def mem(self):
        rng = np.random.default_rng(13)
        held = np.concatenate([self.A.keys, self.B.keys[
            ~np.isin(sm.skeys(self.B.keys), sm.skeys(self.A.keys))]])
        n1 = self.N_T
        k1 = np.concatenate([held[rng.permutation(len(held))[:n1 // 2]],
                             sm.make_keys(rng, n1 - n1 // 2, n1 // 6)])
        m1 = sm.make_entries(rng, k1[rng.permutation(n1)], 0.10, 1 << 43)
        n2 = self.N_W
        k2 = np.concatenate([m1.keys[rng.permutation(n1)[:n2 // 2]],
                             sm.make_keys(rng, n2 - n2 // 2, n2 // 6)])
        m2 = sm.make_entries(rng, k2[rng.permutation(n2)], 0.10, 1 << 44)
        both = sm.Entries.concat([m1, m2])
        surv, (d, x) = sm.flush_model(both)
        assert len(np.unique(sm.skeys(m1.keys))) == n1
        assert len(surv) == n1 + n2 - n2 // 2 > self.T
        return m1, m2, surv, d, x

    @cached_property
    def compacted(self):
        import oracle

        od, oi, on = oracle.compact(self.runs, keep_tombstones=False)
        assert on > self.T
        keys = sm.Table(od, oi, K).keys
        return od, oi, on, bloom_model.build(keys)


@pytest.fixture(scope="module")
def w():
    return World()


@pytest.fixture(params=["radix", "merge"])
def order(request, monkeypatch):
    monkeypatch.setenv("DBEEL_BATCH_ORDER", request.param)
    return request.param


def _assert_get(got, w, hits, voff, vals, what):
    ghits, gvoff, gvals, st = got
    sm.assert_fields(ghits, hits, what + " hits")
    sm.assert_fields(gvoff, voff, what + " value offsets")
    sm.assert_bytes(gvals, vals, what + " values")
    assert st["hits"] == int((hits["run"] >= 0).sum()), what
    assert st["tombstones"] == int(hits["is_tombstone"].sum()), what
    return st


# ---- 1. open + get, no filters ----

def test_get_without_filters(w):
    hits, (voff, vals) = w.hits, w.values
    assert vals.size == 8 * int((hits["value_len"] > 0).sum())
    with Reader(w.runs, device=0) as rd:
        st = _assert_get(rd.get_raw(w.q_list), w, hits, voff, vals, "get")
    assert st["bloom_probes"] == 0 and st["bloom_skips"] == 0
    # run 1 is visited by every query, run 0 by those run 1 does not hold
    assert st["searches"] == w.N_T + int((hits["run"] != 1).sum())
    old = lookup_raw(w.runs, w.q_list, device=0)
    sm.assert_fields(old, hits, "dbeel_gpu_lookup")


# ---- 2. filters ----

@pytest.mark.parametrize("r", [0, 1])
def test_job_bloom_bytes(w, r):
    keys = (w.A, w.B)[r].keys
    n_bits = bloom_model.n_bits_for(w.N_T)
    tail_bits = bloom_model.bit_positions(keys[w.T:], n_bits)
    assert np.unique(tail_bits).size > 7 * (w.N_T - w.T) // 2
    with Job([w.runs[r]], device=0) as job:
        _, n, _ = job.run(True)
        assert n == w.N_T
        got = job.bloom()
    sm.assert_bytes(got, w.blooms[r], f"filter of run {r}")


def test_job_fetch_into_rebased(w):
    """Every index offset leaves with index_base added on the device, the
    job's own result unchanged."""
    base = (1 << 40) + 12345
    d, x = w.runs[0]
    exp = x.view(INDEX_DTYPE).copy()
    exp["offset"] += np.uint64(base)
    with Job([w.runs[0]], device=0) as job:
        job.run(True)
        gd, gx = guarded(d.size + 4096), guarded(x.size + 4096)
        dl, il, _ = job.fetch_into(gd, gx, index_base=base)
        assert (dl, il) == (d.size, x.size)
        sm.assert_fields(gx[:il].view(INDEX_DTYPE), exp, "rebased index")
        sm.assert_bytes(gd[:dl], d, "fetch_into data")
        sm.assert_guard(gd, dl, GUARD, "fetch_into data")
        sm.assert_guard(gx, il, GUARD, "fetch_into index")
        fd, fx, n = job.fetch()
        assert n == w.N_T
        sm.assert_bytes(fx, x, "job index after a rebased fetch")
        sm.assert_bytes(fd, d, "job data after a rebased fetch")


def test_get_with_filters(w):
    hits, (voff, vals) = w.hits, w.values
    maybe_a = bloom_model.maybe(w.blooms[0], w.q)
    maybe_b = bloom_model.maybe(w.blooms[1], w.q)
    visit_a = hits["run"] != 1
    probes = w.N_T + int(visit_a.sum())
    skips = int((~maybe_b).sum()) + int((visit_a & ~maybe_a).sum())
    assert skips > 1000 and (~maybe_b[w.T - 1000:]).sum() > 0
    with Reader(w.runs, blooms=w.blooms, device=0) as rd:
        st = _assert_get(rd.get_raw(w.q_list), w, hits, voff, vals,
                         "filtered get")
    assert st["bloom_probes"] == probes
    assert st["bloom_skips"] == skips
    assert st["searches"] == probes - skips


# ---- 3. write batch ----

def test_write_batch(w, order):
    surv, md, mx, tied = w.batch_expect
    bloom = bloom_model.build(surv.keys)
    with Reader([TINY], device=0) as rd:
        d, x, b, st = rd.write_batch(w.batch_writes, build_bloom=True)
        sm.assert_bytes(x, mx, "write_batch index")
        sm.assert_bytes(d, md, "write_batch data")
        sm.assert_bytes(b, bloom, "write_batch filter")
        assert st["writes_in"] == w.N_T
        assert st["entries_out"] == len(surv)
        assert st["data_bytes_out"] == md.size
        assert st["prefix_tied"] == tied
        assert rd.n_runs == 2
        # the new table answers: survivors from its far end, filter in place
        qk = surv.keys[-(w.N_T - w.T):]
        h = sm.ReadModel([(md, mx)], K).hits(qk)
        got, _, _, gst = rd.get_raw(sm.key_list(qk))
        h["run"] = 1
        sm.assert_fields(got, h, "get after write_batch")
        assert gst["bloom_skips"] == 0 and gst["bloom_probes"] == len(qk)
    fd, fx, fn = engine.flush_batch(w.batch_writes, device=0)
    assert fn == len(surv)
    sm.assert_bytes(fx, mx, "flush_batch index")
    sm.assert_bytes(fd, md, "flush_batch data")


# ---- 4. memtable ----

def test_memtable(w):
    m1, m2, surv, md, mx = w.mem
    first, (d1, x1) = sm.flush_model(m1)
    with Reader(w.runs, device=0) as rd:
        st = rd.put(m1.writes())      # into an empty memtable: adopted
        assert (st["writes_in"], st["batch_entries"], st["replaced"],
                st["entries"]) == (w.N_T, w.N_T, 0, w.N_T)
        assert st["data_bytes"] == d1.size
        assert st["prefix_tied"] == sm.prefix_tied(m1.keys)
        d, x = rd.memtable_fetch()
        sm.assert_bytes(x, x1, "memtable index after the first put")
        sm.assert_bytes(d, d1, "memtable data after the first put")
        st = rd.put(m2.writes())      # merged: m + nb > T
        assert (st["writes_in"], st["batch_entries"], st["replaced"],
                st["entries"]) == (w.N_W, w.N_W, w.N_W // 2, len(surv))
        assert st["data_bytes"] == md.size
        d, x = rd.memtable_fetch()
        sm.assert_bytes(x, mx, "memtable index")
        sm.assert_bytes(d, md, "memtable data")

        # gets see the memtable first, reported at run == n_runs
        model = sm.ReadModel(w.runs, K, mem_run=(md, mx))
        rng = np.random.default_rng(14)
        q = w.q.copy()
        swap = rng.permutation(w.N_T)[:w.N_T // 3]
        q[swap] = surv.keys[rng.integers(0, len(surv), swap.size)]
        live = np.flatnonzero(model.vlen != 0)  # the tail: values only
        q[w.T:] = model.keys[live[rng.integers(
            0, live.size, w.N_T - w.T)]].view(np.uint8).reshape(-1, K)
        hits = model.hits(q)
        voff, vals = model.values(q)
        assert set(hits["run"].tolist()) == {-1, 0, 1, 2}
        assert np.all(hits["value_len"][w.T:] == 8)
        assert set(hits["run"][w.T:].tolist()) == {0, 1, 2}
        ql = sm.key_list(q)
        st = _assert_get(rd.get_raw(ql), w, hits, voff, vals,
                         "get over the memtable")
        assert st["searches"] == (w.N_T + int((hits["run"] < 2).sum())
                                  + int((hits["run"] < 1).sum()))

        fd, fx, _ = rd.memtable_flush()
        sm.assert_bytes(fx, mx, "memtable_flush index")
        sm.assert_bytes(fd, md, "memtable_flush data")
        assert rd.n_runs == 3 and rd.memtable_info["entries"] == 0
        _assert_get(rd.get_raw(ql), w, hits, voff, vals, "get after flush")


# ---- 5. get_entries and get_merged ----

def _entries_call(rd, w, p, cap, buf):
    """One get_entries call for the queries from p on into the guarded
    buffer: everything it reports against the model."""
    hits = w.hits[p:]
    roff, rec = w.records
    base = roff[p]
    exp_off = roff[p:] - base
    n = w.N_T - p
    ka = np.ascontiguousarray(w.q[p:]).reshape(-1)
    koff = np.arange(n + 1, dtype=np.uint64) * K
    ghits = guarded(n, HIT_DTYPE)
    goff = guarded(n + 1, np.uint64)
    buf[:] = GUARD
    rc, page, st = rd._get_entries_into(ka, koff, ghits, goff, buf, cap)
    assert rc == 0, rc
    page = page.as_dict()
    assert page == sm.paging(exp_off, cap)
    sm.assert_fields(ghits, hits, f"get_entries hits from {p}")
    sm.assert_fields(goff, exp_off, f"get_entries offsets from {p}")
    used = page["records_len"]
    sm.assert_bytes(buf[:used], rec[int(base):int(base) + used],
                    f"get_entries records from {p}")
    sm.assert_guard(buf, used, GUARD, f"get_entries records from {p}")
    assert st.hits == int((hits["run"] >= 0).sum())
    return page


def test_get_entries(w):
    roff, rec = w.records
    assert np.all(np.diff(roff)[w.T:] == 32)
    total = int(roff[-1])
    buf = np.empty(total + 4096, dtype=np.uint8)
    with Reader(w.runs, device=0) as rd:
        page = _entries_call(rd, w, 0, total, buf)
        assert page["n_done"] == w.N_T and page["needed"] == 0
        # one short page whose boundary lies past W
        page = _entries_call(rd, w, 0, int(roff[w.W + 77]) + 5, buf)
        assert w.W < page["n_done"] < w.T
        # three pages, the first boundary past T
        p = 0
        for upto in (w.T + 100, w.T + 300, w.N_T):
            page = _entries_call(rd, w, p, int(roff[upto] - roff[p]) + 7,
                                 buf)
            assert page["n_done"] == upto - p
            p = upto


@pytest.fixture(scope="module")
def replicas(w):
    """Two more replicas and the expected pick over (C reader, D's uploaded
    answer, local A + B)."""
    rng = np.random.default_rng(15)
    C = sm.make_remote(rng, w.B, w.N_T // 2, 1 << 42)
    D = sm.make_remote(rng, w.A, w.N_T // 2, 1 << 41)
    rc, rd_ = sm.encode_run(C), sm.encode_run(D)
    q = w.q.copy()
    third = w.N_T // 3
    q[:third] = C.keys[rng.integers(0, len(C), third)]
    q[third:2 * third] = D.keys[rng.integers(0, len(D), third)]
    q = q[rng.permutation(w.N_T)]
    models = [sm.ReadModel([rc], K), sm.ReadModel([rd_], K), w.model]
    hits, _, _ = sm.merge_expect([m.records(q) for m in models])
    # the tail: queries whose winner is a value, whoever holds it
    good = np.flatnonzero(hits["value_len"][:w.T] == 8)
    q[w.T:] = q[good[rng.integers(0, good.size, w.N_T - w.T)]]
    answers = [m.records(q) for m in models]
    hits, roff, rec = sm.merge_expect(answers)
    local = w.model.hits(q)
    lt = local["is_tombstone"] == 1
    assert (lt & (hits["source"] == 2)).sum() > 100   # local tombstone wins
    assert (lt & (hits["source"] == 0)).sum() > 100   # ... and loses
    assert set(hits["source"].tolist()) == {-1, 0, 1, 2}
    assert len(set(hits["stale_mask"].tolist())) >= 6
    assert set(hits["source"][w.T:].tolist()) == {0, 1, 2}
    assert np.all(hits["value_len"][w.T:] == 8)
    return rc, q, answers, hits, roff, rec


def _merged_call(rd, src_reader, w, replicas, p, cap, buf):
    _, q, answers, hits, roff, rec = replicas
    n = w.N_T - p
    base = roff[p]
    exp_off = roff[p:] - base
    doff, drec = answers[1]
    pair = (doff[p:] - doff[p], drec[int(doff[p]):])
    srcs, keep = Reader._merge_sources([src_reader, pair])
    ka = np.ascontiguousarray(q[p:]).reshape(-1)
    koff = np.arange(n + 1, dtype=np.uint64) * K
    ghits = guarded(n, MERGE_HIT_DTYPE)
    goff = guarded(n + 1, np.uint64)
    buf[:] = GUARD
    rc, page, st = rd._get_merged_into(ka, koff, srcs, 2, ghits, goff, buf,
                                       cap)
    del keep
    assert rc == 0, rc
    page = page.as_dict()
    assert page == sm.paging(exp_off, cap)
    sm.assert_fields(ghits, hits[p:], f"get_merged hits from {p}")
    sm.assert_fields(goff, exp_off, f"get_merged offsets from {p}")
    used = page["records_len"]
    sm.assert_bytes(buf[:used], rec[int(base):int(base) + used],
                    f"get_merged records from {p}")
    sm.assert_guard(buf, used, GUARD, f"get_merged records from {p}")
    h = hits[p:]
    assert st.winners == int((h["source"] >= 0).sum())
    assert st.tombstones == int(h["is_tombstone"].sum())
    assert st.from_local == int((h["source"] == 2).sum())
    return page


def test_get_merged(w, replicas):
    rc, q, answers, hits, roff, rec = replicas
    total = int(roff[-1])
    buf = np.empty(total + 4096, dtype=np.uint8)
    with Reader(w.runs, device=0) as rd, Reader([rc], device=0) as src:
        page = _merged_call(rd, src, w, replicas, 0, total, buf)
        assert page["n_done"] == w.N_T
        page = _merged_call(rd, src, w, replicas, 0,
                            int(roff[w.W + 77]) + 5, buf)
        assert w.W < page["n_done"] < w.T
        p = 0
        for i, upto in enumerate((w.T + 100, w.T + 300, w.N_T)):
            page = _merged_call(rd, src, w, replicas, p,
                                int(roff[upto] - roff[p]), buf)
            assert page["n_done"] == upto - p
            p = upto


# ---- 6. paged scans with one window past T ----

def _drain(sc, w, data_cap, n_cap, ranged):
    """All pages of an open scan into guarded buffers -> (data, index
    rebased into one run file, range ids, pages)."""
    data = np.empty(data_cap, dtype=np.uint8)
    index = np.empty(16 * n_cap, dtype=np.uint8)
    rid = np.empty(n_cap, dtype=np.uint32) if ranged else None
    datas, recs, rids, pages = [], [], [], []
    off = 0
    while True:
        data[:] = GUARD
        index[:] = GUARD
        if ranged:
            rid.view(np.uint8)[:] = GUARD
        pg = sc.next(data, index, rid)
        n = pg["n_entries"]
        sm.assert_guard(data, pg["data_len"], GUARD, "page data")
        sm.assert_guard(index, 16 * n, GUARD, "page index")
        if ranged:
            sm.assert_guard(rid, 4 * n, GUARD, "page range ids")
            rids.append(rid[:n].copy())
        r = index[:16 * n].view(INDEX_DTYPE).copy()
        r["offset"] += off
        off += pg["data_len"]
        datas.append(data[:pg["data_len"]].copy())
        recs.append(r)
        pages.append(pg)
        if pg["done"]:
            break
    return (np.concatenate(datas), np.concatenate(recs).view(np.uint8),
            np.concatenate(rids) if ranged else None, pages)


def _scan_filters(w):
    start = bytes(w.A.keys[w.N_T // 20])
    end = bytes(w.A.keys[-(w.N_T // 20)])
    ranges = [(0x20000000, 0x90000000), (0xF0000000, 0x30000000)]  # 2nd wraps
    return start, end, ranges


def _assert_scan(got, exp, what):
    d, x, rid, _ = got
    ed, ex, erid, _ = exp
    sm.assert_bytes(x, ex, what + " index")
    sm.assert_bytes(d, ed, what + " data")
    if rid is not None:
        sm.assert_fields(rid, erid, what + " range ids")


def test_scan_window_past_the_cap(w):
    start, end, ranges = _scan_filters(w)
    exp = sm.scan_model(w.tabs, start, end, ranges)
    n_exp = exp[1].size // 16
    assert n_exp > w.T and set(exp[2].tolist()) == {0, 1}
    assert set(exp[2][w.T:].tolist()) == {0, 1}
    with Reader(w.runs, device=0) as rd:
        with rd.scan_open(start, end, ranges) as sc:   # default window
            got = _drain(sc, w, exp[0].size + 4096, n_exp + 16, True)
        pages = got[3]
        assert pages[0]["candidates"] > w.T and pages[0]["n_entries"] > w.T
        _assert_scan(got, exp, "paged scan")
    d, x, n = engine.scan(w.runs, start, end, ranges, device=0)
    assert n == n_exp
    sm.assert_bytes(x, exp[1], "dbeel_gpu_scan index")
    sm.assert_bytes(d, exp[0], "dbeel_gpu_scan data")


def test_scan_unfiltered_equals_dbeel_gpu_scan(w):
    exp = sm.scan_model(w.tabs)
    assert exp[1].size // 16 == 2 * w.N_T
    with Reader(w.runs, device=0) as rd:
        with rd.scan_open() as sc:
            got = _drain(sc, w, exp[0].size + 4096, 2 * w.N_T + 16, False)
        assert got[3][0]["n_entries"] == min(2 * w.N_T, 1 << 20) > w.T
        _assert_scan(got, exp, "paged scan, no filter")
    d, x, n = engine.scan(w.runs, device=0)
    assert n == 2 * w.N_T
    sm.assert_bytes(x, exp[1], "dbeel_gpu_scan index")
    sm.assert_bytes(d, exp[0], "dbeel_gpu_scan data")


def _small_put(w):
    """N_W writes for a memtable segment: half overwrite keys of B."""
    rng = np.random.default_rng(16)
    n = w.N_W
    keys = np.concatenate([w.B.keys[rng.permutation(w.N_T)[:n // 2]],
                           sm.make_keys(rng, n - n // 2, n // 6)])
    e = sm.make_entries(rng, keys[rng.permutation(n)], 0.10, 1 << 45)
    surv, run = sm.flush_model(e)
    return e, run


def test_snapshot_with_memtable(w):
    start, end, ranges = _scan_filters(w)
    e, run = _small_put(w)
    tabs = w.tabs + [sm.Table(run[0], run[1], K)]
    exp = sm.scan_model(tabs, start, end, ranges)
    n_exp = exp[1].size // 16
    with Reader(w.runs, device=0) as rd:
        rd.put(e.writes())
        with rd.snapshot_open(start, end, ranges, memtable=True) as sc:
            got = _drain(sc, w, exp[0].size + 4096, n_exp + 16, True)
            info = sc.info()
        assert info["has_memtable"] == 1 and info["n_tables"] == 2
        assert info["memtable_candidates"] > w.W
        assert got[3][0]["n_entries"] > w.T
        _assert_scan(got, exp, "snapshot with memtable")


@pytest.mark.parametrize("variant", ["narrow", "full"])
def test_snapshot_newest_only(w, variant, monkeypatch):
    monkeypatch.setenv("DBEEL_SCAN_SHADOW", variant)
    start, end, ranges = _scan_filters(w)
    e, run = _small_put(w)
    tabs = w.tabs + [sm.Table(run[0], run[1], K)]
    exp = sm.scan_model(tabs, start, end, ranges, newest_only=True)
    n_exp = exp[1].size // 16
    assert exp[3] > w.N_T // 4 and n_exp > w.T
    with Reader(w.runs, device=0) as rd:
        rd.put(e.writes())
        with rd.snapshot_open(start, end, ranges, memtable=True,
                              newest_only=True) as sc:
            got = _drain(sc, w, exp[0].size + 4096, n_exp + 16, True)
            info = sc.info()
        assert got[3][0]["candidates"] > w.T
        _assert_scan(got, exp, f"newest-only snapshot ({variant})")
        assert info["shadowed"] == exp[3]


# ---- 7. put_entries / scan_apply ----

def test_scan_apply_and_put_entries(w):
    window = 1 << 20                # SCAN_DEFAULT_CANDIDATES: the first page
    assert w.N_T < window < 2 * w.N_T
    b_part = sm.Table(w.runs[1][0], w.runs[1][1][:16 * (window - w.N_T)], K)
    page = sm.scan_model([w.tabs[0], b_part], ranges=HASH_3)
    pd, px, prid, _ = page
    n_page = px.size // 16
    sel = prid < 2
    assert n_page > w.T and set(prid.tolist()) == {0, 1, 2}
    assert sel.sum() > n_page // 2 and sel[w.T:].sum() > 100
    assert (prid[w.T:] == 0).sum() > 50 and (prid[w.T:] == 1).sum() > 50
    ents = sm.Table(pd, px, K).entries()
    delete_ts = -(1 << 70) - 12345
    puts = ents.take(np.flatnonzero(prid == 0))
    dels = ents.take(np.flatnonzero(prid == 1))
    dels.vlen = np.zeros(len(dels), dtype=np.int64)
    dels.ts = np.tile(np.frombuffer(
        delete_ts.to_bytes(16, "little", signed=True), dtype=np.uint8),
        (len(dels), 1))
    surv, (md, mx) = sm.flush_model(sm.Entries.concat([puts, dels]))
    assert np.any(surv.vlen[-100:] != 0)

    with Reader(w.runs, device=0) as src, Reader([TINY], device=0) as dst, \
            Reader([TINY], device=0) as dst2:
        with src.snapshot_open(hash_ranges=HASH_3) as sc:
            pg, st = sc.apply([("put", dst), ("delete", dst), ("skip",)],
                              page_bytes=pd.size + 4096,
                              page_entries=n_page + 16, delete_ts=delete_ts)
        assert pg["n_entries"] == n_page and pg["candidates"] == window
        assert st["put_entries"] == len(puts)
        assert st["delete_entries"] == len(dels)
        assert st["skipped"] == int((prid == 2).sum())
        d, x = dst.memtable_fetch()
        sm.assert_bytes(x, mx, "scan_apply memtable index")
        sm.assert_bytes(d, md, "scan_apply memtable data")

        # the host route: the same page fetched, then put_entries twice
        with src.snapshot_open(hash_ranges=HASH_3) as sc:
            data = np.empty(pd.size + 4096, dtype=np.uint8)
            index = np.empty(16 * (n_page + 16), dtype=np.uint8)
            rid = np.empty(n_page + 16, dtype=np.uint32)
            pg = sc.next(data, index, rid)
        n = pg["n_entries"]
        assert n == n_page
        sm.assert_bytes(index[:16 * n], px, "page index")
        sm.assert_bytes(data[:pg["data_len"]], pd, "page data")
        sm.assert_fields(rid[:n], prid, "page range ids")
        st = dst2.put_entries(data[:pg["data_len"]], index[:16 * n], rid[:n],
                              take=[1, 0, 0])
        assert st["selected"] == len(puts) and st["entries_in"] == n
        st = dst2.put_entries(data[:pg["data_len"]], index[:16 * n], rid[:n],
                              take=[0, 1, 0], delete_ts=delete_ts)
        assert st["selected"] == len(dels) and st["entries"] == len(surv)
        d, x = dst2.memtable_fetch()
        sm.assert_bytes(x, mx, "put_entries memtable index")
        sm.assert_bytes(d, md, "put_entries memtable data")


# ---- 8. live reader compaction ----

def test_live_compaction(w):
    od, oi, on, bloom = w.compacted
    with Reader(w.runs, device=0) as rd:
        d, x, b, st = rd.compact_begin([0, 1], keep_tombstones=False,
                                       bloom=True)
        assert st["entries_out"] == on and st["entries_in"] == 2 * w.N_T
        sm.assert_bytes(x, oi, "compact_begin index")
        sm.assert_bytes(d, od, "compact_begin data")
        sm.assert_bytes(b, bloom, "adopted filter")
        gd, gx = guarded(len(od) + 4096), guarded(len(oi) + 4096)
        dl, il, _ = rd.compact_fetch_into(gd, gx)
        assert (dl, il) == (len(od), len(oi))
        sm.assert_bytes(gx[:il], oi, "compact_fetch_into index")
        sm.assert_bytes(gd[:dl], od, "compact_fetch_into data")
        sm.assert_guard(gd, dl, GUARD, "compact_fetch_into data")
        sm.assert_guard(gx, il, GUARD, "compact_fetch_into index")
        rd.compact_commit(0)
        assert rd.n_runs == 1
        # gets afterwards: the one table, tombstones gone, filter probed
        model = sm.ReadModel([(od, oi)], K)
        hits = model.hits(w.q)
        voff, vals = model.values(w.q)
        assert np.all(hits["value_len"][w.T:] == 8)
        got = rd.get_raw(w.q_list)
        st = _assert_get(got, w, hits, voff, vals, "get after compaction")
        skips = int((~bloom_model.maybe(bloom, w.q)).sum())
        assert st["bloom_probes"] == w.N_T and st["bloom_skips"] == skips
        assert skips > 1000


# ---- 9. compact_into, the filter across slices ----

@pytest.mark.parametrize("n_slices", [1, 3])
def test_compact_into_slices(w, n_slices):
    od, oi, on, bloom = w.compacted
    gd, gx = guarded(len(od) + 4096), guarded(len(oi) + 4096)
    dl, il, n, st, b = engine.compact_into(
        w.runs, False, gd, gx, device=0, n_slices=n_slices, bloom=True)
    assert (dl, il, n) == (len(od), len(oi), on)
    assert st["slices"] == n_slices
    sm.assert_bytes(gx[:il], oi, "compact_into index")
    sm.assert_bytes(gd[:dl], od, "compact_into data")
    sm.assert_guard(gd, dl, GUARD, "compact_into data")
    sm.assert_guard(gx, il, GUARD, "compact_into index")
    sm.assert_bytes(b, bloom, "filter across slices")


# ---- 10. encode_run ----

def _encode_arrays(keys_blob, koff, vals_blob, voff, ts):
    lib = engine.load()
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    res = CompactResult()
    rc = lib.dbeel_gpu_encode_run(
        len(koff) - 1, keys_blob.ctypes.data_as(u8), koff.ctypes.data_as(u64),
        vals_blob.ctypes.data_as(u8), voff.ctypes.data_as(u64),
        ts.ctypes.data_as(u8), 0, ctypes.byref(res))
    assert rc == 0, lib.dbeel_gpu_last_error().decode()
    try:
        return (engine._ptr_bytes(res.data, res.data_len),
                engine._ptr_bytes(res.index, res.index_len))
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))


def test_encode_run_fixed(w):
    rng = np.random.default_rng(17)
    e = w.A.take(np.arange(w.N_T))
    e.ts = sm.ts_bytes(rng.integers(0, 1 << 63, w.N_T, dtype=np.uint64),
                       rng.integers(-3, 3, w.N_T))
    assert np.any(e.ts[w.T:, 15] == 0xFF) and np.any(e.vlen[w.T:] == 8)
    assert np.any(e.vlen[w.T:] == 0)
    md, mx = sm.encode_run(e)
    d, x = _encode_arrays(
        np.ascontiguousarray(e.keys).reshape(-1),
        np.arange(w.N_T + 1, dtype=np.uint64) * K,
        np.ascontiguousarray(e.vals[e.vlen != 0]).reshape(-1),
        sm.offsets_of(e.vlen), np.ascontiguousarray(e.ts).reshape(-1))
    sm.assert_bytes(x, mx, "encode_run index")
    sm.assert_bytes(d, md, "encode_run data")


# ---- 11. the wave-per-item kernels at N_W, awkward lengths ----

KEY_LENS = (1, 7, 8, 9, 33)
VAL_LENS = (0, 1, 7, 8, 9, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def ragged(w):
    """N_W entries whose key and value lengths cycle through the awkward
    ones (1-byte keys as long as there are any), unsorted, unique."""
    rng = np.random.default_rng(18)
    seen, writes = set(), []
    for i in range(w.N_W):
        kl = KEY_LENS[i % len(KEY_LENS)]
        if kl > 1:
            k = b"%0*d" % (kl, i)   # neighbours share their first 8 bytes
        elif i // len(KEY_LENS) < 256:
            k = bytes([i // len(KEY_LENS)])
        else:                       # all 256 one-byte keys are taken
            k = b"x%032d" % i
        assert k not in seen and len(k) in KEY_LENS
        seen.add(k)
        vl = VAL_LENS[(i * 7 + i // 9) % len(VAL_LENS)]
        v = bytes(rng.integers(1, 256, vl, dtype=np.uint8))
        writes.append((k, v, int(rng.integers(-10**15, 10**15))))
    order = rng.permutation(w.N_W)
    writes = [writes[int(j)] for j in order]
    run = batch_model.flush_run(writes)
    model = gem.Model([run])
    keys = [e.key for e in batch_model.flush_entries(writes)]
    keys = [keys[int(j)] for j in rng.permutation(w.N_W)]
    assert {len(k) for k in keys} == set(KEY_LENS)
    # every value length lies in a later trip, a value in the third
    assert {len(model.where[k][2].data) for k in keys[w.W:]} == set(VAL_LENS)
    assert any(model.where[k][2].data for k in keys[2 * w.W:])
    assert any(w_[1] for w_ in writes[2 * w.W:])
    return writes, run, model, keys


def test_ragged_get_and_get_entries(w, ragged):
    writes, run, model, keys = ragged
    hits, offsets, records, _, _ = model.expect(keys)
    hits = gem.hits_array(hits, HIT_DTYPE)
    vals = b"".join(model.where[k][2].data for k in keys)
    with Reader([run], device=0) as rd:
        ghits, gvoff, gvals, _ = rd.get_raw(keys)
        sm.assert_fields(ghits, hits, "ragged get hits")
        sm.assert_fields(gvoff, sm.offsets_of(hits["value_len"]),
                         "ragged get offsets")
        sm.assert_bytes(gvals, vals, "ragged get values")
        buf = guarded(len(records) + 4096)
        ehits, eoff, view, page, _ = rd.get_entries_raw(keys, records=buf)
        assert page["n_done"] == w.N_W and page["records_len"] == len(records)
        sm.assert_fields(ehits, hits, "ragged get_entries hits")
        sm.assert_fields(eoff, np.array(offsets, dtype=np.uint64),
                         "ragged get_entries offsets")
        sm.assert_bytes(view, records, "ragged get_entries records")
        sm.assert_guard(buf, len(records), GUARD, "ragged get_entries")


def test_ragged_write_batch_and_put_entries(w, ragged, order):
    writes, run, model, keys = ragged
    with Reader([TINY], device=0) as rd, Reader([TINY], device=0) as dst:
        d, x, _, st = rd.write_batch(writes)
        sm.assert_bytes(x, run[1], "ragged write_batch index")
        sm.assert_bytes(d, run[0], "ragged write_batch data")
        assert st["entries_out"] == w.N_W
        pd, px = migrate_model.encode_page(writes)
        st = dst.put_entries(pd, px)
        assert st["selected"] == w.N_W and st["entries"] == w.N_W
        d, x = dst.memtable_fetch()
        sm.assert_bytes(x, run[1], "ragged put_entries index")
        sm.assert_bytes(d, run[0], "ragged put_entries data")


def test_ragged_encode_run(w, ragged):
    writes, run, _, _ = ragged
    ents = batch_model.flush_entries(writes)
    assert {len(e.data) for e in ents[w.W:]} >= set(VAL_LENS)
    assert any(e.data for e in ents[2 * w.W:])
    d, x, _ = engine.encode_run([(e.key, e.data, e.timestamp) for e in ents],
                                device=0)
    sm.assert_bytes(x, run[1], "ragged encode_run index")
    sm.assert_bytes(d, run[0], "ragged encode_run data")
