"""Prefix-tie handling in k_corank and the device-resident step totals.

k_corank settles pairs whose 8-byte key prefixes are equal ahead of its
walk (a per-thread scout notes up to CORANK_TIE_HINTS such pairs), never
evaluates one pair twice, and its diagonal searches decide on prefixes
alone where those can decide. The inputs here put ties where those paths
differ: 0 .. 4 ties per 8-position sub-window, pairs straddling the
8-position and 2048-position seams, prefix groups wider than the walk's 8
steps, keys present in many runs with equal timestamps. The second half
covers the emit -> copy hand-off through the device totals record: no
survivors, less than one copy window, exactly one and two full windows,
repeated runs, and a corrupt input followed by a valid one.

Every GPU result is compared byte-for-byte with the C oracle, for both
keep_tombstones settings and both corank block sizes. The CPU test pins
the oracle on the same inputs against the independent Python merge.
"""
import functools
import struct

import numpy as np
import pytest

import oracle
import pymerge
from dbeel_amd.format import Entry, build_run, parse_run

N_PER_RUN = 3000  # 2 runs -> 6000 merged positions = 3 windows of 2048


def _rand_keys(rng, n, klen):
    """n distinct klen-byte keys with distinct 8-byte prefixes, sorted."""
    pfx = rng.choice(1 << 62, size=n, replace=False)
    keys = []
    for p in np.sort(pfx):
        tail = bytes(rng.integers(0, 256, klen - 8, dtype=np.uint8))
        keys.append(int(p).to_bytes(8, "big") + tail)
    return keys


def _val(rng):
    return bytes(rng.integers(1, 256, 8, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def density_runs(j, klen, lead):
    """Run 0 holds N keys; every j-th of them is also in run 1 (the rest
    of run 1 is its own keys), so sub-windows see 4 (j=1), 2-3 (j=2) ...
    <= 1 (j=8) ties per 8 merged positions. Which side is newer is drawn
    per key. lead=1 puts one unshared smallest key into run 0, which moves
    every tie pair one position along: pairs then straddle the 8-position
    and 2048-position seams."""
    rng = np.random.default_rng(1000 * j + klen + lead)
    pool = _rand_keys(rng, 2 * N_PER_RUN, klen)
    k0 = pool[0::2]
    own1 = pool[1::2]
    k1 = sorted(k0[i] if i % j == 0 else own1[i] for i in range(N_PER_RUN))
    shared = set(k0) & set(k1)
    newer0 = {k: bool(rng.integers(0, 2)) for k in shared}
    e0, e1 = [], []
    if lead:
        e0.append(Entry(b"\x00" * klen, _val(rng), 5))
    for k in k0:
        ts = 200 if newer0.get(k, False) else 100
        e0.append(Entry(k, b"" if rng.random() < 0.05 else _val(rng), ts))
    for k in k1:
        ts = 100 if newer0.get(k, True) else 200
        e1.append(Entry(k, b"" if rng.random() < 0.05 else _val(rng), ts))
    return (build_run(e0), build_run(e1))


@functools.lru_cache(maxsize=None)
def family_runs(g, klen, lead):
    """Groups of g keys sharing their first 8 bytes (and, past them, all
    but the last 4 bytes, so long keys also tie through the staged
    suffix), present in both runs. A run-1 member is, by draw, identical
    to its run-0 partner, different only in its last byte, or a strict
    prefix of it (different only in length). The groups fill both runs, so
    they lie across every sub-window and window seam; g = 9 is wider than
    the 8 steps of one sub-window."""
    rng = np.random.default_rng(7000 + 100 * g + klen + lead)
    n_fam = N_PER_RUN // g
    pfx = np.sort(rng.choice(1 << 62, size=n_fam, replace=False))
    s0, s1 = set(), set()
    for p in pfx:
        common = int(p).to_bytes(8, "big") + bytes(
            rng.integers(0, 256, klen - 12, dtype=np.uint8))
        tails = rng.choice(1 << 24, size=g, replace=False)
        for t in tails:
            k = common + struct.pack(">I", int(t) << 8 | 0x10)
            s0.add(k)
            kind = int(rng.integers(0, 4))
            if kind == 0:
                s1.add(k)                      # identical across runs
            elif kind == 1:
                s1.add(k[:-1] + b"\x11")       # differs after byte 8
            elif kind == 2:
                s1.add(k[: -int(rng.integers(1, 4))])  # length only
            else:
                s1.add(k)
                s1.add(k[:-2])                 # both: equal and shorter
    e0 = [Entry(b"\x00" * klen, _val(rng), 5)] if lead else []
    for k in sorted(s0):
        e0.append(Entry(k, b"" if rng.random() < 0.1 else _val(rng),
                        int(rng.integers(0, 3))))
    e1 = [Entry(k, b"" if rng.random() < 0.1 else _val(rng),
                int(rng.integers(0, 3))) for k in sorted(s1)]
    return (build_run(e0), build_run(e1))


@functools.lru_cache(maxsize=None)
def partner_runs(k):
    """k non-empty runs drawing from one key pool, so most keys sit in 3
    or more runs; all timestamps equal, so the run index decides. Empty
    runs sit between and after them."""
    rng = np.random.default_rng(31 * k)
    pool = _rand_keys(rng, 1500, 32)
    runs = []
    for r in range(k):
        take = rng.random(len(pool)) < (0.8 if k == 3 else 0.5)
        ents = [Entry(key, b"" if rng.random() < 0.1 else bytes([r + 1]) * 8,
                      7)
                for key, t in zip(pool, take) if t]
        runs.append(build_run(ents))
        if r == 0:
            runs.append((b"", b""))
    runs.append((b"", b""))
    return tuple(runs)


def _big_entries(n):
    """n entries of exactly 1024 B: 16-B key + 976-B value."""
    return [Entry(struct.pack(">QQ", i + 1, i), bytes([i % 251 + 1]) * 976,
                  i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def window_runs(n_windows):
    """Survivor data of exactly n_windows x 64 KiB (1024-B entries spread
    over two runs) plus one 32-B tombstone with the empty key: dropped, the
    output ends exactly on a window edge; kept, it is 32 B longer and every
    entry sits 32 B off the window grid."""
    ents = _big_entries(64 * n_windows)
    e0 = [Entry(b"", b"", 1)] + ents[0::2]
    e1 = ents[1::2]
    return (build_run(e0), build_run(e1))


@functools.lru_cache(maxsize=None)
def small_runs(kind):
    rng = np.random.default_rng(5)
    keys = _rand_keys(rng, 40, 16)
    if kind == "all_tombstones":
        return (build_run([Entry(k, b"", 1) for k in keys[0::2]]),
                build_run([Entry(k, b"", 2) for k in keys[1::2]]))
    # "tiny": far less than one copy window of output
    return (build_run([Entry(k, _val(rng), 1) for k in keys[:30]]),
            build_run([Entry(k, _val(rng), 2) for k in keys[20:]]))


CASES = {}
for _j in (1, 2, 3, 5, 8):
    for _klen in (16, 32, 48):
        for _lead in (0, 1):
            CASES[f"density-j{_j}-k{_klen}-lead{_lead}"] = functools.partial(
                density_runs, _j, _klen, _lead)
for _g in (1, 2, 3, 9):
    for _klen in (16, 32, 64):
        for _lead in (0, 1):
            CASES[f"family-g{_g}-k{_klen}-lead{_lead}"] = functools.partial(
                family_runs, _g, _klen, _lead)
for _k in (3, 8):
    CASES[f"partners-k{_k}"] = functools.partial(partner_runs, _k)
for _w in (1, 2):
    CASES[f"windows-{_w}"] = functools.partial(window_runs, _w)
for _kind in ("all_tombstones", "tiny"):
    CASES[f"small-{_kind}"] = functools.partial(small_runs, _kind)


@functools.lru_cache(maxsize=None)
def expected(name, keep):
    return oracle.compact(list(CASES[name]()), keep_tombstones=keep)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_pymerge(name, keep):
    od, oi, on = expected(name, keep)
    pd, pi = pymerge.merge(list(CASES[name]()), keep)
    assert oi == pi
    assert od == pd
    assert on == len(pi) // 16


def test_case_shapes():
    """The inputs are what the cases claim: three corank windows, window
    cases that end exactly on 64 KiB edges, a case without survivors."""
    d0, i0 = density_runs(1, 32, 0)[0]
    assert len(i0) // 16 == N_PER_RUN
    for name in CASES:  # every run strictly sorted by key
        for data, index in CASES[name]():
            keys = [e.key for e in parse_run(data, index)]
            assert all(x < y for x, y in zip(keys, keys[1:])), name
    for w in (1, 2):
        od, _, on = expected(f"windows-{w}", False)
        assert len(od) == w * 65536 and on == 64 * w
        od, _, on = expected(f"windows-{w}", True)
        assert len(od) == w * 65536 + 32 and on == 64 * w + 1
    assert expected("small-all_tombstones", False) == (b"", b"", 0)
    assert 0 < len(expected("small-tiny", False)[0]) < 32768
    # every density setting really has cross-run duplicates, j=1 only those
    for j in (1, 8):
        on = expected(f"density-j{j}-k32-lead0", True)[2]
        assert on == 2 * N_PER_RUN - (N_PER_RUN + j - 1) // j


@pytest.fixture(scope="module")
def engine():
    import dbeel_amd

    return dbeel_amd


@pytest.fixture(params=["256", "512"])
def corank_block(request, monkeypatch):
    monkeypatch.setenv("DBEEL_CORANK_BLOCK", request.param)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_matches_oracle(engine, corank_block, name, keep):
    gd, gi, gn = engine.compact(list(CASES[name]()), keep_tombstones=keep,
                                device=0)
    od, oi, on = expected(name, keep)
    assert gn == on
    assert gi == oi
    assert gd == od


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["windows-2", "density-j2-k32-lead1",
                                  "small-all_tombstones"])
def test_same_job_twice_is_identical(engine, name):
    with engine.Job(list(CASES[name]()), device=0) as job:
        for keep in (False, True, False):
            dl, ne, _ = job.run(keep)
            first = job.fetch()
            assert (dl, ne) == (len(first[0]), first[2])
            dl2, ne2, _ = job.run(keep)
            assert (dl2, ne2) == (dl, ne)
            assert job.fetch() == first
            assert first == expected(name, keep)


@pytest.mark.gpu
def test_corrupt_offset_then_valid_job(engine):
    from dbeel_amd.engine import DbeelGpuError

    good = list(density_runs(2, 32, 1))
    data, index = good[1]
    recs = np.frombuffer(index, dtype=pymerge.INDEX_DTYPE).copy()
    recs["offset"][1500] = len(data) + 4096  # points past the data file
    bad = [good[0], (data, recs.tobytes())]
    with engine.Job(bad, device=0) as job:
        for _ in range(2):
            with pytest.raises(DbeelGpuError) as ei:
                job.run(True)
            assert ei.value.code == 2  # CORRUPT
            with pytest.raises(DbeelGpuError):
                job.fetch()  # no result to hand out
    for keep in (True, False):
        assert engine.compact(good, keep_tombstones=keep, device=0) == \
            expected("density-j2-k32-lead1", keep)
