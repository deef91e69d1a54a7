#!/usr/bin/env python3
"""Randomized GPU-vs-oracle parity fuzzing.

Draws random run-set shapes (run count, entry counts incl. empty runs,
key/value size distributions incl. ragged and zero-length, timestamp
ranges incl. negatives and collisions, overlap patterns) and checks the
HIP engine's output is bit-identical to the CPU oracle for both
keep_tombstones settings; every trial also runs compact_into at a random
slice count against compact(). Heavier than the pytest suite:

    python tools/fuzz_parity.py --trials 150 --seed 1
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import oracle  # noqa: E402
import dbeel_amd  # noqa: E402
from dbeel_amd.format import Entry, build_run  # noqa: E402


def random_runs(rng):
    n_runs = int(rng.integers(1, 17))
    mode = rng.integers(0, 4)
    # shared key pool so overlaps (incl. >2-way) occur
    pool_size = int(rng.integers(5, 4000))
    if mode == 0:  # fixed short keys
        klen = int(rng.integers(1, 17))
        pool = {bytes(rng.integers(0, 256, klen, dtype=np.uint8))
                for _ in range(pool_size)}
    elif mode == 1:  # ragged keys incl. empty + prefixes
        pool = {b"", b"\x00"}
        for _ in range(pool_size):
            L = int(rng.integers(0, 129))
            k = bytes(rng.integers(0, 256, L, dtype=np.uint8))
            pool.add(k)
            if L > 1 and rng.random() < 0.2:
                pool.add(k[: L // 2])  # prefix pairs
    elif mode == 2:  # low-entropy keys (many shared prefixes)
        pool = {bytes(rng.integers(0, 3, int(rng.integers(1, 12)),
                                   dtype=np.uint8))
                for _ in range(pool_size)}
    else:  # long keys past every staged-suffix aux tier
        pool = {bytes(rng.integers(0, 4, int(rng.integers(41, 129)),
                                   dtype=np.uint8))
                for _ in range(pool_size)}
    pool = list(pool)

    ts_mode = rng.integers(0, 3)
    runs = []
    for r in range(n_runs):
        n = int(rng.integers(0, 600))
        if rng.random() < 0.1:
            n = 0  # empty run
        keys = sorted({pool[int(rng.integers(0, len(pool)))]
                       for _ in range(n)})
        ents = []
        for i, k in enumerate(keys):
            vmode = rng.random()
            if vmode < 0.25:
                data = b""  # tombstone
            else:
                data = bytes(rng.integers(0, 256,
                                          int(rng.integers(1, 300)),
                                          dtype=np.uint8))
            if ts_mode == 0:
                ts = (r << 40) + i  # monotone per run
            elif ts_mode == 1:
                ts = int(rng.integers(-100, 100))  # heavy collisions
            else:
                # full i128 range: compose from 128 random bits
                bits = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
                ts = int.from_bytes(bits, "little", signed=True)
            ents.append(Entry(k, data, ts))
        runs.append(build_run(ents))
    return runs


def random_scan_filter(rng):
    kw = {}
    if rng.random() < 0.5:
        kw["start_key"] = bytes(rng.integers(0, 256,
                                             int(rng.integers(0, 8)),
                                             dtype=np.uint8))
    if rng.random() < 0.5:
        kw["end_key"] = bytes(rng.integers(0, 256,
                                           int(rng.integers(0, 8)),
                                           dtype=np.uint8))
    if rng.random() < 0.7:
        n = int(rng.integers(1, 4))
        kw["hash_ranges"] = [
            (int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)))
            for _ in range(n)
        ]
    return kw


def reader_trial(rng, runs, device, mrng):
    """Resident reader vs the host model of the reference read path
    (highest run index wins, b"" = deleted, None = absent), with the
    engine's own filters on a random subset of the runs. Queries: stored
    keys, their one-byte mutations and extensions, and random keys. mrng is
    the get_merged step's own stream, so the other steps' draws stay what
    they were. Returns a mismatch description or None."""
    from dbeel_amd import lsm
    from dbeel_amd.engine import Job, Reader
    from dbeel_amd.format import parse_run

    model = {}
    for r, (d, i) in enumerate(runs):
        for e in parse_run(d, i):
            model[e.key] = (r, e.data)
    blooms = []
    for run in runs:
        if rng.random() < 0.6:
            with Job([run], device=device) as job:
                job.run(True)
                blooms.append(job.bloom())
        else:
            blooms.append(None)
    stored = list(model)
    queries = []
    for _ in range(int(rng.integers(0, 800))):
        pick = rng.random()
        k = stored[int(rng.integers(0, len(stored)))] if stored else b""
        if pick < 0.5:
            queries.append(k)
        elif pick < 0.65:
            queries.append(k + b"\x00")
        elif pick < 0.8 and k:
            queries.append(k[:-1] + bytes([k[-1] ^ 1]))
        elif pick < 0.9:
            queries.append(k[: len(k) // 2])
        else:
            queries.append(bytes(rng.integers(
                0, 256, int(rng.integers(0, 40)), dtype=np.uint8)))
    exp = [model[k][1] if k in model else None for k in queries]
    live_why = scan_why = None
    with Reader(runs, blooms=blooms, device=device) as rd:
        got = rd.get(queries)
        _, _, _, st = rd.get_raw(queries)
        scan_why = (get_entries_step(rng, rd, runs, queries)
                    or get_merged_step(mrng, rd, runs, queries, device)
                    or paged_scan_step(rng, rd, runs, stored)
                    or migrate_step(rng, rd, runs, device))
        if got == exp and not scan_why:
            live_why = live_reader_step(rng, rd, runs, blooms, queries,
                                        device)
    if scan_why or live_why:
        return scan_why or live_why
    if got != exp:
        bad = next(i for i, (g, e) in enumerate(zip(got, exp)) if g != e)
        return f"key {queries[bad].hex()} got {got[bad]} want {exp[bad]}"
    filtered = [b for b in blooms if b is not None]
    if len(filtered) == len(runs):
        if st["searches"] + st["bloom_skips"] != st["bloom_probes"]:
            return f"stats do not add up: {st}"
    # zero false negatives: a filter never hides a stored key
    for r, (d, i) in enumerate(runs):
        if blooms[r] is None:
            continue
        for e in parse_run(d, i)[::17]:
            if not lsm.bloom_contains(blooms[r], e.key):
                return f"filter of run {r} misses stored key {e.key.hex()}"
    return None


def get_entries_step(rng, rd, runs, queries):
    """get_entries of the open reader against tests/get_entries_model: one
    call at a random cap (hits, offsets, page and delivered bytes), then the
    paged loop at a random page size (data and timestamps)."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import get_entries_model as gem
    from dbeel_amd.engine import HIT_DTYPE, DbeelGpuError

    model = gem.Model(runs)
    ehits, eoff, erec, _, _ = model.expect(queries)
    cap = int(rng.integers(0, eoff[-1] + 2))
    _, _, _, erc, epage = model.expect(queries, cap)
    try:
        hits, roff, view, page, _ = rd.get_entries_raw(queries,
                                                       records_cap=cap)
        rc = 0
    except DbeelGpuError as e:
        rc, hits, roff, page = e.code, e.hits, e.record_offsets, e.page
        view = np.zeros(0, dtype=np.uint8)
    if rc != erc or page != epage:
        return f"get_entries cap {cap}: rc {rc} page {page}, want {erc} {epage}"
    if not np.array_equal(hits, gem.hits_array(ehits, HIT_DTYPE)):
        return f"get_entries cap {cap}: hits differ from the model"
    if roff.tolist() != eoff:
        return f"get_entries cap {cap}: record_offsets differ from the model"
    if view.tobytes() != erec[:epage["records_len"]]:
        return f"get_entries cap {cap}: record bytes differ from the model"
    page_bytes = int(rng.integers(0, 4096))
    if rd.get_entries(queries, page_bytes=page_bytes) != model.entries(queries):
        return f"get_entries page_bytes {page_bytes}: entries differ"
    return None


MERGED = {"calls": 0, "sources": 0}  # what the get_merged step compared


def get_merged_step(rng, rd, runs, queries, device):
    """get_merged of the open reader against tests/merge_model: 0..4 random
    sources — readers and answer pairs over random subsets of the reader's
    own runs (equal timestamps, so ties) and over fresh random runs drawn
    from the stored keys with random timestamps — one call at a random cap
    (hits, offsets, page and delivered bytes), then the paging loop."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import get_entries_model as gem
    import merge_model as mm
    from dbeel_amd.engine import MERGE_HIT_DTYPE, DbeelGpuError, Reader
    from dbeel_amd.format import parse_run

    stored = [e for d, i in runs for e in parse_run(d, i)]
    local = gem.Model(runs)
    readers, sources, msources = [], [], []
    try:
        for _ in range(int(rng.integers(0, 5))):
            if rng.random() < 0.5 or not stored:
                k = int(rng.integers(1, len(runs) + 1))
                sub = [runs[int(p)] for p in
                       sorted(rng.choice(len(runs), size=k, replace=False))]
            else:
                picks = {stored[int(j)].key: stored[int(j)] for j in
                         rng.integers(0, len(stored),
                                      int(rng.integers(1, 300)))}
                sub = [build_run([
                    Entry(key, b"" if rng.random() < 0.2 else e.data[::-1],
                          e.timestamp if rng.random() < 0.3 else
                          e.timestamp + int(rng.integers(-3, 4)) *
                          (1 << int(rng.integers(0, 100)))
                          if abs(e.timestamp) < (1 << 126) else e.timestamp)
                    for key, e in sorted(picks.items())])]
            m = gem.Model(sub)
            msources.append(m)
            if rng.random() < 0.5:
                readers.append(Reader(sub, device=device))
                sources.append(readers[-1])
            else:
                off, rec = mm.answers_of(m, queries)
                sources.append((np.array(off, dtype=np.uint64),
                                np.frombuffer(rec, dtype=np.uint8)))
        MERGED["calls"] += 1
        MERGED["sources"] += len(sources)
        ehits, eoff, erec, _, _ = mm.expect(queries, local, msources)
        cap = int(rng.integers(0, eoff[-1] + 2))
        _, _, _, erc, epage = mm.expect(queries, local, msources, cap)
        what = f"get_merged {len(sources)} sources cap {cap}"
        try:
            hits, roff, view, page, _ = rd.get_merged_raw(
                queries, sources, records_cap=cap)
            rc = 0
        except DbeelGpuError as e:
            rc, hits, roff, page = e.code, e.hits, e.record_offsets, e.page
            view = np.zeros(0, dtype=np.uint8)
        if rc != erc or page != epage:
            return f"{what}: rc {rc} page {page}, want {erc} {epage}"
        want = (np.array(ehits, dtype=MERGE_HIT_DTYPE) if ehits
                else np.zeros(0, dtype=MERGE_HIT_DTYPE))
        if not np.array_equal(hits, want):
            return f"{what}: hits differ from the model"
        if roff.tolist() != eoff:
            return f"{what}: record_offsets differ from the model"
        if view.tobytes() != erec[:epage["records_len"]]:
            return f"{what}: record bytes differ from the model"
        page_bytes = int(rng.integers(0, 4096))
        if (rd.get_merged(queries, sources, page_bytes=page_bytes)
                != mm.merged(queries, local, msources)):
            return f"{what}: paging loop at {page_bytes} differs"
    finally:
        for r in readers:
            r.close()
    return None


def paged_scan_step(rng, rd, runs, stored):
    """One paged scan of the open reader with random bounds (stored keys,
    their neighbours, random bytes), hash ranges, page capacities and
    candidate window, against the AsyncIter model."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from pymm3 import between_cmp, murmur3_32, scan_model

    from dbeel_amd.format import parse_run

    kw = random_scan_filter(rng)
    for side in ("start_key", "end_key"):
        if stored and rng.random() < 0.5:
            k = stored[int(rng.integers(0, len(stored)))]
            pick = rng.random()
            kw[side] = (k if pick < 0.5 else k + b"\x00" if pick < 0.75
                        else k[: len(k) // 2])
    md, mi, mn = scan_model(runs, **kw)
    biggest = max([32] + [len(d) for d, _ in runs])
    paging = dict(
        # never below the largest entry: 32 + 128 B key + 299 B value
        page_bytes=int(rng.integers(459, max(460, biggest))),
        page_entries=int(rng.integers(1, 700)),
        max_candidates=int(rng.choice([0, 1, 2, 63, 64, 65, 1000])),
        pinned=bool(rng.random() < 0.2))
    if paging["max_candidates"] == 1 and sum(len(i) for _, i in runs) > 16000:
        paging["max_candidates"] = 17  # keep the page count bounded
    gd, gi, gn, ids = rd.scan(return_range_ids=True, **kw, **paging)
    if (gd, gi, gn) != (md, mi, mn):
        return f"paged scan {kw} {paging}: n {gn} vs {mn}"
    ranges = kw.get("hash_ranges")
    if ranges:
        want = [next(j for j, (s, t) in enumerate(ranges)
                     if between_cmp(murmur3_32(e.key, 0), s, t))
                for e in parse_run(md, mi)]
        if ids.tolist() != want:
            return f"paged scan {kw} {paging}: range ids differ"
    return None


def migrate_step(rng, rd, runs, device):
    """One random migrate of the open reader (its memtable is empty here):
    random hash ranges with a random action each — skip, put into one of two
    destination readers, delete into the second — small random pages, plain
    or NEWEST_ONLY, either order path, against tests/migrate_model over the
    snapshot model's yield."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import migrate_model
    import snapshot_model
    from dbeel_amd.engine import SCAN_MEMTABLE, SCAN_NEWEST_ONLY, Reader

    if not any(len(i) for _, i in runs):
        return None
    n = int(rng.integers(1, 5))
    ranges = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)))
              for _ in range(n)]
    newest = bool(rng.integers(0, 2))
    dts = int(rng.integers(-2**62, 2**62))
    segs = snapshot_model.segments(runs)
    model = snapshot_model.snapshot_model(segs, hash_ranges=ranges,
                                          newest_only=newest)
    page = migrate_model.decode_page(model[0], model[1])
    rids = snapshot_model.first_range_ids(model, ranges)
    kinds = [("skip",), ("put", "A"), ("put", "B"), ("delete", "B")]
    named = [kinds[int(rng.integers(0, len(kinds)))] for _ in range(n)]
    want = migrate_model.migrate([(page, rids)], named, dts)
    order = ("radix", "merge")[int(rng.integers(0, 2))]
    paging = dict(page_bytes=int(rng.integers(459, 20000)),
                  max_candidates=int(rng.choice([0, 63, 64, 65, 1000])))
    what = f"migrate {ranges} {named} newest={newest} {paging} order={order}"
    nonempty = next(r for r in runs if len(r[1]))
    os.environ["DBEEL_BATCH_ORDER"] = order
    try:
        with Reader([nonempty], device=device) as A, \
                Reader([nonempty], device=device) as B:
            dst = {"A": A, "B": B}
            acts = [(a[0],) if a[0] == "skip" else (a[0], dst[a[1]])
                    for a in named]
            st = rd.migrate(acts, hash_ranges=ranges, delete_ts=dts,
                            flags=SCAN_MEMTABLE
                            | (SCAN_NEWEST_ONLY if newest else 0), **paging)
            if st["entries"] != len(page):
                return f"{what}: {st['entries']} entries, model {len(page)}"
            for name, r in dst.items():
                exp = want[name].run() if name in want else (b"", b"")
                if r.memtable_fetch() != exp:
                    return f"{what}: memtable of {name} differs from the model"
    finally:
        os.environ.pop("DBEEL_BATCH_ORDER", None)
    if rd.held_bytes:
        return f"{what}: {rd.held_bytes} bytes still held"
    return None


def write_batch_step(rng, rd, runs, blooms, queries):
    """One random write batch (arrival order, repeated keys drawn from the
    query set, tombstones, any timestamp; either order path) into the open
    reader at a random position, against the memtable model; runs and
    blooms are edited in place to the list the reader should now hold."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import batch_model

    pool = queries or [b"", b"k"]
    writes = []
    for _ in range(int(rng.integers(0, 400))):
        k = pool[int(rng.integers(0, len(pool)))]
        v = (b"" if rng.random() < 0.2 else bytes(rng.integers(
            0, 256, int(rng.integers(0, 80)), dtype=np.uint8)))
        writes.append((k, v, int(rng.integers(-2**62, 2**62))))
    pos = int(rng.integers(0, len(runs) + 1))
    with_bloom = bool(rng.integers(0, 2))
    order = ("radix", "merge")[int(rng.integers(0, 2))]
    os.environ["DBEEL_BATCH_ORDER"] = order
    try:
        gd, gi, gb, st = rd.write_batch(writes, pos=pos,
                                        build_bloom=with_bloom)
    finally:
        os.environ.pop("DBEEL_BATCH_ORDER", None)
    what = f"write batch of {len(writes)} at {pos} order={order}"
    if (gd, gi) != batch_model.flush_run(writes):
        return f"{what}: run differs from the memtable model"
    if st["prefix_tied"] != batch_model.prefix_tied(writes):
        return f"{what}: prefix_tied {st['prefix_tied']}"
    if writes:
        runs.insert(pos, (gd, gi))
        blooms.insert(pos, gb)
    return None


def live_reader_step(rng, rd, runs, blooms, queries, device):
    """One random insert, one random write batch and one random compaction
    applied to the open reader, each compared field for field against a freshly opened reader
    over the resulting list (the compaction's output from the oracle)."""
    from dbeel_amd.engine import Reader

    def differs(what):
        with Reader(runs, blooms=blooms, device=device) as fresh:
            got, want = rd.get_raw(queries), fresh.get_raw(queries)
        for f in ("run", "is_tombstone", "value_offset", "value_len"):
            if not np.array_equal(got[0][f], want[0][f]):
                return f"after {what}: hit field {f} differs from a reopen"
        if (not np.array_equal(got[1], want[1])
                or got[2].tobytes() != want[2].tobytes()):
            return f"after {what}: values differ from a reopen"
        return None

    runs, blooms = list(runs), list(blooms)
    if len(runs) < 64:
        new = random_runs(rng)[0]
        pos = int(rng.integers(0, len(runs) + 1))
        rd.insert_run(pos, new)
        runs.insert(pos, new)
        blooms.insert(pos, None)
        why = differs(f"insert at {pos}")
        if why:
            return why
    if len(runs) < 64:
        why = write_batch_step(rng, rd, runs, blooms, queries)
        if why:
            return why
        why = differs("write batch")
        if why:
            return why
    n = len(runs)
    k = int(rng.integers(1, n + 1))
    positions = sorted(int(p) for p in rng.choice(n, size=k, replace=False))
    out_pos = int(rng.integers(0, n - k + 1))
    keep = bool(rng.integers(0, 2))
    with_bloom = bool(rng.integers(0, 2))
    gd, gi, gb, _ = rd.compact(positions, out_pos, keep, bloom=with_bloom)
    od, oi, _ = oracle.compact([runs[p] for p in positions],
                               keep_tombstones=keep)
    what = f"compact {positions} -> {out_pos} keep={keep}"
    if (gd, gi) != (od, oi):
        return f"{what}: output differs from the oracle"
    chosen = set(positions)
    runs = [r for p, r in enumerate(runs) if p not in chosen]
    blooms = [b for p, b in enumerate(blooms) if p not in chosen]
    runs.insert(out_pos, (od, oi))
    blooms.insert(out_pos, gb)
    return differs(what)


def compact_into_step(rng, runs, keep, want, device):
    """compact_into at a random slice count (forced, or through a random
    budget), with and without the filter, against compact()'s result and
    the whole job's filter. Returns a mismatch description or None."""
    from dbeel_amd.engine import Job, compact_into

    data = np.empty(sum(len(d) for d, _ in runs) + 1, dtype=np.uint8)
    index = np.empty(sum(len(i) for _, i in runs) + 1, dtype=np.uint8)
    total = len(data) + len(index)
    kw = ({"n_slices": int(rng.integers(1, 20))} if rng.random() < 0.7
          else {"max_resident_bytes": int(rng.integers(1, total + 1))})
    bloom = bool(rng.integers(0, 2))
    dl, il, n, st, gb = compact_into(runs, keep, data, index, device=device,
                                     bloom=bloom, **kw)
    got = (data[:dl].tobytes(), index[:il].tobytes(), n)
    if got != tuple(want):
        return f"{kw}: n {n} vs {want[2]} in {st['slices']} slices"
    if bloom:
        with Job(runs, device=device) as job:
            job.run(keep)
            if job.bloom() != gb:
                return f"{kw}: filter differs from the whole job's"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scan", action="store_true",
                    help="also fuzz dbeel_gpu_scan vs the AsyncIter model")
    ap.add_argument("--reader", action="store_true",
                    help="also fuzz the resident reader vs the host model "
                         "of the read path")
    args = ap.parse_args()

    if args.scan:
        sys.path.insert(0, os.path.join(
            os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
        from pymm3 import scan_model

        from dbeel_amd.engine import scan as gpu_scan

    failures = 0
    for t in range(args.trials):
        rng = np.random.default_rng(args.seed * 1_000_003 + t)
        runs = random_runs(rng)
        # its own stream: the draws of the older steps stay what they were
        srng = np.random.default_rng([args.seed, t, 0x51])
        for keep in (True, False):
            od, oi, on = oracle.compact(runs, keep_tombstones=keep)
            gd, gi, gn = dbeel_amd.compact(runs, keep_tombstones=keep,
                                           device=args.device)
            if (gd, gi, gn) != (od, oi, on):
                failures += 1
                print(f"TRIAL {t} keep={keep} MISMATCH: "
                      f"n {gn} vs {on}, index {gi == oi}, data {gd == od}")
            why = compact_into_step(srng, runs, keep, (gd, gi, gn),
                                    args.device)
            if why:
                failures += 1
                print(f"TRIAL {t} keep={keep} COMPACT_INTO MISMATCH: {why}")
        if args.scan:
            kw = random_scan_filter(rng)
            sd, si, sn = gpu_scan(runs, device=args.device, **kw)
            md, mi, mn = scan_model(runs, **kw)
            if (sd, si, sn) != (md, mi, mn):
                failures += 1
                print(f"TRIAL {t} SCAN MISMATCH {kw}: n {sn} vs {mn}")
        if args.reader:
            why = reader_trial(rng, runs, args.device,
                               np.random.default_rng([args.seed, t, 0x4D]))
            if why:
                failures += 1
                print(f"TRIAL {t} READER MISMATCH: {why}")
        if (t + 1) % 25 == 0:
            print(f"{t + 1}/{args.trials} trials OK")
    if failures:
        print(f"FUZZ FAILED: {failures} mismatches")
        sys.exit(1)
    if args.reader:
        print(f"get_merged: {MERGED['calls']} batches against the model, "
              f"{MERGED['sources']} sources in all")
    print(f"FUZZ OK: {args.trials} trials x 2 settings, all bit-identical")


if __name__ == "__main__":
    main()
