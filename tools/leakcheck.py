#!/usr/bin/env python3
"""Device-memory stability check: churn job create/run/fetch/destroy,
streamed ingests (each creates ~per-chunk HIP events), batched jobs,
scans, sliced compactions and resident readers (open / get x N / get_entries
at three page sizes / compact begin + compact_fetch x 2 into caller buffers +
abort / paged
scans begin + next + end, one left for close to end / insert / compact
begin + abort + commit / write batches with fetch on and off, a filter,
both order paths and a refused call / memtable put x N + get + fetch +
flush + clear, with the storage pair checked never to shrink nor to regrow
after a flush / snapshot scans begun, paged and ended across an insert, two
puts and a compaction, one left for close / close with a non-empty
memtable / put_entries of a host page, a refused corrupt page, scan_apply
into a second reader with deletes back into the source, flushes, close with
that scan open / get_merged with 0, 1 and 3 sources, one of them a reader,
at two page sizes, and a refused corrupt answer) and compact_into (1 and several slices, pinned and pageable
destinations, with and without the filter, a refused short cap, a job's
fetch_into), reporting hipMemGetInfo drift. A leak in any path shows as monotonically shrinking free memory.

    python tools/leakcheck.py --iters 40
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import dbeel_amd  # noqa: E402
from dbeel_amd.engine import (  # noqa: E402
    BatchJob,
    DbeelGpuError,
    Job,
    Reader,
    compact_into,
    compact_sliced,
    flush_batch,
    load,
    pin_host,
    scan,
    unpin_host,
)
from dbeel_amd.genruns import make_runs  # noqa: E402


def free_mem():
    lib = ctypes.CDLL("libamdhip64.so")
    free = ctypes.c_size_t()
    total = ctypes.c_size_t()
    lib.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return int(free.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    load()

    runs = make_runs(4, 20_000, 16, 256, overlap_frac=0.4,
                     tombstone_frac=0.1, seed=77)
    runs2 = make_runs(4, 20_000, 16, 256, overlap_frac=0.4,
                      tombstone_frac=0.1, seed=78)
    # equal shapes for ingest (tombstone draws differ -> regenerate
    # without tombstones for the ingest pair)
    ri_a = make_runs(3, 15_000, 16, 128, overlap_frac=0.3, seed=80)
    ri_b = make_runs(3, 15_000, 16, 128, overlap_frac=0.3, seed=81)
    for d, i in ri_b:
        pin_host(d)
        pin_host(i)
    # caller buffers of compact_fetch: the data one pinned
    fetch_d = np.empty(sum(d.nbytes for d, _ in runs), dtype=np.uint8)
    fetch_i = np.empty(sum(i.nbytes for _, i in runs), dtype=np.uint8)
    pin_host(fetch_d)

    probe_rng = np.random.default_rng(5)
    probe_keys = [bytes(probe_rng.integers(0, 256, 16, dtype=np.uint8))
                  for _ in range(10_000)]
    for d, i in runs:  # half present, half absent
        recs = np.frombuffer(i, dtype="<u8").reshape(-1, 2)[:2500, 0]
        probe_keys += [d[int(o) + 8 : int(o) + 24].tobytes() for o in recs]

    # an unsorted write batch with repeated keys, shared 8-byte prefixes
    # among them (the settle stage allocates only then)
    batch = [(k if j % 3 else b"user:000" + k[:5],
              bytes(probe_rng.integers(0, 256, j % 97, dtype=np.uint8)), j)
             for j, k in enumerate(probe_keys + probe_keys[:5000])]

    os.environ["DBEEL_STREAM_CHUNK_MB"] = "1"
    base = None
    total_in = sum(d.nbytes + i.nbytes for d, i in runs)
    try:
        for it in range(args.iters):
            # plain compact (job create/run/fetch/destroy)
            dbeel_amd.compact(runs, keep_tombstones=False, device=0)
            # resident job + ingest churn
            with Job(ri_a, device=0) as job:
                job.ingest(ri_b)
                job.run(False)
                job.fetch()
            # batched
            with BatchJob([runs, runs2], device=0) as bj:
                bj.run(True)
                bj.fetch_job(1)
            # scan + sliced
            scan(runs, hash_ranges=[(0, 1 << 31)], device=0)
            compact_sliced(runs, keep_tombstones=True, device=0,
                           max_resident_bytes=total_in // 3)
            # resident reader: open / get x N (scratch regrowth) / close
            with Job(runs[:1], device=0) as job:
                job.run(True)
                bloom0 = job.bloom()
            with Reader(runs, blooms=[bloom0, None, None, None],
                        device=0) as rd:
                for n in (10, 4000, 100, 20_000):
                    rd.get(probe_keys[:n])
                # get_entries at three caps: one page, a few pages, many
                # (the record scratch is sized by each page, shared with
                # get, and regrows); the results live in caller memory
                for n, cap in ((20_000, 64 << 20), (20_000, 1 << 20),
                               (2000, 1 << 10)):
                    rd.get_entries(probe_keys[:n], page_bytes=cap)
                # compact_fetch: the pending table copied out twice into
                # caller buffers, one pinned, and a refused short one
                rd.compact_begin([1, 2], True, fetch=False)
                try:
                    rd.compact_fetch_into(fetch_d[:8], fetch_i)
                    raise SystemExit("compact_fetch accepted a short buffer")
                except DbeelGpuError:
                    pass
                for _ in range(2):
                    rd.compact_fetch_into(fetch_d, fetch_i)
                rd.compact_abort()
                # paged scans: begin / next x N / end with growing and
                # shrinking windows and page buffers (scratch regrowth), a
                # pinned one, and one abandoned mid-way for close to end
                for pb, pe, mc in ((1 << 16, 100, 1000), (1 << 22, 50_000, 0),
                                   (1 << 14, 7, 64)):
                    for page in rd.scan_pages(hash_ranges=[(0, 1 << 30)],
                                              page_bytes=pb, page_entries=pe,
                                              max_candidates=mc):
                        if mc == 64 and page[2]:
                            break  # generator closed early: scan_end
                rd.scan(start_key=b"\x40", page_bytes=1 << 20, pinned=True)
                abandoned = rd.scan_open(end_key=b"\xc0", max_candidates=500)
                abandoned.next(np.empty(1 << 16, dtype=np.uint8),
                               np.empty(16 * 64, dtype=np.uint8))
                # live updates: insert / compact / abort / commit — every
                # table they allocate is freed by the swap or by close
                rd.insert_run(2, runs2[0])
                rd.compact_begin([0, 2], True, bloom=True)
                rd.compact_abort()
                rd.compact([1, 3, 4], 0, False, bloom=True)
                rd.compact_begin([0, 1], True, fetch=False)  # close aborts
                # write batches: staging, sort scratch and pinned record
                # are the call's; the tables go with close
                for fetch, bloom in ((True, True), (False, False)):
                    rd.write_batch(batch, build_bloom=bloom, fetch=fetch)
                os.environ["DBEEL_BATCH_ORDER"] = "radix"
                rd.write_batch(batch[::3], pos=0)
                del os.environ["DBEEL_BATCH_ORDER"]
                try:
                    rd.write_batch(batch, pos=99)  # fails before the device
                    raise SystemExit("write_batch accepted a bad position")
                except DbeelGpuError:
                    pass
                rd.get(probe_keys[:4000])
                # resident memtable: put x N (the ping-pong pair grows in
                # the first iteration's first puts only — a reader is new
                # each iteration, so its growth recurs but is freed by
                # close) / get / fetch / flush / clear, and close with a
                # non-empty memtable
                reserved = 0
                for lo in range(0, len(batch), 4000):
                    rd.put(batch[lo:lo + 4000])
                    now = rd.memtable_info["reserved_bytes"]
                    if now < reserved:
                        raise SystemExit("memtable storage shrank")
                    reserved = now
                rd.get(probe_keys[:4000])
                rd.memtable_fetch()
                rd.memtable_flush(build_bloom=True)
                rd.put(batch[:3000])
                rd.memtable_clear()
                rd.put(batch[::2])
                if rd.memtable_info["reserved_bytes"] != reserved:
                    raise SystemExit("memtable storage regrew after a flush")
                rd.get(probe_keys[:1000])
                # snapshot scans: begin, edit the list and the memtable
                # under them, page, end — what the list and the pair let go
                # of is freed by the last scan's end, or by close for the
                # one left open
                page = (np.empty(1 << 20, dtype=np.uint8),
                        np.empty(16 * 4096, dtype=np.uint8))
                snaps = [rd.snapshot_open(memtable=True, newest_only=True,
                                          max_candidates=4096),
                         rd.snapshot_open(memtable=True),
                         rd.snapshot_open(end_key=b"\x80", memtable=True)]
                snaps[0].next(*page)
                rd.compact_abort()  # the one pending from above
                rd.insert_run(0, runs2[1])
                rd.put(batch[:2000])
                rd.put(batch[2000:4000])  # displaces the held buffer
                rd.compact([1, 2], 1, True, fetch=False)
                if not rd.held_bytes:
                    raise SystemExit("nothing held after compact + puts")
                for sc in snaps[:2]:
                    while not sc.next(*page)["done"]:
                        pass
                    sc.close()
                if not rd.held_bytes:
                    raise SystemExit("the open snapshot holds nothing")
                rd.compact_begin([0, 1], True, fetch=False)
                # close aborts that, ends snaps[2] and frees the memtable
            # migration inside HBM: a host page through put_entries, a
            # refused corrupt page, scan pages applied into a second reader
            # and as deletes back into the source (staging and merge scratch
            # are each call's; the displaced memtable buffer is the scan's),
            # both memtables flushed, and close with the scan still open
            with Reader(runs[:2], device=0) as src, \
                    Reader(runs2[:1], device=0) as dst:
                pd, px, _ = src.scan(end_key=b"\x20", page_bytes=1 << 22)
                pd = np.frombuffer(pd, dtype=np.uint8)
                px = np.frombuffer(px, dtype=np.uint8).copy()
                dst.put_entries(pd, px)
                bad = px.copy()
                bad[16 + 8:16 + 12] = 0  # key_size 0 in the second record
                try:
                    dst.put_entries(pd, bad)
                    raise SystemExit("put_entries accepted a corrupt page")
                except DbeelGpuError:
                    pass
                halves = [(0, 1 << 31), (1 << 31, 0xFFFFFFFF)]
                src.put(batch[:3000])
                mig = src.snapshot_open(hash_ranges=halves, memtable=True,
                                        max_candidates=6000)
                for _ in range(4):
                    mig.apply([("put", dst), ("delete", src)], 1 << 20,
                              delete_ts=it)
                if not src.held_bytes:
                    raise SystemExit("deletes displaced no held buffer")
                dst.memtable_flush(fetch=False)
                src.memtable_flush(fetch=False)
                # close ends mig and frees what it holds
            # replicated reads: get_merged with 0, 1 and 3 sources, one of
            # them a reader, at two page sizes (candidate, answer and record
            # scratch are the local reader's and regrow), and one corrupt
            # answer refused on the device
            with Reader(runs[:2], device=0) as loc, \
                    Reader(runs[2:], device=0) as rep, \
                    Reader(runs2[:2], device=0) as rep2:
                mk = probe_keys[:20_000]
                a1 = tuple(x.copy() for x in rep.get_entries_raw(mk)[1:3])
                a2 = tuple(x.copy() for x in rep2.get_entries_raw(mk)[1:3])
                for srcs in ([], [a1], [a1, rep2, a2]):
                    for cap in (64 << 20, 1 << 18):
                        loc.get_merged(mk, srcs, page_bytes=cap)
                bad = a1[1].copy()
                bad[:8] = 0xFF  # the first record's data_len
                try:
                    loc.get_merged_raw(mk, [rep2, (a1[0], bad)])
                    raise SystemExit("get_merged accepted a corrupt answer")
                except DbeelGpuError as e:
                    if e.code != 2:
                        raise
            # compact_into: jobs, events, the hash array and the filter
            # bitmap are the call's; pinned (data) and pageable (index)
            # destinations, 1 and several slices, with and without the
            # filter, and a refused short cap that still runs every slice
            for n_slices, bloom in ((1, False), (1, True), (5, True),
                                    (9, False)):
                compact_into(runs, False, fetch_d, fetch_i, device=0,
                             n_slices=n_slices, bloom=bloom)
            compact_into(runs, True, fetch_d, fetch_i, device=0,
                         max_resident_bytes=total_in // 3, bloom=True)
            try:
                compact_into(runs, True, fetch_d[:4096], fetch_i, device=0,
                             n_slices=4, bloom=True)
                raise SystemExit("compact_into accepted a short buffer")
            except DbeelGpuError:
                pass
            with Job(runs, device=0) as job:
                job.run(False)
                job.fetch_into(fetch_d, fetch_i, index_base=1 << 33)
            flush_batch(batch[:7000], device=0)
            f = free_mem()
            if base is None:
                base = f
            drift = base - f
            if it % 5 == 4 or it == args.iters - 1:
                print(f"iter {it + 1}/{args.iters}: free={f / 1e9:.3f} GB "
                      f"drift={drift / 1e6:.1f} MB")
            if drift > 512 * 1024 * 1024:
                print("LEAKCHECK FAILED: device memory drift "
                      f"{drift / 1e6:.1f} MB after {it + 1} iters")
                sys.exit(1)
    finally:
        for d, i in ri_b:
            unpin_host(d)
            unpin_host(i)
        unpin_host(fetch_d)
        os.environ.pop("DBEEL_STREAM_CHUNK_MB", None)
    print(f"LEAKCHECK OK: {args.iters} iterations across every API path, "
          f"drift {(base - free_mem()) / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
