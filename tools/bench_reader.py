#!/usr/bin/env python3
"""Resident-reader benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B
keys, 1 KiB values): one 1 M-key batch, half present and half absent.

Records, per batch and timed at the C ABI (no Python list building):
  - the reader's search_ms / gather_ms (HIP events) and wall, opened with
    and without the runs' filters;
  - the wall of the old dbeel_gpu_lookup on the same inputs (it uploads
    every run and builds a compaction job per call, and returns hit
    records only — no value bytes).
and checks that all three paths return identical hit records.

    python tools/bench_reader.py                  # -> profiles/reader_cfg3.json

--entries measures only dbeel_gpu_reader_get (the baseline) against
dbeel_gpu_reader_get_entries into a pageable buffer, into a pinned buffer and
as a call-again loop with a pinned 64 MiB page, interleaved:

    python tools/bench_reader.py --entries  # -> profiles/reader_get_entries.json

Kernel times of the old and the new search kernel come from a profiler
run of their own (tracing slows the host, so never mixed with the walls):

    rocprofv3 --kernel-trace --stats -d OUT -o reader -- \\
        python tools/bench_reader.py --profile-pass
    python tools/bench_reader.py --kernel-stats OUT/.../reader_kernel_stats.csv
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

from dbeel_amd import engine  # noqa: E402
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_cfg3.json")
ENTRIES_OUT = os.path.join(REPO, "profiles", "reader_get_entries.json")
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)


def make_queries(runs, n_keys, key_size, seed):
    """(n_keys, key_size) u8 matrix: half drawn from the stored entries
    (uniform over runs and positions), half random (absent with
    overwhelming probability at 32 B), shuffled."""
    rng = np.random.default_rng(seed)
    n_present = n_keys // 2
    keys = rng.integers(0, 256, (n_keys, key_size), dtype=np.uint8)
    which = rng.integers(0, len(runs), n_present)
    col = np.arange(key_size, dtype=np.int64)[None, :]
    for r, (data, index) in enumerate(runs):
        sel = np.flatnonzero(which == r)
        offs = np.frombuffer(index, dtype="<u8").reshape(-1, 2)[:, 0]
        pick = offs[rng.integers(0, len(offs), len(sel))].astype(np.int64)
        keys[sel] = data[pick[:, None] + 8 + col]
    keys = keys[rng.permutation(n_keys)]
    return np.ascontiguousarray(keys)


class Batch:
    def __init__(self, keys):
        n, k = keys.shape
        self.n = n
        self.blob = keys.reshape(-1)
        self.off = np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
        self.blob_p = self.blob.ctypes.data_as(U8P)
        self.off_p = self.off.ctypes.data_as(U64P)


def reader_get(lib, rd, batch):
    """One dbeel_gpu_reader_get; -> (wall_ms, stats dict, hits copy)."""
    res = engine.GetResult()
    st = engine.GetStats()
    t0 = time.perf_counter()
    rc = lib.dbeel_gpu_reader_get(rd._h, batch.blob_p, batch.off_p, batch.n,
                                  ctypes.byref(res), ctypes.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    hits = np.empty(batch.n, dtype=engine.HIT_DTYPE)
    ctypes.memmove(hits.ctypes.data, res.hits,
                   batch.n * engine.HIT_DTYPE.itemsize)
    values_len = int(res.values_len)
    lib.dbeel_gpu_get_result_free(ctypes.byref(res))
    d = st.as_dict()
    d["values_len"] = values_len
    return wall, d, hits


def old_lookup(lib, views, n_runs, batch, device):
    hits = np.zeros(batch.n, dtype=engine.HIT_DTYPE)
    t0 = time.perf_counter()
    rc = lib.dbeel_gpu_lookup(views, n_runs, batch.blob_p, batch.off_p,
                              batch.n, device,
                              hits.ctypes.data_as(
                                  ctypes.POINTER(engine.LookupHit)))
    wall = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    return wall, hits


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def bench_reader(lib, runs, blooms, batch, device, warmup, reps):
    t0 = time.perf_counter()
    rd = engine.Reader(runs, blooms=blooms, device=device)
    open_ms = (time.perf_counter() - t0) * 1e3
    with rd:
        for _ in range(warmup):
            reader_get(lib, rd, batch)
        walls, search, gather, h2d, d2h = [], [], [], [], []
        for _ in range(reps):
            wall, st, hits = reader_get(lib, rd, batch)
            walls.append(wall)
            search.append(st["search_ms"])
            gather.append(st["gather_ms"])
            h2d.append(st["h2d_ms"])
            d2h.append(st["d2h_ms"])
        out = {
            "open_ms": open_ms,
            "table_bytes": rd.table_bytes,
            "wall_ms": summarize(walls),
            "search_ms": summarize(search),
            "gather_ms": summarize(gather),
            "h2d_ms": summarize(h2d),
            "d2h_ms": summarize(d2h),
            "counters": {k: st[k] for k in (
                "bloom_probes", "bloom_skips", "searches", "hits",
                "tombstones", "values_len")},
        }
    return out, hits


class EntryBuffers:
    """Caller-owned buffers of one dbeel_gpu_reader_get_entries call."""

    def __init__(self, n, cap, pinned):
        self.hits = np.empty(n, dtype=engine.HIT_DTYPE)
        self.roff = np.empty(n + 1, dtype=np.uint64)
        self.rec = np.empty(max(cap, 1), dtype=np.uint8)
        self.rec[:] = 0  # touched: no first-use page faults in the samples
        self.cap = cap
        self.pinned = pinned
        if pinned:
            for a in (self.hits, self.roff, self.rec):
                engine.pin_host(a)

    def buf(self, first_key=0):
        return engine.GetBuffers(
            self.hits[first_key:].ctypes.data_as(
                ctypes.POINTER(engine.LookupHit)),
            self.roff[first_key:].ctypes.data_as(U64P),
            self.rec.ctypes.data_as(U8P), self.cap)

    def release(self):
        if self.pinned:
            for a in (self.hits, self.roff, self.rec):
                engine.unpin_host(a)


def get_entries(lib, rd, batch, bufs, first_key=0):
    """One dbeel_gpu_reader_get_entries over keys [first_key, n);
    -> (rc, wall_ms, stats dict, page dict)."""
    b = bufs.buf(first_key)
    page = engine.GetPage()
    st = engine.GetStats()
    key_bytes = int(batch.off[1])  # fixed-width keys: offsets stay from 0
    blob_p = ctypes.cast(ctypes.addressof(batch.blob_p.contents)
                         + first_key * key_bytes, U8P)
    t0 = time.perf_counter()
    rc = lib.dbeel_gpu_reader_get_entries(
        rd._h, blob_p, batch.off_p, batch.n - first_key, ctypes.byref(b),
        ctypes.byref(page), ctypes.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    return rc, wall, st.as_dict(), page.as_dict()


def paged_loop(lib, rd, batch, bufs, check_against=None):
    """The call-again loop over the whole batch with a bufs.cap-byte page;
    -> summed wall / stats and the number of calls."""
    tot = {"wall_ms": 0.0, "search_ms": 0.0, "gather_ms": 0.0, "d2h_ms": 0.0,
           "h2d_ms": 0.0, "calls": 0, "bytes": 0}
    done = 0
    while done < batch.n:
        rc, wall, st, page = get_entries(lib, rd, batch, bufs, done)
        if rc != 0:
            raise engine.DbeelGpuError(rc,
                                       lib.dbeel_gpu_last_error().decode())
        if check_against is not None:
            lo = tot["bytes"]
            assert np.array_equal(bufs.rec[:page["records_len"]],
                                  check_against[lo:lo + page["records_len"]])
        tot["wall_ms"] += wall
        for k in ("search_ms", "gather_ms", "d2h_ms", "h2d_ms"):
            tot[k] += st[k]
        tot["calls"] += 1
        tot["bytes"] += page["records_len"]
        done += page["n_done"]
    return tot


def bench_get_entries(lib, runs, batch, device, warmup, reps, page_bytes):
    """reader_get (the untouched baseline) against get_entries into a
    pageable and into a pinned buffer of records_total bytes, and the
    call-again loop with a pinned page_bytes page — interleaved round by
    round."""
    fields = ("wall_ms", "search_ms", "gather_ms", "d2h_ms", "h2d_ms")
    paths = ("reader_get", "entries_pageable", "entries_pinned",
             "entries_paged_loop")
    samples = {p: {f: [] for f in fields} for p in paths}
    with engine.Reader(runs, device=device) as rd:
        probe = EntryBuffers(batch.n, 0, False)
        rc, _, _, page = get_entries(lib, rd, batch, probe)
        assert rc in (0, 3), rc
        total = page["records_total"]
        pageable = EntryBuffers(batch.n, total, False)
        pinned = EntryBuffers(batch.n, total, True)
        loop = EntryBuffers(batch.n, page_bytes, True)
        try:
            checks = {}
            for rnd in range(warmup + reps):
                wall, st, hits = reader_get(lib, rd, batch)
                st["wall_ms"] = wall
                got = {"reader_get": st}
                for name, bufs in (("entries_pageable", pageable),
                                   ("entries_pinned", pinned)):
                    rc, wall, st_e, page = get_entries(lib, rd, batch, bufs)
                    if rc != 0:
                        raise engine.DbeelGpuError(
                            rc, lib.dbeel_gpu_last_error().decode())
                    assert page["n_done"] == batch.n
                    st_e["wall_ms"] = wall
                    got[name] = st_e
                first = rnd == 0
                got["entries_paged_loop"] = paged_loop(
                    lib, rd, batch, loop, pinned.rec if first else None)
                if first:
                    checks["hits_equal_reader_get"] = bool(
                        np.array_equal(pageable.hits, hits)
                        and np.array_equal(pinned.hits, hits))
                    checks["records_pageable_equal_pinned"] = bool(
                        np.array_equal(pageable.rec, pinned.rec)
                        and np.array_equal(pageable.roff, pinned.roff))
                    checks["loop_bytes_equal_one_shot"] = bool(
                        got["entries_paged_loop"]["bytes"] == total)
                    checks["counters_equal_reader_get"] = all(
                        got["reader_get"][k] == got["entries_pinned"][k]
                        for k in ("bloom_probes", "bloom_skips", "searches",
                                  "hits", "tombstones"))
                    values_len = got["reader_get"]["values_len"]
                    loop_calls = got["entries_paged_loop"]["calls"]
                if rnd < warmup:
                    continue
                for p in paths:
                    for f in fields:
                        samples[p][f].append(got[p][f])
        finally:
            for b in (pinned, loop):
                b.release()
    return {
        "records_total": total, "values_len": values_len,
        "records_over_values": total / values_len if values_len else None,
        "page_bytes": page_bytes, "paged_loop_calls": loop_calls,
        "pinned_buffers": "hits, record_offsets and records",
        "paths": {p: {f: summarize(samples[p][f]) for f in fields}
                  for p in paths},
        "checks": checks,
    }


def run_bloom(run, device):
    with engine.Job([run], device=device) as job:
        job.run(True)
        return job.bloom()


def merge_kernel_stats(csv_path, out_path):
    """Fold a rocprofv3 --kernel-trace --stats CSV (Name, Calls,
    TotalDurationNs, AverageNs, ...) into the results file."""
    want = {"k_lookup": "k_lookup", "k_reader_search": "k_reader_search",
            "k_reader_gather": "k_reader_gather"}
    found = {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if name.startswith("void "):  # a template instantiation
                name = name[5:]
            for key, label in want.items():
                if name.startswith((key + "(", key + "<")) or name == key:
                    found[label] = {
                        "calls": int(row["Calls"]),
                        "avg_ms": float(row["AverageNs"]) / 1e6,
                        "min_ms": float(row["MinNs"]) / 1e6,
                        "max_ms": float(row["MaxNs"]) / 1e6,
                    }
    res = json.load(open(out_path))
    res["kernel_trace"] = {
        "source": "rocprofv3 --kernel-trace --stats, a run of its own",
        "kernels": found,
    }
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--profile-pass", action="store_true",
                    help="one old lookup + reader gets with and without "
                         "filters, nothing written: the program to put "
                         "under the kernel tracer")
    ap.add_argument("--entries", action="store_true",
                    help="only reader_get against get_entries (pageable, "
                         "pinned, paged loop) -> "
                         "profiles/reader_get_entries.json")
    ap.add_argument("--page-mb", type=int, default=64,
                    help="page of the --entries call-again loop, MiB")
    ap.add_argument("--kernel-stats", metavar="CSV",
                    help="merge a kernel-stats CSV into --out and exit")
    args = ap.parse_args()

    if args.kernel_stats:
        merge_kernel_stats(args.kernel_stats, args.out)
        return

    lib = engine._load_reader()
    lib.dbeel_gpu_lookup.restype = ctypes.c_int
    lib.dbeel_gpu_lookup.argtypes = [
        ctypes.POINTER(engine.RunView), ctypes.c_size_t, U8P, U64P,
        ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(engine.LookupHit),
    ]

    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    batch = Batch(make_queries(runs, args.keys, 32, seed=0xBEAD))
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    input_bytes = sum(d.nbytes + i.nbytes for d, i in runs)
    views, keepalive = engine._views(runs)

    if args.entries:
        out = (ENTRIES_OUT if args.out == DEFAULT_OUT else args.out)
        res = {
            "workload": "cfg3", "scale": args.scale, "n_runs": len(runs),
            "input_bytes": input_bytes, "batch_keys": args.keys,
            "present_frac": 0.5, "warmup": args.warmup, "reps": args.reps,
            "method": "interleaved round by round; wall at the C ABI call, "
                      "the rest HIP events; paged loop = sums over its calls",
            **bench_get_entries(lib, runs, batch, args.device, args.warmup,
                                args.reps, args.page_mb << 20),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
        print(json.dumps(res))
        if not all(res["checks"].values()):
            sys.exit("get_entries disagrees with reader_get or with itself")
        return

    if args.profile_pass:
        old_lookup(lib, views, len(runs), batch, args.device)
        blooms = [run_bloom(r, args.device) for r in runs]
        for b in (None, blooms):
            with engine.Reader(runs, blooms=b, device=args.device) as rd:
                reader_get(lib, rd, batch)
        print("profile pass done")
        return

    blooms = [run_bloom(r, args.device) for r in runs]
    print("filters built", flush=True)
    plain, hits_plain = bench_reader(lib, runs, None, batch, args.device,
                                     args.warmup, args.reps)
    print("reader (no filters):", json.dumps(plain), flush=True)
    filt, hits_filt = bench_reader(lib, runs, blooms, batch, args.device,
                                   args.warmup, args.reps)
    print("reader (filters):", json.dumps(filt), flush=True)

    old_lookup(lib, views, len(runs), batch, args.device)  # warm-up
    old_walls = []
    for _ in range(args.old_reps):
        wall, hits_old = old_lookup(lib, views, len(runs), batch,
                                    args.device)
        old_walls.append(wall)
    same = bool(np.array_equal(hits_plain, hits_old)
                and np.array_equal(hits_filt, hits_old))

    res = {
        "workload": "cfg3", "scale": args.scale,
        "n_runs": len(runs), "entries": sum(i.nbytes // 16 for _, i in runs),
        "input_bytes": input_bytes, "bloom_bytes": sum(map(len, blooms)),
        "batch_keys": args.keys, "present_frac": 0.5,
        "timed_at": "C ABI call (wall), HIP events (search/gather)",
        "reader_no_bloom": plain,
        "reader_bloom": filt,
        "old_lookup_wall_ms": summarize(old_walls),
        "hits_identical_across_paths": same,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({"old_lookup_wall_ms": res["old_lookup_wall_ms"],
                      "hits_identical_across_paths": same}))
    if not same:
        sys.exit("hit records differ between the old and the new path")
    del keepalive


if __name__ == "__main__":
    main()
