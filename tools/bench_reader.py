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
