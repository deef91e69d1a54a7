#!/usr/bin/env python3
"""Resident-memtable benchmark, timed at the C ABI (wall clock around the
calls, which end synchronised; HIP-event stage times from the stats).

  put    dbeel_gpu_reader_put of an unsorted batch (8,192 and 2^20 writes,
         32-B keys, 1 KiB values, 10 % rewrites; random prefixes and
         all-shared prefixes) into a memtable holding 0 and 2^20 entries,
         against what the engine offered before for the same batch:
         dbeel_gpu_reader_write_batch(pos = n_runs, out = NULL). No
         threshold: both and the ratio are recorded — the merge is O(m + b)
         bandwidth work by design, and its cost at m = 2^20 is what a caller
         needs to pick a capacity.
  flush  dbeel_gpu_reader_memtable_flush(out = NULL) of that memtable,
         against write_batch of the concatenated arrivals.
  get    the one pass/fail timing: the get path must not pay for an EMPTY
         memtable. --parent-lib names the parent commit's library (built from
         a git worktree into a separate .so); its reader and this build's are
         opened over tools/bench_reader.py's cfg3 runs and alternated on the
         1 M-key batch in one process. Accepted when this build's median
         search_ms (HIP events) lies inside the parent's own min-max over the
         same repetitions. Both sets of samples are written out.
  get_nonempty  search_ms over cfg3 with 8,192 writes held in the memtable,
         against the same writes held as a 9th table. Recorded, no
         threshold.

One warm-up round, then --reps interleaved rounds; median / min / max.

    python tools/bench_reader_memtable.py --parts put,flush
    python tools/bench_reader_memtable.py --parts get --parent-lib PARENT.so
        # -> profiles/reader_memtable.json (parts merge into the file)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_reader  # noqa: E402
import bench_reader_write as brw  # noqa: E402
from dbeel_amd import engine  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_memtable.json")
PREFILL = 1 << 20


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def make_arrivals(n, shared, seed, prefill):
    """A batch as bench_reader_write makes it (10 % of its writes rewrite an
    earlier one); with a prefill, a further 10 % rewrite keys the memtable
    already holds."""
    batch, _ = brw.make_batch(n, shared, seed)
    if prefill is not None:
        rng = np.random.default_rng(seed + 1)
        rows = rng.choice(n, size=max(1, n // 10), replace=False)
        batch.keys[rows] = prefill.keys[rng.integers(0, prefill.n, len(rows))]
    return batch


def concat(a, b):
    return brw.Arrays(np.concatenate([a.keys, b.keys]),
                      np.concatenate([a.vals, b.vals]),
                      np.concatenate([a.ts[:, 0], b.ts[:, 0]]))


def put(lib, h, arrays):
    st = engine.MemtablePutStats()
    t0 = brw.now_ms()
    rc = lib.dbeel_gpu_reader_put(h, *arrays.args(), ctypes.byref(st))
    t1 = brw.now_ms()
    brw.check(lib, rc)
    return {"total": t1 - t0, **st.as_dict()}


def write_batch(lib, h, arrays):
    st = engine.WriteBatchStats()
    n_runs = lib.dbeel_gpu_reader_run_count(h)
    t0 = brw.now_ms()
    rc = lib.dbeel_gpu_reader_write_batch(h, n_runs, *arrays.args(), 0, None,
                                          None, None, ctypes.byref(st))
    t1 = brw.now_ms()
    brw.check(lib, rc)
    return {"total": t1 - t0, **st.as_dict()}


def flush(lib, h):
    t0 = brw.now_ms()
    rc = lib.dbeel_gpu_reader_memtable_flush(h, 0, None, None, None)
    t1 = brw.now_ms()
    brw.check(lib, rc)
    return {"total": t1 - t0}


def fetch_run(lib, h, pos):
    """Run bytes of the table at pos, through a single-run rewrite."""
    res = engine.CompactResult()
    p = (ctypes.c_uint32 * 1)(pos)
    brw.check(lib, lib.dbeel_gpu_reader_compact_begin(
        h, p, 1, 1, 0, ctypes.byref(res), None, None, None))
    lib.dbeel_gpu_reader_compact_abort(h)
    out = brw.result_bytes(res)
    lib.dbeel_gpu_result_free(ctypes.byref(res))
    return out


def sample(lib, device, prefill, batch, both, check_bytes=False):
    """One sample of every variant, each on a fresh reader: put (+ flush)
    into a memtable holding the prefill, and write_batch of the batch (of the
    concatenation for the flush comparison) on a reader that holds the
    prefill as a table."""
    out = {}
    h = brw.open_reader(lib, device)
    if prefill is not None:
        put(lib, h, prefill)  # not timed
    out["put"] = put(lib, h, batch)
    out["flush"] = flush(lib, h)
    mem_run = fetch_run(lib, h, 1) if check_bytes else None
    lib.dbeel_gpu_reader_close(h)

    h = brw.open_reader(lib, device)
    if prefill is not None:
        write_batch(lib, h, prefill)  # not timed
    out["write_batch"] = write_batch(lib, h, batch)
    lib.dbeel_gpu_reader_close(h)

    h = brw.open_reader(lib, device)
    out["write_batch_concat"] = write_batch(lib, h, both)
    if check_bytes:
        wb_run = fetch_run(lib, h, 1)
        assert np.array_equal(mem_run[0], wb_run[0]), "data differs"
        assert np.array_equal(mem_run[1], wb_run[1]), "index differs"
    lib.dbeel_gpu_reader_close(h)
    return out


def bench_put_flush(lib, device, reps, big):
    shapes = {}
    for shared in (False, True):
        fill = brw.make_batch(PREFILL, shared, seed=77 + int(shared))[0]
        for m in (0, PREFILL):
            prefill = fill if m else None
            for n in (8192, big):
                name = (f"m{m}_b{n}_"
                        f"{'shared' if shared else 'distinct'}_prefix")
                batch = make_arrivals(n, shared, n + m + int(shared), prefill)
                both = concat(prefill, batch) if m else batch
                sample(lib, device, prefill, batch, both, check_bytes=True)
                rows = [sample(lib, device, prefill, batch, both)
                        for _ in range(reps)]
                rec = {"memtable_entries_before": m, "writes": n,
                       "shared_prefix": shared, "key_bytes": brw.KLEN,
                       "value_bytes": brw.VLEN}
                for k in rows[0]:
                    rec[k] = {f: summarize([r[k][f] for r in rows])
                              for f in rows[0][k]
                              if f == "total" or f.endswith("_ms")}
                for f in ("batch_entries", "replaced", "entries",
                          "data_bytes"):
                    rec[f] = rows[0]["put"][f]
                rec["put_over_write_batch"] = (
                    rec["put"]["total"]["median"]
                    / rec["write_batch"]["total"]["median"])
                rec["flush_over_write_batch_concat"] = (
                    rec["flush"]["total"]["median"]
                    / rec["write_batch_concat"]["total"]["median"])
                print(f"{name}: put {rec['put']['total']['median']:.2f} ms "
                      f"(merge {rec['put']['merge_ms']['median']:.2f}) vs "
                      f"write_batch "
                      f"{rec['write_batch']['total']['median']:.2f} "
                      f"(x{rec['put_over_write_batch']:.2f}); flush "
                      f"{rec['flush']['total']['median']:.2f} vs concat "
                      f"{rec['write_batch_concat']['total']['median']:.2f}",
                      flush=True)
                shapes[name] = rec
    return shapes


def bind_get(lib):
    """The calls the get comparison needs, on any build of the library."""
    lib.dbeel_gpu_last_error.restype = ctypes.c_char_p
    lib.dbeel_gpu_reader_open.restype = ctypes.c_int
    lib.dbeel_gpu_reader_open.argtypes = [
        ctypes.POINTER(engine.RunView), ctypes.POINTER(engine.BloomView),
        ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.dbeel_gpu_reader_get.restype = ctypes.c_int
    lib.dbeel_gpu_reader_get.argtypes = [
        ctypes.c_void_p, bench_reader.U8P, bench_reader.U64P, ctypes.c_uint64,
        ctypes.POINTER(engine.GetResult), ctypes.POINTER(engine.GetStats)]
    lib.dbeel_gpu_get_result_free.restype = None
    lib.dbeel_gpu_get_result_free.argtypes = [
        ctypes.POINTER(engine.GetResult)]
    lib.dbeel_gpu_reader_close.restype = None
    lib.dbeel_gpu_reader_close.argtypes = [ctypes.c_void_p]
    return lib


class RawReader:
    def __init__(self, lib, views, n_runs, device):
        self._h = ctypes.c_void_p()
        rc = lib.dbeel_gpu_reader_open(views, None, n_runs, device,
                                       ctypes.byref(self._h))
        if rc != 0:
            raise engine.DbeelGpuError(rc,
                                       lib.dbeel_gpu_last_error().decode())


def bench_get(parent_path, device, scale, n_keys, reps):
    libs = {"parent": bind_get(ctypes.CDLL(os.path.abspath(parent_path))),
            "this": bind_get(engine._load_reader())}
    assert not hasattr(libs["parent"], "dbeel_gpu_reader_put"), \
        "--parent-lib already has the memtable"
    runs = bench_reader.make_config("cfg3", scale=scale)
    batch = bench_reader.Batch(bench_reader.make_queries(runs, n_keys, 32,
                                                         seed=0xBEAD))
    views, keepalive = engine._views(runs)
    readers = {k: RawReader(lib, views, len(runs), device)
               for k, lib in libs.items()}
    del keepalive
    hits = {}
    for k in libs:  # warm-up round, and the cross-check
        hits[k] = bench_reader.reader_get(libs[k], readers[k], batch)[2]
    assert np.array_equal(hits["parent"], hits["this"]), "hits differ"
    samples = {k: [] for k in libs}
    for _ in range(reps):
        for k in libs:  # interleaved
            samples[k].append(
                bench_reader.reader_get(libs[k], readers[k], batch)[1]
                ["search_ms"])
    for k in libs:
        libs[k].dbeel_gpu_reader_close(readers[k]._h)
    p, t = summarize(samples["parent"]), summarize(samples["this"])
    ok = p["min"] <= t["median"] <= p["max"]
    rec = {"workload": "cfg3", "scale": scale, "batch_keys": n_keys,
           "what": "search_ms (HIP events) with an empty memtable, parent "
                   "library and this build alternated in one process",
           "parent_samples": samples["parent"], "this_samples": samples["this"],
           "parent": p, "this": t,
           "this_median_inside_parent_min_max": ok}
    print(json.dumps({"parent": p, "this": t, "accepted": ok}), flush=True)
    return rec


def bench_get_nonempty(device, scale, n_keys, reps):
    """search_ms with 8,192 writes held in the memtable, against the same
    writes held as a 9th table (write_batch at the end): two readers of this
    build over cfg3, alternated."""
    lib = bind_get(engine._load_reader())
    runs = bench_reader.make_config("cfg3", scale=scale)
    batch = bench_reader.Batch(bench_reader.make_queries(runs, n_keys, 32,
                                                         seed=0xBEAD))
    writes = brw.make_batch(8192, False, seed=8192)[0]
    writes.keys[::2] = batch.blob.reshape(-1, 32)[:4096]  # half are queried
    views, keepalive = engine._views(runs)
    readers = {k: RawReader(lib, views, len(runs), device)
               for k in ("memtable", "ninth_table")}
    del keepalive
    put(lib, readers["memtable"]._h, writes)
    write_batch(lib, readers["ninth_table"]._h, writes)
    hits = {k: bench_reader.reader_get(lib, readers[k], batch)[2]
            for k in readers}  # warm-up round, and the cross-check
    assert np.array_equal(hits["memtable"], hits["ninth_table"]), "hits differ"
    samples = {k: [] for k in readers}
    for _ in range(reps):
        for k in readers:  # interleaved
            samples[k].append(
                bench_reader.reader_get(lib, readers[k], batch)[1]
                ["search_ms"])
    for k in readers:
        lib.dbeel_gpu_reader_close(readers[k]._h)
    rec = {"workload": "cfg3", "scale": scale, "batch_keys": n_keys,
           "what": "search_ms (HIP events), 8,192 writes held in the "
                   "memtable vs as a 9th unfiltered table",
           "memtable_hits": int((hits["memtable"]["run"] == len(runs)).sum())}
    for k in readers:
        rec[k] = summarize(samples[k])
        rec[k + "_samples"] = samples[k]
    print(json.dumps({k: rec[k] for k in readers}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="put,flush")
    ap.add_argument("--big", type=int, default=1 << 20,
                    help="writes in the large put shape")
    ap.add_argument("--parent-lib", help="the parent commit's library")
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run (get part)")
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--get-reps", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if parts & {"put", "flush"}:
        out["put_flush"] = {
            "what": "reader put / memtable_flush vs write_batch(pos = n_runs, "
                    "out = NULL), C ABI wall ms and HIP-event stage ms",
            "reps": args.reps,
            "shapes": bench_put_flush(engine._load_reader(), args.device,
                                      args.reps, args.big)}
    failed = False
    if "get" in parts:
        if not args.parent_lib:
            sys.exit("--parts get needs --parent-lib")
        out["get_empty_memtable"] = bench_get(
            args.parent_lib, args.device, args.scale, args.keys,
            args.get_reps)
        failed = not out["get_empty_memtable"][
            "this_median_inside_parent_min_max"]
    if "get_nonempty" in parts:
        out["get_nonempty_memtable"] = bench_get_nonempty(
            args.device, args.scale, args.keys, args.get_reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)
    if failed:
        sys.exit("search_ms median outside the parent's min-max")


if __name__ == "__main__":
    main()
