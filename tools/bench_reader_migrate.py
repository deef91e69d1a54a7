#!/usr/bin/env python3
"""Migration benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B keys,
1 KiB values): 2 of 16 equal murmur3 hash ranges of a resident reader moved
into the memtable of a second reader on the same device, 64 MiB pages, timed
at the C ABI (host wall clock around the whole loop).

Three routes:

  a_decode_put   scan_next into pinned buffers, the page decoded on the host
                 into put's five arrays, dbeel_gpu_reader_put. The decode is
                 numpy (vectorised gathers over the index records), not an
                 engine path: it stands for what any receiver had to do
                 before put_entries existed, and is labelled as such.
  b_put_entries  scan_next into pinned buffers, dbeel_gpu_reader_put_entries
                 of the page as it lies there.
  c_scan_apply   dbeel_gpu_reader_scan_apply: the page never leaves HBM.

plus c with the DELETE action over the same ranges. The routes are
interleaved round by round: --warmup rounds, then --reps rounds; median, min
and max are recorded. Every round starts from a cleared destination
memtable; the first round checks that the three routes leave the same
memtable bytes. Per page the stats of the last round are kept.

--parts put_ab --parent-lib PARENT.so is the one pass/fail timing: put must
not have become slower by sharing its merge with put_entries. The parent
commit's library (built from a git worktree into a separate .so) and this
build are alternated in one process on tools/bench_reader_memtable.py's put
rows (8,192 and 2^20 writes, distinct and shared prefixes, into 0 and 2^20
entries), each sample on a fresh reader; accepted when this build's median
lies inside the parent's own min-max for every row. Both sample sets are
written out.

    python tools/bench_reader_migrate.py   # -> profiles/reader_migrate.json
    python tools/bench_reader_migrate.py --parts put_ab --parent-lib PARENT.so
        # parts merge into the file
"""
import argparse
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
from dbeel_amd.format import INDEX_DTYPE, Entry, build_run  # noqa: E402
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_migrate.json")
PAGE_BYTES = 64 << 20
PAGE_ENTRIES = 1 << 17  # 64 MiB of >= 512-B entries
RANGES = [(3 << 28, 4 << 28), (11 << 28, 12 << 28)]  # 3 and 11 of 16
DELETE_TS = 1_700_000_000_000_000_000


def now_ms():
    return time.perf_counter() * 1e3


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def _gather(data, starts, lens):
    """The bytes data[starts[i] : starts[i] + lens[i]] concatenated, and
    their offsets (n + 1)."""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    if not total:
        return np.zeros(1, dtype=np.uint8), off
    idx = (np.repeat(starts.astype(np.int64) - off[:-1].astype(np.int64),
                     lens.astype(np.int64))
           + np.arange(total, dtype=np.int64))
    return data[idx], off


def decode_arrays(data, index):
    """A page -> put's five arrays, in numpy."""
    rec = index.view(INDEX_DTYPE)
    off = rec["offset"].astype(np.uint64)
    klen = rec["key_size"].astype(np.uint64) - 8
    vlen = rec["full_size"].astype(np.uint64) - 32 - klen
    keys, koff = _gather(data, off + 8, klen)
    vals, voff = _gather(data, off + 16 + klen, vlen)
    ts, _ = _gather(data, off + 16 + klen + vlen,
                    np.full(len(rec), 16, dtype=np.uint64))
    return keys, koff, vals, voff, ts


def route_a(src, dst, bufs):
    data, index, rid = bufs
    lib = dst._lib
    U8P, U64P = engine._U8P, engine._U64P
    pages = []
    decode_ms = 0.0
    t0 = now_ms()
    sc = src.snapshot_open(hash_ranges=RANGES)
    try:
        while True:
            pg = sc.next(data, index, rid)
            n = pg["n_entries"]
            if n:
                t1 = now_ms()
                k, ko, v, vo, ts = decode_arrays(data[:pg["data_len"]],
                                                 index[:n * 16])
                decode_ms += now_ms() - t1
                st = engine.MemtablePutStats()
                rc = lib.dbeel_gpu_reader_put(
                    dst._h, n, k.ctypes.data_as(U8P), ko.ctypes.data_as(U64P),
                    v.ctypes.data_as(U8P), vo.ctypes.data_as(U64P),
                    ts.ctypes.data_as(U8P), ctypes.byref(st))
                dst._check(rc)
                pages.append(dict(pg, **st.as_dict()))
            if pg["done"]:
                break
    finally:
        sc.close()
    return {"ms": now_ms() - t0, "host_decode_ms": decode_ms, "pages": pages}


def route_b(src, dst, bufs):
    data, index, rid = bufs
    pages = []
    t0 = now_ms()
    sc = src.snapshot_open(hash_ranges=RANGES)
    try:
        while True:
            pg = sc.next(data, index, rid)
            n = pg["n_entries"]
            if n:
                st = dst.put_entries(data[:pg["data_len"]], index[:n * 16])
                pages.append(dict(pg, **st))
            if pg["done"]:
                break
    finally:
        sc.close()
    return {"ms": now_ms() - t0, "pages": pages}


def route_c(src, dst, kind):
    pages = []
    acts = [(kind, dst)] * len(RANGES)
    t0 = now_ms()
    sc = src.snapshot_open(hash_ranges=RANGES)
    try:
        while True:
            pg, st = sc.apply(acts, PAGE_BYTES, PAGE_ENTRIES,
                              delete_ts=DELETE_TS if kind == "delete"
                              else None)
            pages.append(dict(pg, **st))
            if pg["done"]:
                break
    finally:
        sc.close()
    return {"ms": now_ms() - t0, "pages": pages}


def bind_put(lib):
    """The calls the put comparison needs, on any build of the library."""
    lib.dbeel_gpu_last_error.restype = ctypes.c_char_p
    lib.dbeel_gpu_reader_open.restype = ctypes.c_int
    lib.dbeel_gpu_reader_open.argtypes = [
        ctypes.POINTER(engine.RunView), ctypes.POINTER(engine.BloomView),
        ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.dbeel_gpu_reader_put.restype = ctypes.c_int
    lib.dbeel_gpu_reader_put.argtypes = (
        [ctypes.c_void_p] + engine._BATCH_ARGTYPES
        + [ctypes.POINTER(engine.MemtablePutStats)])
    lib.dbeel_gpu_reader_close.restype = None
    lib.dbeel_gpu_reader_close.argtypes = [ctypes.c_void_p]
    return lib


def put_ab(parent_path, device, reps, big):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench_reader_memtable as brm
    import bench_reader_write as brw

    libs = {"parent": bind_put(ctypes.CDLL(os.path.abspath(parent_path))),
            "this": bind_put(engine._load_reader())}
    assert not hasattr(libs["parent"], "dbeel_gpu_reader_put_entries"), \
        "--parent-lib already has put_entries"

    def one(lib, prefill, batch):
        h = brw.open_reader(lib, device)
        if prefill is not None:
            brm.put(lib, h, prefill)  # not timed
        r = brm.put(lib, h, batch)
        lib.dbeel_gpu_reader_close(h)
        return r

    rows = {}
    ok = True
    for shared in (False, True):
        fill = brw.make_batch(brm.PREFILL, shared, seed=77 + int(shared))[0]
        for m in (0, brm.PREFILL):
            prefill = fill if m else None
            for n in (8192, big):
                name = (f"m{m}_b{n}_"
                        f"{'shared' if shared else 'distinct'}_prefix")
                batch = brm.make_arrivals(n, shared, n + m + int(shared),
                                          prefill)
                stats = {k: one(lib, prefill, batch)
                         for k, lib in libs.items()}  # warm-up round
                for f in ("batch_entries", "replaced", "entries",
                          "data_bytes"):
                    assert stats["parent"][f] == stats["this"][f], f
                samples = {k: [] for k in libs}
                for _ in range(reps):
                    for k, lib in libs.items():  # interleaved
                        samples[k].append(one(lib, prefill, batch)["total"])
                ps, ts = summarize(samples["parent"]), summarize(samples["this"])
                inside = ps["min"] <= ts["median"] <= ps["max"]
                ok &= inside
                rows[name] = {"parent_samples": samples["parent"],
                              "this_samples": samples["this"],
                              "parent": ps, "this": ts,
                              "this_median_inside_parent_min_max": inside}
                print(f"{name}: parent {ps['median']:.3f} "
                      f"({ps['min']:.3f}-{ps['max']:.3f}) this "
                      f"{ts['median']:.3f} ({ts['min']:.3f}-{ts['max']:.3f}) "
                      f"inside={inside}", flush=True)
    return {"what": "dbeel_gpu_reader_put wall ms at the C ABI, the parent "
                    "commit's library and this build alternated in one "
                    "process, a fresh reader per sample",
            "reps": reps, "rows": rows, "accepted": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="migrate")
    ap.add_argument("--parent-lib", help="the parent commit's library")
    ap.add_argument("--big", type=int, default=1 << 20,
                    help="writes in the large put shape")
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    if "put_ab" in parts:
        if not args.parent_lib:
            sys.exit("--parts put_ab needs --parent-lib")
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        out["put_parent_vs_this"] = put_ab(args.parent_lib, args.device,
                                           args.reps, args.big)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
        if not out["put_parent_vs_this"]["accepted"]:
            sys.exit("a put median lies outside the parent's min-max")
    if "migrate" not in parts:
        return

    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    total_entries = sum(i.nbytes // 16 for _, i in runs)

    data = np.empty(PAGE_BYTES, dtype=np.uint8)
    index = np.empty(PAGE_ENTRIES * 16, dtype=np.uint8)
    rid = np.empty(PAGE_ENTRIES, dtype=np.uint32)
    bufs = (data, index, rid)
    for b in bufs:
        b[:] = 0  # touch the pages before locking them
        engine.pin_host(b)
    src = engine.Reader(runs, device=args.device)
    # the destination: a reader whose only table is one unrelated entry,
    # its memtable empty at the start of every route
    dst = engine.Reader([build_run([Entry(b"\xff" * 40, b"x", 0)])],
                        device=args.device)
    names = ("a_decode_put", "b_put_entries", "c_scan_apply",
             "c_scan_apply_delete")
    samples = {k: [] for k in names}
    decode = []
    last = {}
    checks = {}
    try:
        for rnd in range(args.warmup + args.reps):
            got = {}
            for name in names:
                dst.memtable_clear()
                if name == "a_decode_put":
                    r = route_a(src, dst, bufs)
                elif name == "b_put_entries":
                    r = route_b(src, dst, bufs)
                else:
                    r = route_c(src, dst, "delete" if name.endswith("delete")
                                else "put")
                r["memtable"] = dst.memtable_info
                if rnd == 0:
                    got[name] = dst.memtable_fetch()
                if rnd >= args.warmup:
                    samples[name].append(r["ms"])
                    if "host_decode_ms" in r:
                        decode.append(r["host_decode_ms"])
                    last[name] = r
                print(f"round {rnd} {name}: {r['ms']:.1f} ms, "
                      f"{len(r['pages'])} pages, memtable "
                      f"{r['memtable']['entries']} entries", flush=True)
            if rnd == 0:
                checks["a_b_c_memtable_bytes_identical"] = (
                    got["a_decode_put"] == got["b_put_entries"]
                    == got["c_scan_apply"])
                print("check", checks, flush=True)
    finally:
        dst.close()
        src.close()
        for b in bufs:
            engine.unpin_host(b)

    keys = ("n_entries", "data_len", "flag_ms", "emit_ms", "copy_ms",
            "d2h_ms", "h2d_ms", "order_ms", "merge_ms", "apply_ms",
            "put_entries", "delete_entries")
    res = {
        "workload": "cfg3", "scale": args.scale, "n_runs": len(runs),
        "total_entries": total_entries, "hash_ranges": RANGES,
        "page_bytes": PAGE_BYTES, "page_entries": PAGE_ENTRIES,
        "timed_at": "C ABI calls from Python, host wall clock around the "
                    "whole scan loop; per-page fields are HIP events "
                    "(apply_ms: host wall inside scan_apply)",
        "route_a_decode": "numpy gathers on the host, not an engine path",
        "not_timed": "reader opens, pinning, memtable_clear between routes",
        "warmup_rounds": args.warmup,
        "routes": {},
        "host_decode_ms_in_a": summarize(decode) if decode else None,
        "checks": checks,
    }
    for name, r in last.items():
        res["routes"][name] = {
            "wall_ms": summarize(samples[name]),
            "samples_ms": samples[name],
            "n_pages": len(r["pages"]),
            "memtable_after": r["memtable"],
            "per_page_last_round": [
                {k: pg[k] for k in keys if k in pg} for pg in r["pages"]],
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if "put_parent_vs_this" in old:
        res["put_parent_vs_this"] = old["put_parent_vs_this"]
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items()
                      if k not in ("routes", "put_parent_vs_this")}))
    for name in res["routes"]:
        print(name, res["routes"][name]["wall_ms"])
    if not all(checks.values()):
        sys.exit("the routes leave different memtables")


if __name__ == "__main__":
    main()
