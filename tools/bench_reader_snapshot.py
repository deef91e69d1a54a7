#!/usr/bin/env python3
"""Snapshot-scan benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B keys,
1 KiB values, 50% overlap), timed at the C ABI (host wall clock around the
calls; per-page fields are HIP events on the reader's stream). Modelled on
tools/bench_reader_scan.py; the filters are its two.

  parity      flags=0 snapshot pages against the old scan's pages, interleaved
              round by round, 64 MiB pinned page buffers. With --parent-lib
              the old scan runs in THAT library (a build of the parent commit,
              loaded next to this one, its own reader over the same runs);
              without it, in this library's dbeel_gpu_reader_scan_begin. The
              launched kernels are the same, so the snapshot's median must lie
              inside the old scan's own min-max band.
  newest      NEWEST_ONLY against the plain snapshot scan of the same filter
              (full scan and 2-of-16 hash ranges): entries and bytes emitted,
              total and summed flag_ms, both shadow-pass variants
              (DBEEL_SCAN_SHADOW=narrow|full), interleaved, with pinned and
              with pageable page buffers, all at --newest-max-candidates
              (default 2^17 = the page's entry capacity). The expected
              emitted share comes from a host count over a scaled-down cfg3
              generator run.
  begin       begin+end with DBEEL_SCAN_MEMTABLE at memtables of 2^10 and 2^20
              entries: begin copies nothing, so the two must not scale.
  disturbed   a ~64-page scan with a put + memtable_flush between pages (the
              flushed tables are compacted into one whenever 32 have piled
              up), against the same scan undisturbed; the scan's own time is
              the sum of its next() calls.

    python tools/bench_reader_snapshot.py   # -> profiles/reader_snapshot.json
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
from dbeel_amd.format import parse_run  # noqa: E402
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_snapshot.json")
PAGE_BYTES = 64 << 20
PAGE_ENTRIES = 1 << 17  # 64 MiB of >= 512-B entries

HASH_2_OF_16 = dict(hash_ranges=[(3 << 28, 4 << 28), (11 << 28, 12 << 28)])
KEY_1PCT = dict(start_key=b"\x40", end_key=b"\x42\x8f")


def now_ms():
    return time.perf_counter() * 1e3


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def drive(sc, data, index, rid, between=None):
    """next until done; -> totals, the sum of the next() calls' wall time and
    the per-page HIP-event sums. between(page_no) is not timed."""
    out = dict(entries=0, data_bytes=0, candidates=0, pages=0, next_ms=0.0,
               flag_ms=0.0, emit_ms=0.0, copy_ms=0.0, d2h_ms=0.0)
    while True:
        t0 = now_ms()
        pg = sc.next(data, index, rid)
        out["next_ms"] += now_ms() - t0
        out["pages"] += 1
        out["entries"] += pg["n_entries"]
        out["data_bytes"] += pg["data_len"]
        out["candidates"] += pg["candidates"]
        for k in ("flag_ms", "emit_ms", "copy_ms", "d2h_ms"):
            out[k] += pg[k]
        if pg["done"]:
            return out
        if between is not None:
            between(out["pages"])


def timed_scan(opener, kw, bufs, between=None):
    """begin -> pages -> end as a whole."""
    data, index, rid = bufs
    t0 = now_ms()
    sc = opener()
    try:
        out = drive(sc, data, index, rid if kw.get("hash_ranges") else None,
                    between)
        out["shadowed"] = sc.info()["shadowed"]
    finally:
        sc.close()
    out["ms"] = now_ms() - t0
    return out


def load_parent(path, runs, device):
    """A second library (the parent commit's build) with its own reader over
    the same runs. It gets the prototypes of the calls the old scan uses."""
    lib = engine._load_reader()
    par = ctypes.CDLL(os.path.abspath(path))
    for name in ("dbeel_gpu_reader_open", "dbeel_gpu_reader_close",
                 "dbeel_gpu_reader_scan_begin", "dbeel_gpu_reader_scan_next",
                 "dbeel_gpu_reader_scan_end", "dbeel_gpu_last_error",
                 "dbeel_gpu_reader_run_count", "dbeel_gpu_reader_table_bytes"):
        getattr(par, name).argtypes = getattr(lib, name).argtypes
        getattr(par, name).restype = getattr(lib, name).restype
    views, keepalive = engine._views(runs)
    h = ctypes.c_void_p()
    rc = par.dbeel_gpu_reader_open(views, None, len(runs), device,
                                   ctypes.byref(h))
    del keepalive
    if rc:
        sys.exit("parent library: reader_open failed: "
                 + par.dbeel_gpu_last_error().decode())
    rd = engine.Reader.__new__(engine.Reader)
    rd._lib, rd._h, rd._scans = par, h, []
    return rd


def bench_parity(rd, old_rd, bufs, warmup, reps):
    res = {}
    for name, kw in (("hash_2_of_16", HASH_2_OF_16), ("key_1pct", KEY_1PCT)):
        old, snap = [], []
        for rnd in range(warmup + reps):
            o = timed_scan(lambda: old_rd.scan_open(**kw), kw, bufs) \
                if old_rd._lib is rd._lib else timed_old(old_rd, kw, bufs)
            s = timed_scan(lambda: rd.snapshot_open(**kw), kw, bufs)
            if (o["entries"], o["data_bytes"]) != (s["entries"],
                                                   s["data_bytes"]):
                sys.exit(f"parity {name}: old {o['entries']} entries, "
                         f"snapshot {s['entries']}")
            if rnd >= warmup:
                old.append(o["ms"])
                snap.append(s["ms"])
                print(f"parity {name} round {rnd - warmup + 1}/{reps}: old "
                      f"{o['ms']:.2f} ms, snapshot {s['ms']:.2f} ms",
                      flush=True)
        so, ss = summarize(old), summarize(snap)
        res[name] = {
            "entries_out": s["entries"], "data_bytes_out": s["data_bytes"],
            "pages": s["pages"], "old_scan_ms": so,
            "snapshot_flags0_ms": ss,
            "snapshot_median_inside_old_band":
                so["min"] <= ss["median"] <= so["max"],
        }
    return res


def timed_old(old_rd, kw, bufs):
    """The old scan in the parent library: its scans have no info()."""
    data, index, rid = bufs
    t0 = now_ms()
    sc = old_rd.scan_open(**kw)
    try:
        out = drive(sc, data, index, rid if kw.get("hash_ranges") else None)
    finally:
        sc.close()
    out["ms"] = now_ms() - t0
    return out


def expected_share(scale, kw):
    """Emitted / examined entries under NEWEST_ONLY on a scaled-down cfg3
    generator run, counted on the host (tables only)."""
    runs = make_config("cfg3", scale=scale)
    parsed = [parse_run(bytes(d), bytes(i)) for d, i in runs]
    later = set()
    kept = total = 0
    for entries in reversed(parsed):
        for e in entries:
            total += 1
            kept += e.key not in later
        later |= {e.key for e in entries}
    return {"scale": scale, "entries": total, "emitted": kept,
            "emitted_share": kept / total}


def bench_newest(rd, pinned_bufs, warmup, reps, mc):
    pageable = tuple(np.empty_like(b) for b in pinned_bufs)
    for b in pageable:
        b[:] = 0
    res = {}
    for name, kw in (("full", {}), ("hash_2_of_16", HASH_2_OF_16)):
        entry = {}
        for bname, bufs in (("pinned", pinned_bufs), ("pageable", pageable)):
            samples = {"plain": [], "narrow": [], "full": []}
            last = {}
            for rnd in range(warmup + reps):
                for variant in ("plain", "narrow", "full"):
                    if variant != "plain":
                        os.environ["DBEEL_SCAN_SHADOW"] = variant
                    r = timed_scan(
                        lambda: rd.snapshot_open(
                            max_candidates=mc,
                            newest_only=variant != "plain", **kw), kw, bufs)
                    if rnd >= warmup:
                        samples[variant].append(r)
                    last[variant] = r
                print(f"newest {name} {bname} round {rnd + 1}: " + ", ".join(
                    f"{v} {last[v]['ms']:.1f} ms (flag {last[v]['flag_ms']:.2f})"
                    for v in last), flush=True)
            if (last["narrow"]["entries"], last["narrow"]["data_bytes"]) != (
                    last["full"]["entries"], last["full"]["data_bytes"]):
                sys.exit("the two shadow-pass variants disagree")
            entry[bname] = {
                v: {"total_ms": summarize([r["ms"] for r in samples[v]]),
                    "flag_ms_sum": summarize([r["flag_ms"]
                                              for r in samples[v]]),
                    "d2h_ms_sum": summarize([r["d2h_ms"]
                                             for r in samples[v]]),
                    "entries_out": last[v]["entries"],
                    "data_bytes_out": last[v]["data_bytes"],
                    "candidates": last[v]["candidates"],
                    "shadowed": last[v]["shadowed"],
                    "pages": last[v]["pages"]} for v in samples}
            p, n = entry[bname]["plain"], entry[bname]["narrow"]
            entry[bname]["emitted_bytes_share"] = (n["data_bytes_out"]
                                                   / p["data_bytes_out"])
            entry[bname]["emitted_entries_share"] = (n["entries_out"]
                                                     / p["entries_out"])
            if not n["data_bytes_out"] < p["data_bytes_out"]:
                sys.exit("NEWEST_ONLY did not lower the emitted bytes")
        res[name] = entry
    os.environ.pop("DBEEL_SCAN_SHADOW", None)
    return res


def rand_writes(rng, n, klen=32, vlen=64):
    keys = rng.integers(0, 256, (n, klen), dtype=np.uint8)
    vals = rng.integers(0, 256, (n, vlen), dtype=np.uint8)
    return [(keys[j].tobytes(), vals[j].tobytes(), j) for j in range(n)]


def bench_begin(runs, device, reps):
    res = {}
    rng = np.random.default_rng(1)
    for log2 in (10, 20):
        with engine.Reader(runs[:1], device=device) as rd:
            rd.put(rand_writes(rng, 1 << log2))
            entries = rd.memtable_info["entries"]
            ms = []
            for _ in range(reps + 2):
                t0 = now_ms()
                sc = rd.snapshot_open(memtable=True, **KEY_1PCT)
                t1 = now_ms()
                sc.close()
                ms.append(t1 - t0)
            res[f"memtable_2^{log2}"] = {"memtable_entries": entries,
                                         "begin_ms": summarize(ms[2:])}
    return res


def bench_disturbed(rd, bufs, reps):
    """hash_2_of_16 in 16 MiB pages (~62 pages)."""
    kw = HASH_2_OF_16
    data, index, rid = bufs
    small = (data[:16 << 20], index, rid)
    rng = np.random.default_rng(2)
    base_tables = rd.n_runs
    edits = {"ms": 0.0, "n": 0}

    def between(page_no):
        t0 = now_ms()
        rd.put(rand_writes(rng, 256))
        rd.memtable_flush(fetch=False)
        if rd.n_runs >= base_tables + 32:
            rd.compact(list(range(base_tables, rd.n_runs)), base_tables,
                       keep_tombstones=True, fetch=False)
        edits["ms"] += now_ms() - t0
        edits["n"] += 1

    calm, rough = [], []
    for rnd in range(reps + 1):
        c = timed_scan(lambda: rd.snapshot_open(**kw), kw, small)
        r = timed_scan(lambda: rd.snapshot_open(**kw), kw, small, between)
        if rnd:
            calm.append(c["next_ms"])
            rough.append(r["next_ms"])
        print(f"disturbed round {rnd}: calm {c['next_ms']:.1f} ms, with "
              f"edits {r['next_ms']:.1f} ms ({r['pages']} pages, "
              f"{rd.n_runs} tables, held {rd.held_bytes} B)", flush=True)
    return {"pages": r["pages"], "edits_per_scan": edits["n"] // (reps + 1),
            "edit_ms_mean": edits["ms"] / max(1, edits["n"]),
            "undisturbed_next_ms_sum": summarize(calm),
            "disturbed_next_ms_sum": summarize(rough),
            "tables_at_end": rd.n_runs, "held_bytes_at_end": rd.held_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None,
                    help="libdbeel_gpu.so built from the parent commit")
    ap.add_argument("--model-scale", type=float, default=0.002)
    ap.add_argument("--newest-max-candidates", type=int, default=1 << 17,
                    help="window of the NEWEST_ONLY comparison (all three "
                         "variants): the shadow pass examines the whole "
                         "window, a page consumes what its buffers hold")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()

    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    bufs = (np.empty(PAGE_BYTES, dtype=np.uint8),
            np.empty(PAGE_ENTRIES * 16, dtype=np.uint8),
            np.empty(PAGE_ENTRIES, dtype=np.uint32))
    for b in bufs:
        b[:] = 0  # touch the pages before locking them
        engine.pin_host(b)
    rd = engine.Reader(runs, device=args.device)
    old_rd = (load_parent(args.parent_lib, runs, args.device)
              if args.parent_lib else rd)
    res = {
        "workload": "cfg3", "scale": args.scale, "n_runs": len(runs),
        "total_entries": sum(i.nbytes // 16 for _, i in runs),
        "input_bytes": sum(d.nbytes + i.nbytes for d, i in runs),
        "page_bytes": PAGE_BYTES, "page_entries": PAGE_ENTRIES,
        "max_candidates": "default (2^20)",
        "timed_at": "C ABI calls, host wall clock; flag/d2h sums are HIP "
                    "events on the reader's stream; flag_ms includes the "
                    "shadow pass",
        "old_scan_library": ("parent commit's build, loaded next to this one"
                             if args.parent_lib else
                             "this build's dbeel_gpu_reader_scan_begin"),
        "warmup_rounds": args.warmup, "reps": args.reps,
    }
    try:
        res["parity_flags0"] = bench_parity(rd, old_rd, bufs, args.warmup,
                                            args.reps)
        if old_rd is not rd:
            old_rd._lib.dbeel_gpu_reader_close(old_rd._h)
            old_rd._h = None
        res["newest_only"] = bench_newest(rd, bufs, args.warmup,
                                          max(3, args.reps // 2 + 1),
                                          args.newest_max_candidates)
        res["newest_only"]["max_candidates"] = args.newest_max_candidates
        res["newest_only"]["model_expected"] = expected_share(
            args.model_scale, {})
        res["begin_with_memtable"] = bench_begin(runs, args.device, args.reps)
        res["disturbed_scan"] = bench_disturbed(rd, bufs, 3)
    finally:
        rd.close()
        for b in bufs:
            engine.unpin_host(b)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    if not all(v["snapshot_median_inside_old_band"]
               for v in res["parity_flags0"].values()):
        sys.exit("flags=0 snapshot median outside the old scan's band")


if __name__ == "__main__":
    main()
