#!/usr/bin/env python3
"""Migration-scan benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B
keys, 1 KiB values): dbeel_gpu_scan against the paged scan over a resident
reader, timed at the C ABI (host wall clock around the calls).

Two scans a migration issues:

  hash_2_of_16   the whole key range, 2 of 16 equal murmur3 hash ranges
                 (one shard's share of a 16-shard ring moving out);
  key_1pct       a key range covering about 1% of the keys, no hash filter.

Each through

  baseline  dbeel_gpu_scan from host bytes: job create, upload of every
            run, flag of every entry, one engine-allocated result, teardown;
  paged     dbeel_gpu_reader_scan_begin / _next / _end on a reader that
            already holds the runs, into one pair of 64 MiB pinned buffers
            (pinned once, outside the timed region; the reader's open is
            not timed either — it is the state the read path keeps anyway).

The two are interleaved round by round: --warmup rounds, then --reps
rounds; median, min and max are recorded. The warm-up round checks that the
pages concatenated (offsets rebased) are the baseline's bytes. Per page the
HIP-event times of the last round are kept, and the candidates examined are
set against the total entry count.

    python tools/bench_reader_scan.py     # -> profiles/reader_scan_cfg3.json
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
from dbeel_amd.format import INDEX_DTYPE  # noqa: E402
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_scan_cfg3.json")
PAGE_BYTES = 64 << 20
PAGE_ENTRIES = 1 << 17  # 64 MiB of >= 512-B entries

SCANS = {
    # ranges 3 and 11 of 16 equal ones
    "hash_2_of_16": dict(hash_ranges=[(3 << 28, 4 << 28),
                                      (11 << 28, 12 << 28)]),
    # uniformly random keys: 2.56 / 256 of the first byte's span
    "key_1pct": dict(start_key=b"\x40", end_key=b"\x42\x8f"),
}


def now_ms():
    return time.perf_counter() * 1e3


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def baseline_scan(runs, device, kw, keep):
    """engine.scan without its Python copies: time the C call alone."""
    lib = engine.load()
    views, keepalive = engine._views(runs)
    U8P = ctypes.POINTER(ctypes.c_uint8)

    def kb(b):
        if b is None:
            return None, 0, None
        a = np.frombuffer(b or b"\0", dtype=np.uint8)
        return a.ctypes.data_as(U8P), len(b), a

    sp, sl, sa = kb(kw.get("start_key"))
    ep, el, ea = kb(kw.get("end_key"))
    ranges = kw.get("hash_ranges") or []
    rs = np.array([r[0] for r in ranges], dtype=np.uint32)
    re_ = np.array([r[1] for r in ranges], dtype=np.uint32)
    U32P = ctypes.POINTER(ctypes.c_uint32)
    res = engine.CompactResult()
    t0 = now_ms()
    rc = lib.dbeel_gpu_scan(
        views, len(runs), sp, sl, ep, el,
        rs.ctypes.data_as(U32P) if ranges else None,
        re_.ctypes.data_as(U32P) if ranges else None,
        len(ranges), device, ctypes.byref(res))
    ms = now_ms() - t0
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    out = {"ms": ms, "entries": int(res.entries_written),
           "data_bytes": int(res.data_len)}
    try:
        if keep:
            out["data"] = np.ctypeslib.as_array(
                res.data, shape=(int(res.data_len),)).copy()
            out["index"] = np.ctypeslib.as_array(
                res.index, shape=(int(res.index_len),)).copy()
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    del keepalive
    return out


def paged_scan(rd, kw, data, index, rid, compare=None):
    """begin -> next until done -> end, timed as a whole. compare = the
    baseline's (data, index) to check every page against."""
    pages = []
    entries = nbytes = cand = 0
    same = True
    t0 = now_ms()
    sc = rd.scan_open(**kw)
    try:
        while True:
            pg = sc.next(data, index, rid if kw.get("hash_ranges") else None)
            pages.append(pg)
            if compare is not None and pg["n_entries"]:
                n, ln = pg["n_entries"], pg["data_len"]
                same &= bool(np.array_equal(
                    data[:ln], compare[0][nbytes:nbytes + ln]))
                rec = index[:n * 16].view(INDEX_DTYPE).copy()
                rec["offset"] += np.uint64(nbytes)
                same &= bool(np.array_equal(
                    rec.view(np.uint8),
                    compare[1][entries * 16:(entries + n) * 16]))
            entries += pg["n_entries"]
            nbytes += pg["data_len"]
            cand += pg["candidates"]
            if pg["done"]:
                break
    finally:
        sc.close()
    ms = now_ms() - t0
    if compare is not None:
        same &= entries * 16 == len(compare[1]) and nbytes == len(compare[0])
    return {"ms": ms, "entries": entries, "data_bytes": nbytes,
            "candidates": cand, "pages": pages, "same": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()

    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    total_entries = sum(i.nbytes // 16 for _, i in runs)
    input_bytes = sum(d.nbytes + i.nbytes for d, i in runs)

    data = np.empty(PAGE_BYTES, dtype=np.uint8)
    index = np.empty(PAGE_ENTRIES * 16, dtype=np.uint8)
    rid = np.empty(PAGE_ENTRIES, dtype=np.uint32)
    bufs = (data, index, rid)
    for b in bufs:
        b[:] = 0  # touch the pages before locking them
        engine.pin_host(b)
    t0 = now_ms()
    rd = engine.Reader(runs, device=args.device)
    open_ms = now_ms() - t0
    samples = {k: {"baseline": [], "paged": []} for k in SCANS}
    checks = {}
    last = {}
    try:
        for rnd in range(args.warmup + args.reps):
            first = rnd == 0
            for name, kw in SCANS.items():
                b = baseline_scan(runs, args.device, kw, keep=first)
                p = paged_scan(rd, kw, data, index, rid,
                               (b["data"], b["index"]) if first else None)
                if first:
                    checks[name + "_bytes_identical"] = p["same"]
                    print("check", name, p["same"], flush=True)
                if (p["entries"], p["data_bytes"]) != (b["entries"],
                                                       b["data_bytes"]):
                    sys.exit(f"{name}: paged {p['entries']} entries / "
                             f"{p['data_bytes']} B, baseline {b['entries']} "
                             f"/ {b['data_bytes']} B")
                if rnd < args.warmup:
                    continue
                samples[name]["baseline"].append(b["ms"])
                samples[name]["paged"].append(p["ms"])
                last[name] = p
                print(f"round {rnd - args.warmup + 1}/{args.reps} {name}: "
                      f"baseline {b['ms']:.1f} ms, paged {p['ms']:.1f} ms "
                      f"({len(p['pages'])} pages)", flush=True)
    finally:
        rd.close()
        for b in bufs:
            engine.unpin_host(b)

    res = {
        "workload": "cfg3", "scale": args.scale, "n_runs": len(runs),
        "total_entries": total_entries, "input_bytes": input_bytes,
        "page_bytes": PAGE_BYTES, "page_entries": PAGE_ENTRIES,
        "max_candidates": "default (2^20)",
        "timed_at": "C ABI calls, host wall clock; per-page fields are HIP "
                    "events on the reader's stream",
        "not_timed": "reader open (below, once) and pinning of the page "
                     "buffers",
        "reader_open_ms": open_ms,
        "warmup_rounds": args.warmup,
        "scans": {},
        "checks": checks,
    }
    for name, p in last.items():
        pages = p["pages"]
        res["scans"][name] = {
            "filter": {k: (v.hex() if isinstance(v, bytes) else v)
                       for k, v in SCANS[name].items()},
            "entries_out": p["entries"], "data_bytes_out": p["data_bytes"],
            "candidates": p["candidates"],
            "candidates_over_total_entries": p["candidates"] / total_entries,
            "baseline_dbeel_gpu_scan_ms": summarize(samples[name]["baseline"]),
            "paged_reader_scan_ms": summarize(samples[name]["paged"]),
            "n_pages": len(pages),
            "per_page_last_round": [
                {k: pg[k] for k in ("candidates", "n_entries", "data_len",
                                    "flag_ms", "emit_ms", "copy_ms",
                                    "d2h_ms")} for pg in pages],
            "per_page_median_ms": {
                k: statistics.median(pg[k] for pg in pages)
                for k in ("flag_ms", "emit_ms", "copy_ms", "d2h_ms")},
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    if not all(checks.values()):
        sys.exit("the paged scan and dbeel_gpu_scan disagree")


if __name__ == "__main__":
    main()
