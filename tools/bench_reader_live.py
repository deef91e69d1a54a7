#!/usr/bin/env python3
"""Live-reader benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B keys,
1 KiB values), timed at the C ABI (wall clock around the calls, no Python
copies of the outputs).

State change measured: "the 8 resident runs are compacted into one, and the
reader serves the result".

  live      dbeel_gpu_reader_compact_begin + _commit on an open 8-run
            reader — with the output fetched to the host (what a caller
            writes to the .compact_* files), without, and without but
            building the filter;
  baseline  what the engine offered before the reader was live:
            dbeel_gpu_compact_timed from host bytes (upload, pipeline,
            fetch), then dbeel_gpu_reader_open over the resulting run
            (upload again).

Insert: dbeel_gpu_reader_insert_run of one more run into an open reader,
against the full dbeel_gpu_reader_open of all 8 runs a snapshot reader
needs for the same change.

Every repetition starts from a freshly opened reader, so the opens are the
"full reopen" samples. One warm-up round, then --reps rounds; median, min
and max are recorded. The paths are checked against each other: equal
output bytes, and equal answers to one get batch.

    python tools/bench_reader_live.py      # -> profiles/reader_live_cfg3.json

--fetch-into measures only the output fetch: compact_begin(out) against
compact_begin(out = NULL) + dbeel_gpu_reader_compact_fetch into pinned caller
buffers, same method:

    python tools/bench_reader_live.py --fetch-into
                                           # -> profiles/reader_fetch_into.json
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
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_live_cfg3.json")
FETCH_OUT = os.path.join(REPO, "profiles", "reader_fetch_into.json")
U8P = ctypes.POINTER(ctypes.c_uint8)


def now_ms():
    return time.perf_counter() * 1e3


def check(lib, rc):
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def open_reader(lib, views, n, device):
    h = ctypes.c_void_p()
    t0 = now_ms()
    check(lib, lib.dbeel_gpu_reader_open(views, None, n, device,
                                         ctypes.byref(h)))
    return h, now_ms() - t0


def result_arrays(res):
    """Views (no copy) of an engine-allocated result."""
    d = (np.ctypeslib.as_array(res.data, shape=(int(res.data_len),))
         if res.data_len else np.zeros(0, np.uint8))
    i = (np.ctypeslib.as_array(res.index, shape=(int(res.index_len),))
         if res.index_len else np.zeros(0, np.uint8))
    return d, i


def get_hits(rd_handle, keys):
    rd = engine.Reader._from_handle(rd_handle)
    try:
        hits, voff, values, _ = rd.get_raw(keys)
    finally:
        rd._h = None  # the caller owns the handle
    return hits, voff, values


def probe_keys(runs, n, seed=0xBEAD):
    rng = np.random.default_rng(seed)
    keys = []
    for _ in range(n // 2):
        d, i = runs[int(rng.integers(0, len(runs)))]
        offs = np.frombuffer(i, dtype="<u8").reshape(-1, 2)[:, 0]
        o = int(offs[int(rng.integers(0, len(offs)))])
        keys.append(d[o + 8 : o + 40].tobytes())
    keys += [bytes(rng.integers(0, 256, 32, dtype=np.uint8))
             for _ in range(n - n // 2)]
    return keys


def live_round(lib, views, n, device, fetch, bloom, positions, keys=None):
    """open (timed) -> begin + commit (timed) -> optional get -> close."""
    h, open_ms = open_reader(lib, views, n, device)
    res = engine.CompactResult()
    st = engine.ReaderCompactStats()
    out = {"open_ms": open_ms}
    try:
        t0 = now_ms()
        check(lib, lib.dbeel_gpu_reader_compact_begin(
            h, positions, n, 1, int(bloom),
            ctypes.byref(res) if fetch else None, None, None,
            ctypes.byref(st)))
        t1 = now_ms()
        check(lib, lib.dbeel_gpu_reader_compact_commit(h, 0))
        t2 = now_ms()
        out.update(begin_ms=t1 - t0, commit_ms=t2 - t1, total_ms=t2 - t0,
                   stats=st.as_dict())
        if keys is not None:
            out["answers"] = get_hits(h, keys)
            if fetch:
                d, i = result_arrays(res)
                out["bytes"] = (d.copy(), i.copy())
    finally:
        if fetch:
            lib.dbeel_gpu_result_free(ctypes.byref(res))
        lib.dbeel_gpu_reader_close(h)
    return out


def fetch_into_round(lib, views, n, device, positions, darr, iarr):
    """open -> begin(out = NULL) + compact_fetch into the caller's (pinned)
    arrays + commit, timed -> close."""
    h, open_ms = open_reader(lib, views, n, device)
    st = engine.ReaderCompactStats()
    dl, il = ctypes.c_uint64(), ctypes.c_uint64()
    ms = ctypes.c_double()
    try:
        t0 = now_ms()
        check(lib, lib.dbeel_gpu_reader_compact_begin(
            h, positions, n, 1, 0, None, None, None, ctypes.byref(st)))
        t1 = now_ms()
        check(lib, lib.dbeel_gpu_reader_compact_fetch(
            h, darr.ctypes.data_as(U8P), darr.size,
            iarr.ctypes.data_as(U8P), iarr.size, ctypes.byref(dl),
            ctypes.byref(il), ctypes.byref(ms)))
        t2 = now_ms()
        check(lib, lib.dbeel_gpu_reader_compact_commit(h, 0))
        t3 = now_ms()
    finally:
        lib.dbeel_gpu_reader_close(h)
    return {"open_ms": open_ms, "begin_ms": t1 - t0, "fetch_ms": t2 - t1,
            "commit_ms": t3 - t2, "total_ms": t3 - t0,
            "fetch_d2h_ms": ms.value, "stats": st.as_dict(),
            "lens": (int(dl.value), int(il.value))}


def bench_fetch_into(lib, runs, views, n, device, positions, warmup, reps,
                     out_path):
    """compact_begin(out) against compact_begin(out = NULL) + compact_fetch
    into pinned caller buffers, interleaved round by round, every round from
    a freshly opened reader."""
    # the output is no larger than the input
    darr = np.zeros(sum(d.nbytes for d, _ in runs), dtype=np.uint8)
    iarr = np.zeros(sum(i.nbytes for _, i in runs), dtype=np.uint8)
    engine.pin_host(darr)
    engine.pin_host(iarr)
    rows = {"begin_out": [], "begin_then_fetch_pinned": []}
    checks = {}
    try:
        for rnd in range(warmup + reps):
            first = rnd == 0
            a = live_round(lib, views, n, device, True, False, positions,
                           [b"k"] if first else None)
            b = fetch_into_round(lib, views, n, device, positions, darr, iarr)
            if first:
                dl, il = b["lens"]
                checks["bytes_identical"] = bool(
                    np.array_equal(a["bytes"][0], darr[:dl])
                    and np.array_equal(a["bytes"][1], iarr[:il]))
                print("checks:", json.dumps(checks), flush=True)
            if rnd < warmup:
                continue
            rows["begin_out"].append(a)
            rows["begin_then_fetch_pinned"].append(b)
            print(f"round {rnd - warmup + 1}/{reps}: begin(out) "
                  f"{a['total_ms']:.1f} ms, begin + fetch_into "
                  f"{b['total_ms']:.1f} ms", flush=True)
    finally:
        engine.unpin_host(darr)
        engine.unpin_host(iarr)
    fa, fb = rows["begin_out"], rows["begin_then_fetch_pinned"]
    res = {
        "workload": "cfg3", "n_runs": n,
        "output_bytes": sum(fb[-1]["lens"]),
        "timed_at": "C ABI calls, host wall clock; *d2h_ms are HIP events",
        "warmup_rounds": warmup, "reps": reps,
        "begin_out": {
            "begin_ms": summarize([r["begin_ms"] for r in fa]),
            "commit_ms": summarize([r["commit_ms"] for r in fa]),
            "total_ms": summarize([r["total_ms"] for r in fa]),
            "d2h_ms": summarize([r["stats"]["d2h_ms"] for r in fa]),
        },
        "begin_then_fetch_pinned": {
            "begin_ms": summarize([r["begin_ms"] for r in fb]),
            "fetch_ms": summarize([r["fetch_ms"] for r in fb]),
            "commit_ms": summarize([r["commit_ms"] for r in fb]),
            "total_ms": summarize([r["total_ms"] for r in fb]),
            "d2h_ms": summarize([r["fetch_d2h_ms"] for r in fb]),
        },
        "checks": checks,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    if not all(checks.values()):
        sys.exit("compact_fetch and compact_begin(out) disagree")


def baseline_round(lib, views, n, device, keys=None):
    """compact from host bytes -> open a reader over the output -> close."""
    res = engine.CompactResult()
    tim = engine.CompactTimings()
    out = {}
    t0 = now_ms()
    check(lib, lib.dbeel_gpu_compact_timed(views, n, 1, device,
                                           ctypes.byref(res),
                                           ctypes.byref(tim)))
    t1 = now_ms()
    try:
        one = (engine.RunView * 1)()
        one[0].data, one[0].data_len = res.data, res.data_len
        one[0].index, one[0].index_len = res.index, res.index_len
        h, open_ms = open_reader(lib, one, 1, device)
        t2 = now_ms()
        out.update(compact_ms=t1 - t0, open_ms=open_ms, total_ms=t2 - t0,
                   timings=tim.as_dict())
        try:
            if keys is not None:
                out["answers"] = get_hits(h, keys)
                d, i = result_arrays(res)
                out["bytes"] = (d.copy(), i.copy())
        finally:
            lib.dbeel_gpu_reader_close(h)
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    return out


def same_answers(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                and np.array_equal(a[2], b[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-keys", type=int, default=100_000)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--fetch-into", action="store_true",
                    help="only compact_begin(out) against begin(out = NULL) "
                         "+ compact_fetch into pinned buffers -> "
                         "profiles/reader_fetch_into.json")
    args = ap.parse_args()

    lib = engine._load_reader()
    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    keys = [] if args.fetch_into else probe_keys(runs, args.probe_keys)
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    n = len(runs)
    views, keepalive = engine._views(runs)
    positions = (ctypes.c_uint32 * n)(*range(n))
    input_bytes = sum(d.nbytes + i.nbytes for d, i in runs)

    if args.fetch_into:
        out = FETCH_OUT if args.out == DEFAULT_OUT else args.out
        bench_fetch_into(lib, runs, views, n, args.device, positions,
                         args.warmup, args.reps, out)
        del keepalive
        return

    # ---- compaction: live vs baseline, interleaved round by round ----
    variants = {"live_fetch": (True, False), "live_nofetch": (False, False),
                "live_nofetch_bloom": (False, True)}
    samples = {k: [] for k in list(variants) + ["baseline"]}
    reopen = []
    checks = {}
    for rnd in range(args.warmup + args.reps):
        first = rnd == 0
        kk = keys if first else None
        got = {"baseline": baseline_round(lib, views, n, args.device, kk)}
        for name, (fetch, bloom) in variants.items():
            got[name] = live_round(lib, views, n, args.device, fetch, bloom,
                                   positions, kk)
        if first:
            b = got["baseline"]
            checks["output_bytes_identical"] = bool(
                np.array_equal(b["bytes"][0], got["live_fetch"]["bytes"][0])
                and np.array_equal(b["bytes"][1],
                                   got["live_fetch"]["bytes"][1]))
            checks["answers_identical"] = all(
                same_answers(b["answers"], got[v]["answers"])
                for v in variants)
            print("checks:", json.dumps(checks), flush=True)
        if rnd < args.warmup:
            continue
        for name in samples:
            samples[name].append(got[name])
        reopen += [got[v]["open_ms"] for v in variants]
        print(f"round {rnd - args.warmup + 1}/{args.reps}: " + ", ".join(
            f"{k} {got[k]['total_ms']:.1f} ms" for k in samples), flush=True)

    def live_summary(rows):
        s = {k: summarize([r[k] for r in rows])
             for k in ("begin_ms", "commit_ms", "total_ms")}
        s["pipeline_kernel_ms"] = summarize(
            [r["stats"]["pipeline"]["kernel_ms"] for r in rows])
        for k in ("adopt_ms", "d2h_ms"):
            s[k] = summarize([r["stats"][k] for r in rows])
        s["d2h_bytes"] = rows[-1]["stats"]["d2h_bytes"]
        return s

    last = samples["live_fetch"][-1]["stats"]
    base_rows = samples["baseline"]
    res = {
        "workload": "cfg3", "scale": args.scale, "n_runs": n,
        "entries_in": last["entries_in"], "entries_out": last["entries_out"],
        "input_bytes": input_bytes,
        "output_bytes": last["data_bytes_out"] + 16 * last["entries_out"],
        "timed_at": "C ABI calls, host wall clock; stats fields are HIP "
                    "events",
        "warmup_rounds": args.warmup,
        "compaction": {
            "baseline_compact_then_open": {
                "compact_ms": summarize([r["compact_ms"] for r in base_rows]),
                "open_ms": summarize([r["open_ms"] for r in base_rows]),
                "total_ms": summarize([r["total_ms"] for r in base_rows]),
                "h2d_ms": summarize([r["timings"]["h2d_ms"]
                                     for r in base_rows]),
                "kernel_ms": summarize([r["timings"]["kernel_ms"]
                                        for r in base_rows]),
                "d2h_ms": summarize([r["timings"]["d2h_ms"]
                                     for r in base_rows]),
            },
            **{k: live_summary(samples[k]) for k in variants},
        },
        "checks": checks,
    }

    # ---- insert: one run into an open reader vs a full reopen ----
    h, _ = open_reader(lib, views, n - 1, args.device)
    ins = []
    try:
        for rnd in range(args.warmup + args.reps):
            t0 = now_ms()
            check(lib, lib.dbeel_gpu_reader_insert_run(
                h, lib.dbeel_gpu_reader_run_count(h),
                ctypes.byref(views[n - 1]), None))
            if rnd >= args.warmup:
                ins.append(now_ms() - t0)
    finally:
        lib.dbeel_gpu_reader_close(h)
    res["insert"] = {
        "run_bytes": int(runs[n - 1][0].nbytes + runs[n - 1][1].nbytes),
        "insert_run_ms": summarize(ins),
        "full_reopen_ms": summarize(reopen),
    }

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    del keepalive
    if not all(checks.values()):
        sys.exit("the live and the baseline path disagree")


if __name__ == "__main__":
    main()
