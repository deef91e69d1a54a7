#!/usr/bin/env python3
"""Host runs in, host bytes out, at the cfg3 workload (8 runs x ~1 GiB, 32-B
keys, 1 KiB values), timed at the C ABI (wall clock around each call, no
Python copies of the outputs).

Routes, interleaved round by round:

  compact           dbeel_gpu_compact_timed — the baseline: output fetched
                    into a fresh engine-allocated pageable buffer;
  into_pageable_1   dbeel_gpu_compact_into, 1 slice, into a pageable caller
                    buffer touched once beforehand;
  into_pinned_1     the same into buffers registered with dbeel_gpu_pin_host;
  into_pinned_S     pinned, S = 2, 4, 8, 16 pipelined slices.

Per route: wall_ms, the summed h2d / kernel / d2h stage times (HIP events)
and, for compact_into, overlap_ms. dbeel_gpu_compact_timed does not time its
fetch: its d2h_ms column is wall - h2d - kernel, the fetch together with the
host allocation it goes into. One warm-up round, which also checks that every
route returns the same bytes, then --reps rounds; median (min-max).

    python tools/bench_compact_stream.py   # -> profiles/compact_stream_cfg3.json
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

DEFAULT_OUT = os.path.join(REPO, "profiles", "compact_stream_cfg3.json")
SLICE_COUNTS = (2, 4, 8, 16)


def now_ms():
    return time.perf_counter() * 1e3


def check(lib, rc):
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


def baseline_round(lib, views, n, device, keep_bytes):
    res = engine.CompactResult()
    tim = engine.CompactTimings()
    t0 = now_ms()
    check(lib, lib.dbeel_gpu_compact_timed(views, n, 0, device,
                                           ctypes.byref(res),
                                           ctypes.byref(tim)))
    wall = now_ms() - t0
    out = {"wall_ms": wall, "h2d_ms": tim.h2d_ms, "kernel_ms": tim.kernel_ms,
           "d2h_ms": wall - tim.h2d_ms - tim.kernel_ms, "overlap_ms": 0.0,
           "slices": 1}
    try:
        if keep_bytes:
            out["bytes"] = (
                np.ctypeslib.as_array(res.data,
                                      shape=(int(res.data_len),)).copy(),
                np.ctypeslib.as_array(res.index,
                                      shape=(int(res.index_len),)).copy())
    finally:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    return out


def into_round(lib, views, n, device, n_slices, darr, iarr):
    res = engine.CompactIntoResult()
    st = engine.CompactIntoStats()
    t0 = now_ms()
    check(lib, lib.dbeel_gpu_compact_into(
        views, n, 0, device, 0, n_slices, darr.ctypes.data, darr.nbytes,
        iarr.ctypes.data, iarr.nbytes, 0, None, None, ctypes.byref(res),
        ctypes.byref(st)))
    wall = now_ms() - t0
    out = st.as_dict()
    out["call_ms"] = wall
    out["lens"] = (int(res.data_len), int(res.index_len))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()

    lib = engine._load_into(engine.load())
    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    print(f"workload built in {time.perf_counter() - t0:.1f}s", flush=True)
    n = len(runs)
    views, keepalive = engine._views(runs)
    dcap = sum(d.nbytes for d, _ in runs)
    icap = sum(i.nbytes for _, i in runs)
    # zeros() + fill: every page of the pageable destination exists already
    page_d, page_i = np.zeros(dcap, np.uint8), np.zeros(icap, np.uint8)
    page_d.fill(1)
    page_i.fill(1)
    pin_d, pin_i = np.zeros(dcap, np.uint8), np.zeros(icap, np.uint8)
    engine.pin_host(pin_d)
    engine.pin_host(pin_i)

    routes = (["compact", "into_pageable_1", "into_pinned_1"]
              + [f"into_pinned_{s}" for s in SLICE_COUNTS])
    samples = {r: [] for r in routes}
    checks = {}
    try:
        for rnd in range(args.warmup + args.reps):
            first = rnd == 0
            got = {"compact": baseline_round(lib, views, n, args.device,
                                             first)}
            want = got["compact"].pop("bytes", None)

            def same(darr, iarr, lens):
                return bool(np.array_equal(want[0], darr[:lens[0]])
                            and np.array_equal(want[1], iarr[:lens[1]]))

            got["into_pageable_1"] = into_round(lib, views, n, args.device, 1,
                                                page_d, page_i)
            if first:
                checks["into_pageable_1"] = same(
                    page_d, page_i, got["into_pageable_1"]["lens"])
            for s in (1,) + SLICE_COUNTS:
                name = f"into_pinned_{s}"
                got[name] = into_round(lib, views, n, args.device, s, pin_d,
                                       pin_i)
                if first:
                    checks[name] = same(pin_d, pin_i, got[name]["lens"])
                    pin_d.fill(0)  # the next route must write it all again
                    pin_i.fill(0)
            if first:
                print("checks:", json.dumps(checks), flush=True)
            if rnd < args.warmup:
                continue
            for r in routes:
                samples[r].append(got[r])
            print(f"round {rnd - args.warmup + 1}/{args.reps}: " + ", ".join(
                f"{r} {got[r]['wall_ms']:.0f}" for r in routes), flush=True)
    finally:
        engine.unpin_host(pin_d)
        engine.unpin_host(pin_i)

    last = samples["into_pinned_1"][-1]
    res = {
        "workload": "cfg3", "scale": args.scale, "n_runs": n,
        "input_bytes": dcap + icap, "output_bytes": sum(last["lens"]),
        "timed_at": "C ABI calls, host wall clock; h2d / kernel / d2h / "
                    "overlap are HIP events summed over slices; compact's "
                    "d2h_ms is wall - h2d - kernel (fetch + host allocation)",
        "warmup_rounds": args.warmup, "reps": args.reps,
        "routes": {
            r: {k: summarize([x[k] for x in samples[r]])
                for k in ("wall_ms", "h2d_ms", "kernel_ms", "d2h_ms",
                          "overlap_ms")}
            | {"slices": samples[r][-1]["slices"]}
            for r in routes},
        "checks": checks,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    del keepalive
    if not all(checks.values()):
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
