#!/usr/bin/env python3
"""Write-batch benchmark, timed at the C ABI (wall clock around the calls,
which end synchronised; no Python copies of the outputs).

State change measured: "a batch of writes in arrival order — unsorted, some
keys rewritten — is a resident table of an open reader".

  batch     dbeel_gpu_reader_write_batch of the unsorted batch, with the
            run fetched to the host (what a caller persists) and without;
  baseline  what the engine offered before: dbeel_gpu_encode_run of the
            stream ALREADY sorted and deduplicated on the host, then
            dbeel_gpu_reader_insert_run of the bytes it returned. The host
            sort is NOT charged to the baseline: it is done once, outside
            the timed region.

Shapes: 8,192 writes (the reference's DEFAULT_TREE_CAPACITY) and 2^20
writes, 32-B keys and 1 KiB values, 10 % of the writes rewriting an earlier
key; each once with random (distinct) 8-byte prefixes and once with every
key sharing its first 8 bytes. order_ms (HIP events) is recorded for both
DBEEL_BATCH_ORDER settings on all four, next to the unset default.

One warm-up round, then --reps interleaved rounds; median, min and max are
recorded. Every sample runs against a freshly opened one-run reader. The
paths are checked against each other: equal run bytes.

    python tools/bench_reader_write.py   # -> profiles/reader_write.json
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
from dbeel_amd.format import Entry, build_run  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_write.json")
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)
KLEN, VLEN = 32, 1024


def now_ms():
    return time.perf_counter() * 1e3


def check(lib, rc):
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())


def summarize(samples):
    return {"median": statistics.median(samples), "min": min(samples),
            "max": max(samples), "n": len(samples)}


class Arrays:
    """The five arrays of a batch of n fixed-size writes."""

    def __init__(self, keys, vals, ts_lo):
        n = len(keys)
        self.n = n
        self.keys = np.ascontiguousarray(keys)
        self.vals = np.ascontiguousarray(vals)
        self.koff = np.arange(n + 1, dtype=np.uint64) * KLEN
        self.voff = np.arange(n + 1, dtype=np.uint64) * VLEN
        self.ts = np.zeros((n, 2), dtype=np.uint64)
        self.ts[:, 0] = ts_lo

    def args(self):
        return (self.n, self.keys.ctypes.data_as(U8P),
                self.koff.ctypes.data_as(U64P), self.vals.ctypes.data_as(U8P),
                self.voff.ctypes.data_as(U64P), self.ts.ctypes.data_as(U8P))


def make_batch(n, shared_prefix, seed):
    """-> (unsorted batch, the same batch sorted by key with the last
    arrival of every key kept)."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n, KLEN), dtype=np.uint8)
    if shared_prefix:
        keys[:, :8] = np.frombuffer(b"user:000", dtype=np.uint8)
    # 10 % of the writes rewrite the key of an earlier write
    re = np.sort(rng.choice(np.arange(1, n), size=n // 10, replace=False))
    keys[re] = keys[(rng.random(len(re)) * re).astype(np.int64)]
    vals = np.empty((n, VLEN), dtype=np.uint8)
    vals[:] = np.arange(VLEN).astype(np.uint8)
    vals[:, :8] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    ts = rng.integers(1, 1 << 60, n).astype(np.uint64)
    batch = Arrays(keys, vals, ts)

    cols = keys.view(">u8")  # (n, 4) big-endian words: u64 order = byte order
    order = np.lexsort((np.arange(n), cols[:, 3], cols[:, 2], cols[:, 1],
                        cols[:, 0]))
    sk = cols[order]
    last = np.ones(n, dtype=bool)
    last[:-1] = (sk[1:] != sk[:-1]).any(axis=1)
    keep = order[last]
    return batch, Arrays(keys[keep], vals[keep], ts[keep])


def open_reader(lib, device):
    base = build_run([Entry(b"\xff" * 48, b"base", 0)])
    views, keepalive = engine._views([base])
    h = ctypes.c_void_p()
    check(lib, lib.dbeel_gpu_reader_open(views, None, 1, device,
                                         ctypes.byref(h)))
    del keepalive
    return h


def result_bytes(res):
    d = np.ctypeslib.as_array(res.data, shape=(int(res.data_len),)).copy()
    i = np.ctypeslib.as_array(res.index, shape=(int(res.index_len),)).copy()
    return d, i


def run_baseline(lib, srt, device, want_bytes):
    h = open_reader(lib, device)
    res = engine.CompactResult()
    t0 = now_ms()
    check(lib, lib.dbeel_gpu_encode_run(*srt.args(), device,
                                        ctypes.byref(res)))
    t1 = now_ms()
    view = engine.RunView(res.data, res.data_len, res.index, res.index_len)
    check(lib, lib.dbeel_gpu_reader_insert_run(h, 1, ctypes.byref(view),
                                               None))
    t2 = now_ms()
    out = result_bytes(res) if want_bytes else None
    lib.dbeel_gpu_result_free(ctypes.byref(res))
    lib.dbeel_gpu_reader_close(h)
    return {"total": t2 - t0, "encode_run": t1 - t0,
            "insert_run": t2 - t1}, out


def run_batch(lib, batch, device, fetch, order, want_bytes):
    h = open_reader(lib, device)
    res = engine.CompactResult()
    st = engine.WriteBatchStats()
    if order:
        os.environ["DBEEL_BATCH_ORDER"] = order
    try:
        t0 = now_ms()
        rc = lib.dbeel_gpu_reader_write_batch(
            h, 1, *batch.args(), 0, ctypes.byref(res) if fetch else None,
            None, None, ctypes.byref(st))
        t1 = now_ms()
    finally:
        os.environ.pop("DBEEL_BATCH_ORDER", None)
    check(lib, rc)
    out = result_bytes(res) if (fetch and want_bytes) else None
    if fetch:
        lib.dbeel_gpu_result_free(ctypes.byref(res))
    lib.dbeel_gpu_reader_close(h)
    return {"total": t1 - t0, **st.as_dict()}, out


def bench_shape(lib, name, n, shared, device, reps):
    batch, srt = make_batch(n, shared, seed=n + int(shared))
    variants = {
        "baseline_encode_then_insert":
            lambda wb: run_baseline(lib, srt, device, wb),
        "write_batch_fetch":
            lambda wb: run_batch(lib, batch, device, True, None, wb),
        "write_batch_nofetch":
            lambda wb: run_batch(lib, batch, device, False, None, wb),
        "write_batch_nofetch_merge":
            lambda wb: run_batch(lib, batch, device, False, "merge", wb),
        "write_batch_nofetch_radix":
            lambda wb: run_batch(lib, batch, device, False, "radix", wb),
        "write_batch_fetch_radix":
            lambda wb: run_batch(lib, batch, device, True, "radix", wb),
    }
    # warm-up round, which is also the cross-check
    outs = {k: f(True)[1] for k, f in variants.items()}
    ref = outs["baseline_encode_then_insert"]
    for k in ("write_batch_fetch", "write_batch_fetch_radix"):
        assert np.array_equal(outs[k][0], ref[0]), f"{name} {k}: data differs"
        assert np.array_equal(outs[k][1], ref[1]), f"{name} {k}: index differs"
    del outs, ref
    del variants["write_batch_fetch_radix"]
    samples = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():  # interleaved
            samples[k].append(f(False)[0])
    rec = {"writes": n, "entries_out": srt.n, "shared_prefix": shared,
           "key_bytes": KLEN, "value_bytes": VLEN,
           "input_bytes": int(n * (KLEN + VLEN + 32))}
    for k, rows in samples.items():
        rec[k] = {f: summarize([r[f] for r in rows])
                  for f in rows[0] if f.endswith("_ms") or f in
                  ("total", "encode_run", "insert_run")}
        if "prefix_tied" in rows[0]:
            rec[k]["prefix_tied"] = rows[0]["prefix_tied"]
    b = rec["baseline_encode_then_insert"]["total"]
    rec["baseline_spread_ms"] = b["max"] - b["min"]
    rec["nofetch_minus_baseline_ms"] = (
        rec["write_batch_nofetch"]["total"]["median"] - b["median"])
    rec["order_ms_radix_settle"] = rec["write_batch_nofetch_radix"]["order_ms"]
    rec["order_ms_single_merge"] = rec["write_batch_nofetch_merge"]["order_ms"]
    print(f"{name}: baseline {b['median']:.2f} ms "
          f"[{b['min']:.2f}, {b['max']:.2f}]  "
          f"fetch {rec['write_batch_fetch']['total']['median']:.2f}  "
          f"nofetch {rec['write_batch_nofetch']['total']['median']:.2f}  "
          f"order radix {rec['order_ms_radix_settle']['median']:.3f} / "
          f"merge {rec['order_ms_single_merge']['median']:.3f}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=1 << 20,
                    help="writes in the large shape")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    lib = engine._load_reader()
    shapes = {}
    for n in (8192, args.big):
        for shared in (False, True):
            name = f"{n}_{'shared' if shared else 'distinct'}_prefix"
            shapes[name] = bench_shape(lib, name, n, shared, args.device,
                                       args.reps)
    out = {
        "what": "reader write batch vs encode_run + insert_run, C ABI wall "
                "ms; the baseline's host sort + dedup is not timed",
        "reps": args.reps, "shapes": shapes,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
