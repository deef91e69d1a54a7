#!/usr/bin/env python3
"""Replicated-read benchmark at the cfg3 workload (8 runs x ~1 GiB, 32-B
keys, 1 KiB values): bench_reader.py's 1 M-key batch, half present and half
absent, answered by a local reader and two replicas. The replicas are readers
over copies of the same runs with a third of the timestamps perturbed, so
every candidate wins some keys and many tie.

Three routes, interleaved round by round in one process, timed at the C ABI:
  - merged_answers: dbeel_gpu_reader_get_merged with the replicas' answers
    as two ANSWERS sources (their get_entries outputs, pinned host memory);
  - host_route: what a caller has without it — get_entries on the local
    reader into pinned buffers, then a numpy merge on the host over the three
    answer sets (timestamps compared as signed high / unsigned low halves,
    the later candidate winning ties, winners' records packed);
  - merged_readers: get_merged with the two replicas as same-GPU READER
    sources, where no replica bytes cross PCIe.
The three must deliver the same offsets and record bytes.

    python tools/bench_reader_merged.py    # -> profiles/reader_merged.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_reader import (Batch, EntryBuffers, U8P, U64P,  # noqa: E402
                          get_entries, make_queries, summarize)
from dbeel_amd import engine  # noqa: E402
from dbeel_amd.genruns import make_config  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "profiles", "reader_merged.json")
STAGES = ("h2d_ms", "search_ms", "pick_ms", "gather_ms", "d2h_ms")


def perturbed(runs, seed):
    """Copies of runs with a third of the timestamps moved by up to +-500
    (clamped at 0): each entry's low timestamp half is its last-16th..9th
    byte."""
    rng = np.random.default_rng(seed)
    out = []
    col = np.arange(8, dtype=np.int64)[None, :]
    for data, index in runs:
        data = data.copy()
        rec = np.frombuffer(index, dtype="<u8").reshape(-1, 2)
        off = rec[:, 0].astype(np.int64)
        full = (rec[:, 1] >> np.uint64(32)).astype(np.int64)
        sel = np.flatnonzero(rng.random(len(off)) < 1 / 3)
        at = (off[sel] + full[sel] - 16)[:, None] + col
        lo = np.ascontiguousarray(data[at]).view("<u8").reshape(-1)
        moved = lo.astype(np.int64) + rng.integers(-500, 501, len(sel))
        lo = np.maximum(moved, 0).astype("<u8")
        data[at] = lo.view(np.uint8).reshape(-1, 8)
        out.append((data, index))
    return out


class MergeBufs:
    """Caller-owned, pinned buffers of one get_merged call."""

    def __init__(self, n, cap):
        self.hits = np.empty(n, dtype=engine.MERGE_HIT_DTYPE)
        self.roff = np.empty(n + 1, dtype=np.uint64)
        self.rec = np.zeros(max(cap, 1), dtype=np.uint8)
        self.cap = cap
        for a in (self.hits, self.roff, self.rec):
            engine.pin_host(a)

    def buf(self):
        return engine.MergeBuffers(
            self.hits.ctypes.data_as(ctypes.POINTER(engine.MergeHit)),
            self.roff.ctypes.data_as(U64P), self.rec.ctypes.data_as(U8P),
            self.cap)

    def release(self):
        for a in (self.hits, self.roff, self.rec):
            engine.unpin_host(a)


def get_merged(lib, rd, batch, srcs, n_src, bufs):
    b = bufs.buf()
    page, st = engine.GetPage(), engine.MergeStats()
    t0 = time.perf_counter()
    rc = lib.dbeel_gpu_reader_get_merged(
        rd._h, batch.blob_p, batch.off_p, batch.n, srcs, n_src,
        ctypes.byref(b), ctypes.byref(page), ctypes.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise engine.DbeelGpuError(rc, lib.dbeel_gpu_last_error().decode())
    assert page.n_done == batch.n
    d = st.as_dict()
    d["wall_ms"] = wall
    return d, int(page.records_len)


def host_merge(answers, out_roff, out_rec):
    """The numpy merge over answer sets [(offsets, records), ...], the local
    one last: -> records_len. Timestamps are gathered per candidate, the
    winner is the greatest (signed high, unsigned low), the later candidate
    on ties; the winners' records are packed group by group of equal
    (candidate, length) with strided window gathers."""
    n = len(answers[0][0]) - 1
    col = np.arange(16, dtype=np.int64)[None, :]
    best_hi = np.zeros(n, dtype=np.int64)
    best_lo = np.zeros(n, dtype=np.uint64)
    win = np.full(n, -1, dtype=np.int64)
    for c, (off, rec) in enumerate(answers):
        off = off.astype(np.int64)
        present = np.flatnonzero(off[1:] > off[:-1])
        ts = np.ascontiguousarray(
            rec[(off[1:][present] - 16)[:, None] + col]).view("<u8")
        lo, hi = ts[:, 0], ts[:, 1].view(np.int64)
        bh, bl, bw = best_hi[present], best_lo[present], win[present]
        take = (bw < 0) | (hi > bh) | ((hi == bh) & (lo >= bl))
        t = present[take]
        best_hi[t], best_lo[t], win[t] = hi[take], lo[take], c
    lens = np.zeros(n, dtype=np.int64)
    starts = np.zeros(n, dtype=np.int64)
    for c, (off, _) in enumerate(answers):
        off = off.astype(np.int64)
        mine = win == c
        lens[mine] = (off[1:] - off[:-1])[mine]
        starts[mine] = off[:-1][mine]
    out_roff[0] = 0
    np.cumsum(lens, out=out_roff[1:].view(np.int64))
    dst = out_roff[:-1].view(np.int64)
    windows = np.lib.stride_tricks.sliding_window_view
    for c, (_, rec) in enumerate(answers):
        mine = win == c
        for L in np.unique(lens[mine]):
            if L == 0:
                continue
            g = np.flatnonzero(mine & (lens == L))
            windows(out_rec, int(L), writeable=True)[dst[g]] = \
                windows(rec, int(L))[starts[g]]
    return int(out_roff[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of cfg3's entries per run")
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()

    lib = engine._load_reader()
    t0 = time.perf_counter()
    runs = make_config("cfg3", scale=args.scale)
    batch = Batch(make_queries(runs, args.keys, 32, seed=0xBEAD))
    n = batch.n
    local = engine.Reader(runs, device=args.device)
    replicas = []
    for seed in (1, 2):
        copy = perturbed(runs, seed)
        replicas.append(engine.Reader(copy, device=args.device))
        del copy
    input_bytes = sum(d.nbytes + i.nbytes for d, i in runs)
    del runs
    print(f"workload and readers built in {time.perf_counter() - t0:.1f}s",
          flush=True)

    held = []
    try:
        # the replicas' answers: their get_entries outputs, pinned
        answers = []
        for rep in replicas:
            probe = EntryBuffers(n, 0, False)
            rc, _, _, page = get_entries(lib, rep, batch, probe)
            assert rc in (0, 3), rc
            eb = EntryBuffers(n, page["records_total"], True)
            held.append(eb)
            rc, _, _, page = get_entries(lib, rep, batch, eb)
            assert rc == 0 and page["n_done"] == n
            answers.append((eb.roff, eb.rec[:page["records_total"]]))
        probe = EntryBuffers(n, 0, False)
        rc, _, _, page = get_entries(lib, local, batch, probe)
        local_eb = EntryBuffers(n, page["records_total"], True)
        held.append(local_eb)
        src_a, keep_a = engine.Reader._merge_sources(answers)
        src_r, keep_r = engine.Reader._merge_sources(replicas)
        # a call with cap 0 sizes the merged output
        sizing = MergeBufs(n, 0)
        b, sized = sizing.buf(), engine.GetPage()
        rc = lib.dbeel_gpu_reader_get_merged(
            local._h, batch.blob_p, batch.off_p, n, src_a, 2,
            ctypes.byref(b), ctypes.byref(sized), None)
        sizing.release()
        assert rc in (0, 3), rc
        cap = int(sized.records_total)
        out_a, out_r = MergeBufs(n, cap), MergeBufs(n, cap)
        held += [out_a, out_r]
        host_roff = np.empty(n + 1, dtype=np.uint64)
        host_rec = np.zeros(max(cap, 1), dtype=np.uint8)
        rows = {"merged_answers": {k: [] for k in STAGES + ("wall_ms",)},
                "merged_readers": {k: [] for k in STAGES + ("wall_ms",)},
                "host_route": {k: [] for k in (
                    "get_entries_wall_ms", "get_entries_d2h_ms",
                    "host_merge_ms", "wall_ms")}}
        checks = {}
        for rnd in range(args.warmup + args.reps):
            st_a, len_a = get_merged(lib, local, batch, src_a, 2, out_a)
            rc, ge_wall, ge_st, ge_page = get_entries(lib, local, batch,
                                                      local_eb)
            assert rc == 0 and ge_page["n_done"] == n
            t1 = time.perf_counter()
            len_h = host_merge(
                answers + [(local_eb.roff,
                            local_eb.rec[:ge_page["records_total"]])],
                host_roff, host_rec)
            merge_ms = (time.perf_counter() - t1) * 1e3
            st_r, len_r = get_merged(lib, local, batch, src_r, 2, out_r)
            if rnd == 0:
                checks["offsets_equal"] = bool(
                    np.array_equal(out_a.roff, host_roff)
                    and np.array_equal(out_r.roff, host_roff))
                checks["records_equal"] = bool(
                    len_a == len_h == len_r
                    and np.array_equal(out_a.rec[:len_a], host_rec[:len_h])
                    and np.array_equal(out_r.rec[:len_r], host_rec[:len_h]))
                checks["hits_equal"] = bool(
                    np.array_equal(out_a.hits, out_r.hits))
                winners = {str(s): int((out_a.hits["source"] == s).sum())
                           for s in (-1, 0, 1, 2)}
                stale_any = int((out_a.hits["stale_mask"] != 0).sum())
                counters = {k: st_a[k] for k in ("winners", "tombstones",
                                                 "from_local")}
                records_len = len_a
            if rnd < args.warmup:
                continue
            for k in rows["merged_answers"]:
                rows["merged_answers"][k].append(st_a[k])
                rows["merged_readers"][k].append(st_r[k])
            h = rows["host_route"]
            h["get_entries_wall_ms"].append(ge_wall)
            h["get_entries_d2h_ms"].append(ge_st["d2h_ms"])
            h["host_merge_ms"].append(merge_ms)
            h["wall_ms"].append(ge_wall + merge_ms)
        del keep_a, keep_r
        res = {
            "workload": "cfg3", "scale": args.scale,
            "input_bytes": input_bytes, "batch_keys": n, "present_frac": 0.5,
            "warmup": args.warmup, "reps": args.reps,
            "method": "three routes interleaved round by round in one "
                      "process; wall at the C ABI call (host_route: "
                      "get_entries call + numpy merge), stages HIP events",
            "replicas": "readers over copies of the runs, a third of the "
                        "timestamps moved by up to +-500",
            "pinned_buffers": "answers, get_entries outputs, merged outputs",
            "answer_bytes_up": [int(len(a[1])) + 8 * (n + 1)
                                for a in answers],
            "local_records_total": int(ge_page["records_total"]),
            "merged_records_len": records_len,
            "winners_by_source": winners, "queries_with_stale": stale_any,
            "counters": counters,
            "rows": {r: {k: summarize(v) for k, v in d.items()}
                     for r, d in rows.items()},
            "checks": checks,
        }
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        if not all(checks.values()):
            sys.exit("the three routes disagree")
    finally:
        for b in held:
            b.release()
        for r in replicas:
            r.close()
        local.close()


if __name__ == "__main__":
    main()
