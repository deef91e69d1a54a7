"""CPU-side checks of dbeel_gpu_job_fetch_into / dbeel_gpu_compact_into /
dbeel_lsm_compact_stream: the symbols and types are declared and exported,
the ctypes mirrors match the header, and everything the header says is
refused on the host IS refused before any device access — so these run
without a GPU. What needs a device is in test_stream_compact_gpu.py."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from conftest import REPO_ROOT
from dbeel_amd.genruns import make_runs

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

INVALID_ARG, CORRUPT = 1, 2
GUARD = 0xA5


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def _lib():
    _built()
    from dbeel_amd.engine import _load_into, load

    return _load_into(load())


def test_symbols_and_types_declared_and_exported():
    lib = ctypes.CDLL(_built())
    gpu = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    lsm = open(os.path.join(REPO_ROOT, "include", "dbeel_lsm.h")).read()
    for sym, hdr in (("dbeel_gpu_job_fetch_into", gpu),
                     ("dbeel_gpu_compact_into", gpu),
                     ("dbeel_lsm_compact_stream", lsm)):
        assert re.search(r"\bint\s+%s\(" % sym, hdr), sym
        assert getattr(lib, sym, None) is not None, sym
    for t in ("dbeel_compact_into_result", "dbeel_compact_into_stats"):
        assert re.search(r"\}\s*%s;" % t, gpu), t
    # the header states where the output rebase happens and the cap promise
    assert "INTO SCRATCH" in gpu and "can never be refused" in gpu


def test_struct_mirrors_match_header_layout():
    _built()
    from dbeel_amd.engine import CompactIntoResult, CompactIntoStats

    assert ctypes.sizeof(CompactIntoResult) == 24
    assert ctypes.sizeof(CompactIntoStats) == 64
    assert [f for f, _ in CompactIntoResult._fields_] == [
        "data_len", "index_len", "entries_written"]
    assert [f for f, _ in CompactIntoStats._fields_] == [
        "slices", "bytes_in", "bytes_out", "h2d_ms", "kernel_ms", "d2h_ms",
        "wall_ms", "overlap_ms"]
    assert CompactIntoStats.h2d_ms.offset == 24
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for name, cls in (("dbeel_compact_into_result", CompactIntoResult),
                      ("dbeel_compact_into_stats", CompactIntoStats)):
        body = hdr[:hdr.index("} %s;" % name)]
        body = body[body.rindex("typedef struct {"):]
        pos = [re.search(r"\b%s[;,]" % f, body).start()
               for f, _ in cls._fields_]
        assert pos == sorted(pos), name


class _Call:
    """One dbeel_gpu_compact_into call over guarded output arrays; every
    argument can be knocked out by name."""

    def __init__(self, runs, n_slices=2):
        from dbeel_amd.engine import (CompactIntoResult, CompactIntoStats,
                                      _views)

        self.views, self.keep = _views(runs)
        self.n_runs = len(runs)
        self.n_slices = n_slices
        self.data = np.full(1 << 16, GUARD, dtype=np.uint8)
        self.index = np.full(1 << 12, GUARD, dtype=np.uint8)
        self.res = CompactIntoResult(7, 7, 7)
        self.st = CompactIntoStats()
        self.st.slices = 7
        self.bp = ctypes.POINTER(ctypes.c_uint8)()
        self.bn = ctypes.c_uint64(7)

    def __call__(self, lib, device=0, want_bloom=0, **null):
        def arg(name, value):
            return None if null.get(name) else value

        return lib.dbeel_gpu_compact_into(
            arg("runs", self.views), self.n_runs, 0, device, 0,
            self.n_slices, arg("data", self.data.ctypes.data),
            self.data.nbytes, arg("index", self.index.ctypes.data),
            self.index.nbytes, want_bloom,
            arg("bloom_bytes", ctypes.byref(self.bp)),
            arg("bloom_len", ctypes.byref(self.bn)),
            arg("result", ctypes.byref(self.res)), ctypes.byref(self.st))

    def untouched(self):
        return bool((self.data == GUARD).all() and (self.index == GUARD).all())

    def zeroed(self, bloom_len_given=True):
        return ((self.res.data_len, self.res.index_len,
                 self.res.entries_written, self.st.slices)
                == (0, 0, 0, 0) and not self.bp
                and self.bn.value == (0 if bloom_len_given else 7))


def _runs():
    return make_runs(3, 200, 16, 32, overlap_frac=0.5, seed=5)


def test_compact_into_refusals_in_header_order():
    """NULL result first (nothing else is touched), then with the outputs
    zeroed: NULL data / index, want_bloom without its outputs, NULL or empty
    runs, device < 0, a bad run view. Each wins over everything after it."""
    lib = _lib()
    c = _Call(_runs())
    # 1. NULL result: nothing zeroed, whatever else is wrong
    assert c(lib, device=-1, result=True, data=True) == INVALID_ARG
    assert c.st.slices == 7 and c.bn.value == 7

    steps = [
        dict(data=True), dict(index=True),
        dict(want_bloom=1, bloom_bytes=True), dict(want_bloom=1, bloom_len=True),
        dict(runs=True),
    ]
    # each refusal holds with every LATER fault present too (device = -1)
    for kw in steps:
        c = _Call(_runs())
        assert c(lib, device=-1, **kw) == INVALID_ARG, kw
        assert c.zeroed(not kw.get("bloom_len")) and c.untouched(), kw
        msg = lib.dbeel_gpu_last_error().decode()
        assert "device" not in msg, (kw, msg)

    c = _Call(_runs())
    c.n_runs = 0
    assert c(lib, device=-1) == INVALID_ARG
    assert "device" not in lib.dbeel_gpu_last_error().decode()

    # device < 0 comes before the run views are looked at
    bad = _runs()
    bad[1] = (bad[1][0], bad[1][1][:-3])       # index_len % 16 != 0
    c = _Call(bad)
    assert c(lib, device=-1) == INVALID_ARG
    assert "device" in lib.dbeel_gpu_last_error().decode()
    assert c.zeroed() and c.untouched()


def test_compact_into_bad_views_refused_before_the_device():
    """job_create's view checks, with a device ordinal no machine has: a
    refusal other than NO_GPU / HIP proves that no device call was made."""
    from dbeel_amd.engine import RunView

    lib = _lib()
    bad = _runs()
    bad[1] = (bad[1][0], bad[1][1][:-3])
    c = _Call(bad)
    assert c(lib, device=1 << 20) == CORRUPT
    assert c.zeroed() and c.untouched()

    c = _Call(_runs())
    c.views[2].data = ctypes.POINTER(ctypes.c_uint8)()   # NULL, data_len > 0
    assert c(lib, device=1 << 20) == INVALID_ARG
    assert c.zeroed() and c.untouched()

    c = _Call(_runs())
    many = (RunView * 65)(*([c.views[0]] * 65))
    c.views, c.n_runs = many, 65
    assert c(lib, device=1 << 20) == INVALID_ARG
    assert c.zeroed() and c.untouched()


@pytest.mark.parametrize("where", ["pivot", "probe", "boundary"])
def test_corrupt_record_refused_during_pivot_selection(where):
    """An index record pointing outside its run, met while the slices are
    laid out on the host (n_slices forces slicing), is CORRUPT — and it is
    reported before the device is touched: device 2^20 does not exist, so
    any device call would have answered NO_GPU instead."""
    lib = _lib()
    runs = [list(r) for r in make_runs(3, 400, 16, 32, seed=12)]
    far = np.frombuffer(struct.pack("<Q", 1 << 40), dtype=np.uint8)
    if where == "pivot":
        # runs are equally long: run 0 gives the pivots; 2 slices -> entry 200
        r, i = 0, 200
    elif where == "probe":
        # the first bisection probe of a run that gives no pivot
        r, i = 2, 200
    else:
        # the record AT a slice boundary supplies the slice's first data
        # offset: find run 1's boundary on clean inputs, then break it
        from dbeel_amd.format import parse_run

        pivot = parse_run(bytes(runs[0][0]), bytes(runs[0][1]))[200].key
        keys = [e.key for e in parse_run(bytes(runs[1][0]), bytes(runs[1][1]))]
        r, i = 1, next(n for n, k in enumerate(keys) if k >= pivot)
    idx = runs[r][1].copy()
    idx[i * 16: i * 16 + 8] = far
    runs[r][1] = idx
    c = _Call([tuple(x) for x in runs], n_slices=2)
    assert c(lib, device=1 << 20) == CORRUPT
    assert "corrupt index record in run %d" % r in \
        lib.dbeel_gpu_last_error().decode()
    assert c.zeroed() and c.untouched()


def test_clean_inputs_reach_the_device():
    """The counterpart of the refusals above: with nothing wrong on the host
    the same call goes on to the device (and, without one, says so)."""
    lib = _lib()
    c = _Call(_runs())
    assert c(lib, device=1 << 20) == 5  # NO_GPU


def test_fetch_into_null_arguments():
    lib = _lib()
    data = np.full(64, GUARD, dtype=np.uint8)
    index = np.full(64, GUARD, dtype=np.uint8)
    dl, il = ctypes.c_uint64(7), ctypes.c_uint64(7)
    ms = ctypes.c_double(7.0)
    rc = lib.dbeel_gpu_job_fetch_into(
        None, data.ctypes.data, 64, index.ctypes.data, 64, 0,
        ctypes.byref(dl), ctypes.byref(il), ctypes.byref(ms))
    assert rc == INVALID_ARG
    assert (dl.value, il.value, ms.value) == (0, 0, 0.0)
    assert (data == GUARD).all() and (index == GUARD).all()


def test_lsm_compact_stream_host_refusals(tmp_path):
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    runs = _runs()
    for i, (d, x) in zip((0, 2, 4), runs):
        lsm.write_run_files(str(tmp_path), i, bytes(d), bytes(x))
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DbeelGpuError) as ei:
        lsm.compact_stream(str(tmp_path), [0, 2, 4], 5, False, device=-1)
    assert ei.value.code == INVALID_ARG
    with pytest.raises(DbeelGpuError) as ei:
        lsm.compact_stream(str(tmp_path), [0, 2, 6], 5, False, device=0)
    assert ei.value.code == 7  # IO: no such input
    assert sorted(os.listdir(tmp_path)) == before
