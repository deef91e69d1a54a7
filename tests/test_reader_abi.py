"""CPU-side checks of the resident-reader ABI: the symbols are declared and
exported, and every argument/shape check of dbeel_gpu_reader_open fires
before any device access (so these run without a GPU)."""
import ctypes
import os
import struct

import pytest

from conftest import REPO_ROOT

LIB = os.path.join(REPO_ROOT, "dbeel_amd", "libdbeel_gpu.so")

READER_SYMBOLS = [
    "dbeel_gpu_reader_open",
    "dbeel_gpu_reader_table_bytes",
    "dbeel_gpu_reader_get",
    "dbeel_gpu_get_result_free",
    "dbeel_gpu_reader_close",
]


def _built():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    return LIB


def _run():
    from dbeel_amd.format import Entry, build_run

    return build_run([Entry(b"a", b"b", 1)])


def _bloom(magic=b"DBLM", version=1, k=7, n_bits=64, seed=0xDBEE1,
           bitmap_len=None):
    if bitmap_len is None:
        bitmap_len = (n_bits + 7) // 8
    return (magic + struct.pack("<IIIQQ", version, k, 0, n_bits, seed)
            + b"\xff" * bitmap_len)


def test_reader_symbols_declared_and_exported():
    lib = ctypes.CDLL(_built())
    hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_gpu.h")).read()
    for sym in READER_SYMBOLS:
        assert sym in hdr, sym
        assert getattr(lib, sym, None) is not None, sym
    for t in ("dbeel_bloom_view", "dbeel_get_result", "dbeel_get_stats"):
        assert t in hdr, t
    lsm_hdr = open(os.path.join(REPO_ROOT, "include", "dbeel_lsm.h")).read()
    assert "dbeel_lsm_reader_open" in lsm_hdr
    assert getattr(lib, "dbeel_lsm_reader_open", None) is not None
    # already exported, now reachable from Python
    assert getattr(lib, "dbeel_gpu_job_bloom", None) is not None


def test_reader_device_minus_one_rejected():
    _built()
    from dbeel_amd.engine import DbeelGpuError, Reader

    with pytest.raises(DbeelGpuError) as ei:
        Reader([_run()], device=-1)
    assert ei.value.code == 1  # INVALID_ARG


def test_reader_65_runs_rejected():
    _built()
    from dbeel_amd.engine import DbeelGpuError, Reader

    with pytest.raises(DbeelGpuError) as ei:
        Reader([_run()] * 65, device=0)
    assert ei.value.code == 1  # INVALID_ARG


@pytest.mark.parametrize(
    "bloom",
    [
        _bloom(magic=b"XBLM"),
        _bloom(version=2),
        _bloom(n_bits=4096, bitmap_len=100),  # header implies 512 B
        b"DBLM" + b"\0" * 8,                  # shorter than the header
        _bloom(n_bits=0, bitmap_len=8),       # modulus would be zero
    ],
    ids=["magic", "version", "short_bitmap", "short_header", "zero_bits"],
)
def test_reader_bad_filter_rejected(bloom):
    """A bad filter is CORRUPT, decided on the host: device=0 is passed and
    the answer must not depend on whether a GPU exists."""
    _built()
    from dbeel_amd.engine import DbeelGpuError, Reader

    # the bad filter sits on the second run: every filter is checked
    with pytest.raises(DbeelGpuError) as ei:
        Reader([_run(), _run()], blooms=[_bloom(), bloom], device=0)
    assert ei.value.code == 2  # CORRUPT


def test_reader_run_count_checked_before_filters():
    """open's order: run validation first, then the filters — 65 runs with
    corrupt filters report the run count."""
    _built()
    from dbeel_amd.engine import DbeelGpuError, Reader

    with pytest.raises(DbeelGpuError) as ei:
        Reader([_run()] * 65, blooms=[_bloom(magic=b"XBLM")] * 65, device=0)
    assert ei.value.code == 1  # run count is checked before the filters


def test_lsm_reader_open_refuses_pending_journal(tmp_path):
    """A leftover .compact_action means a half-swapped directory: IO error
    with a replay-first message, before any device access, and the
    directory is left exactly as it was."""
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    d, i = _run()
    lsm.write_run_files(str(tmp_path), 0, d, i)
    (tmp_path / f"{1:020d}.compact_action").write_bytes(b"\0" * 16)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DbeelGpuError) as ei:
        lsm.open_reader(str(tmp_path), device=0)
    assert ei.value.code == 7  # IO
    assert "replay" in str(ei.value)
    assert sorted(os.listdir(tmp_path)) == before


def test_lsm_reader_open_refuses_more_than_64_sstables(tmp_path):
    _built()
    from dbeel_amd import lsm
    from dbeel_amd.engine import DbeelGpuError

    d, i = _run()
    for n in range(65):
        lsm.write_run_files(str(tmp_path), 2 * n, d, i)
    with pytest.raises(DbeelGpuError) as ei:
        lsm.open_reader(str(tmp_path), device=0)
    assert ei.value.code == 1  # INVALID_ARG
    assert "compact" in str(ei.value)


def test_reader_get_key_batch_refusals_name_their_caller():
    """A key batch whose offsets descend, or of 2^32 keys, is refused before
    the reader handle is looked at or any device call is made: a zeroed
    buffer stands in for the reader. The message is reader_get's own and
    names the index; the result is left zeroed."""
    import numpy as np

    _built()
    from dbeel_amd.engine import GetResult, _load_reader

    lib = _load_reader()
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    ka = np.frombuffer(b"abcdef", dtype=np.uint8)
    koff = np.array([0, 4, 2, 6], dtype=np.uint64)  # descends at index 1
    kp, op = ka.ctypes.data_as(u8p), koff.ctypes.data_as(u64p)
    fake = (ctypes.c_uint8 * 8192)()
    call = lib.dbeel_gpu_reader_get
    for n, text in ((3, b"reader_get: key_offsets not ascending at 1"),
                    (1 << 32, b"reader_get: 2^32 or more keys in one batch")):
        res = GetResult()
        res.n_keys = res.values_len = 9
        assert call(fake, kp, op, n, ctypes.byref(res), None) == 1
        assert lib.dbeel_gpu_last_error() == text
        assert not bytes(res).strip(b"\0")
    assert not bytes(fake).strip(b"\0")
