"""bench.py --dump-outputs writer (CPU): file set, dtypes, exactness of the
sampled records against the output they were drawn from, determinism, and
sensitivity of the block checksums to a single flipped byte."""
import os

import numpy as np
import pytest

import bench
import oracle
from dbeel_amd.format import INDEX_DTYPE
from dbeel_amd.genruns import make_runs

NAMES = ["data_blocks", "index_blocks", "sample_data", "sample_ids",
         "sample_index", "summary"]


@pytest.fixture(scope="module")
def results():
    out = []
    for j in range(2):
        runs = make_runs(3, 700, 16, 64, overlap_frac=0.5,
                         tombstone_frac=0.1, seed=77 + j)
        out.append(oracle.compact(runs, keep_tombstones=True))
    return out


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_files_and_sample_exact(tmp_path, results):
    bench.dump_outputs(str(tmp_path), results)
    got = _load(tmp_path)
    assert sorted(got) == sorted(
        f"job{j}_{n}.npy" for j in range(2) for n in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for j, (data, index, n) in enumerate(results):
        assert list(got[f"job{j}_summary.npy"]) == [len(data), len(index), n]
        recs = np.frombuffer(index, dtype=INDEX_DTYPE)
        ids = got[f"job{j}_sample_ids.npy"].astype(np.int64)
        assert ids.size == min(n, bench.DUMP_SAMPLE_ENTRIES // 2)
        assert np.all(np.diff(ids) > 0)
        si = got[f"job{j}_sample_index.npy"]
        for c, f in enumerate(("offset", "key_size", "full_size")):
            assert np.array_equal(si[:, c], recs[f][ids].astype(np.float64))
        d = np.frombuffer(data, dtype=np.uint8)
        want = np.concatenate([d[int(o): int(o) + int(f)]
                               for o, _, f in si])
        assert np.array_equal(got[f"job{j}_sample_data.npy"], want)
        blocks = got[f"job{j}_data_blocks.npy"]
        assert blocks.size == -(-len(data) // bench.DUMP_DATA_BLOCK)
        pad = np.zeros(-len(data) % 4, dtype=np.uint8)
        words = np.concatenate([d, pad]).view("<u4")
        assert blocks.sum() == float(words.sum(dtype=np.uint64))


def test_dump_deterministic_and_byte_sensitive(tmp_path, results):
    a, b, c = (str(tmp_path / x) for x in "abc")
    bench.dump_outputs(a, results)
    bench.dump_outputs(b, results)
    A, B = _load(a), _load(b)
    assert all(np.array_equal(A[f], B[f]) for f in A)
    data, index, n = results[0]
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 1
    bench.dump_outputs(c, [(bytes(flipped), index, n), results[1]])
    C = _load(c)
    assert not np.array_equal(A["job0_data_blocks.npy"],
                              C["job0_data_blocks.npy"])
    assert np.array_equal(A["job1_data_blocks.npy"],
                          C["job1_data_blocks.npy"])
