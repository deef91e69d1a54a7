"""Bit-exact host restatement of the device-built "DBLM" filter, for the tests
that pin the bitmap's bytes. numpy only, never the code under test.

Every device builder (dbeel_gpu_job_bloom, the filter across slices of
compact_into, and the adopt path of write_batch / memtable_flush /
compact_begin) writes the same file for the same key set:

  header, 32 bytes (include/dbeel_lsm.h):
      "DBLM" | version:u32 = 1 | k:u32 = 7 | pad:u32 = 0
      | n_bits:u64 | seed:u64 = 0xDBEE1
  bitmap, (n_bits + 7) // 8 bytes, NO padding after it: bit b is bit (b & 7)
      of byte b >> 3 (the device sets bit (b & 31) of little-endian u32 word
      b >> 5, which is the same bit). The spare bits of the last byte stay 0.

  n_bits = int(9.585 * max(n, 1)) + 64          (n = number of keys)
  fnv(key, s) = splitmix64_finalizer(FNV-1a-64 over key, basis ^ s)
  h1 = fnv(key, seed); h2 = fnv(key, seed ^ 0x9e3779b97f4a7c15) | 1
  bit_j = (h1 + j * h2) mod 2^64 mod n_bits     for j in 0..6

The length was read off dbeel_gpu_job_bloom: it allocates 32 + (n_bits + 7)
// 8 (+ 4 spare bytes it never reports) and returns exactly that many.

Keys are the rows of a (n, K) uint8 matrix: fixed width, vectorised over the
keys with a loop over the K byte columns. All arithmetic is uint64 with
wrap-around.
"""
import struct

import numpy as np

K_HASHES = 7
SEED = 0xDBEE1
HEADER_LEN = 32

_U = np.uint64
_FNV_BASIS = 1469598103934665603
_FNV_PRIME = _U(1099511628211)
_GOLDEN = 0x9E3779B97F4A7C15


def n_bits_for(n: int) -> int:
    return int(9.585 * float(n if n else 1)) + 64


def _mix64(h):
    h = h ^ (h >> _U(30))
    h = h * _U(0xBF58476D1CE4E5B9)
    h = h ^ (h >> _U(27))
    h = h * _U(0x94D049BB133111EB)
    return h ^ (h >> _U(31))


def _fnv(keys, seed: int):
    keys = np.asarray(keys, dtype=np.uint8)
    h = np.full(keys.shape[0], (_FNV_BASIS ^ seed) & (2**64 - 1), dtype=_U)
    for c in range(keys.shape[1]):
        h = (h ^ keys[:, c].astype(_U)) * _FNV_PRIME
    return _mix64(h)


def bit_positions(keys, n_bits: int, seed: int = SEED) -> np.ndarray:
    """(n, 7) uint64: the bits each key sets, in probe order."""
    h1 = _fnv(keys, seed)
    h2 = _fnv(keys, seed ^ _GOLDEN) | _U(1)
    j = np.arange(K_HASHES, dtype=_U)[None, :]
    return (h1[:, None] + j * h2[:, None]) % _U(n_bits)


def header(n_bits: int, seed: int = SEED) -> bytes:
    return b"DBLM" + struct.pack("<IIIQQ", 1, K_HASHES, 0, n_bits, seed)


def build(keys, n=None) -> bytes:
    """The filter file over the rows of keys, sized for n keys (default: the
    number of rows)."""
    keys = np.asarray(keys, dtype=np.uint8)
    n = keys.shape[0] if n is None else int(n)
    n_bits = n_bits_for(n)
    bitmap = np.zeros((n_bits + 7) // 8, dtype=np.uint8)
    if keys.shape[0]:
        bits = np.unique(bit_positions(keys, n_bits))
        np.bitwise_or.at(bitmap, (bits >> _U(3)).astype(np.int64),
                         (1 << (bits & _U(7))).astype(np.uint8))
    return header(n_bits) + bitmap.tobytes()


def maybe(filter_bytes: bytes, keys) -> np.ndarray:
    """bool per key: all seven bits set, read from the file's own header —
    what a probe of this filter answers."""
    magic, ver, k, _pad, n_bits, seed = struct.unpack_from("<4sIIIQQ",
                                                           filter_bytes)
    assert magic == b"DBLM" and ver == 1 and k == K_HASHES
    bitmap = np.frombuffer(filter_bytes, dtype=np.uint8, offset=HEADER_LEN)
    bits = bit_positions(keys, n_bits, seed)
    got = (bitmap[(bits >> _U(3)).astype(np.int64)]
           >> (bits & _U(7)).astype(np.uint8)) & 1
    return got.all(axis=1)
