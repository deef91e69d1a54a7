"""dbeel_amd — MI355X-native SSTable compaction engine for dbeel.

Product scope: the `LSMTree::compact` hot path
(reference lsm_tree.rs:950-1156), rebuilt from scratch as HIP/CDNA4 kernels
behind a C ABI (include/dbeel_gpu.h). Host-side mirrors of the reference's
format and trigger logic live beside it; everything else in dbeel is out of
scope by contract.
"""
from . import format  # noqa: F401
from .engine import (  # noqa: F401
    BatchJob,
    DbeelGpuError,
    Job,
    Reader,
    compact,
    compact_into,
    compact_sliced,
    encode_run,
    flush_batch,
    lookup,
    lookup_raw,
    pin_host,
    scan,
    unpin_host,
)

__all__ = [
    "compact", "compact_sliced", "compact_into", "scan", "lookup", "encode_run",
    "Job", "BatchJob", "pin_host", "unpin_host", "DbeelGpuError", "format",
    "Reader", "lookup_raw", "flush_batch",
]
