"""Every LIPASR_* environment variable of the project, one row each (README.md shows the same table).

``get(name)`` reads ``os.environ`` when it is called, never at import: a variable set just before a model or a pipeline is
built counts.  Rows whose reader is not "lipasr" are listed for the record only: the native library, bench.py and
__graft_entry__.py read theirs themselves.
"""
import os
from typing import NamedTuple


class Knob(NamedTuple):
    name: str
    default: object  # what get() returns when the variable is unset (None: no value; the reader then applies its own rule)
    parse: object    # int: get() returns int(value); "0/1", "path", a tuple of words: the string itself (float, "set": other readers')
    kind: str        # "product", or "probe": A/B timing, same results
    meaning: str
    reader: str = "lipasr"


TABLE = (
    Knob("LIPASR_LIBRARY", None, "path", "probe", "another build of liblipasr.so to load (never a different backend)"),
    Knob("LIPASR_HDF5_LIBRARY", None, "path", "product", "the libhdf5 to load before the loader's search path is tried"),
    Knob("LIPASR_COMPUTE", "float32", ("float32", "float16x2", "bfloat16"), "product",
         "arithmetic of the training GEMMs of a Model built without compute_dtype (bench.py reads it too, with float16x2 as its default)"),
    Knob("LIPASR_FUSE_BN", "1", "0/1", "probe", "0: BatchNorm as launches of its own instead of inside the producing GEMM"),
    Knob("LIPASR_GEMM_TILES", None, int, "probe",
         "64 x 64 tiles from which a GEMM takes the LDS-tiled / ring kernels (library: 224; a pipeline on a CU share: 128)"),
    Knob("LIPASR_CHAIN_HEAD", None, int, "probe", "leading steps of the product chain run as one launch (lipasr_debug_chain_head)"),
    Knob("LIPASR_GEMM_MODE", None, int, "probe", "bit set of GEMM kernel choices (lipasr_debug_gemm_mode)"),
    Knob("LIPASR_MFCC_CUS", None, int, "probe", "CUs of the extraction stream when mfcc_cus=\"auto\" (unset: the measured share)"),
    Knob("LIPASR_TRAIN_CUS", None, ("rest", "all"), "probe",
         "classifier stream when train_cus=\"auto\" (unset: rest with the built-in MFCC plan, all for PGD or a custom extractor)"),
    Knob("LIPASR_TRAIN_OWN_QUEUE", "1", "0/1", "probe", "0: a classifier that keeps every CU stays on a pool stream"),
    Knob("LIPASR_WIDE_WHEN_IDLE", "1", "0/1", "probe", "0: the extraction keeps to its CU share also while the classifier is idle"),
    Knob("LIPASR_GPU_FLAGS", "auto", ("auto", "0", "1"), "product",
         "hand-offs between the two streams: 1 device flags, 0 events (needed under tools that serialise kernels), auto: flags on one device"),
    Knob("LIPASR_FLAG_TIMEOUT_MS", 30000, int, "product", "what a device-side wait sits out before it reports"),
    Knob("LIPASR_ADAM_SIGNAL", "1", "0/1", "probe", "0: \"buffer free\" as a trailing launch instead of from the Adam kernel"),
    Knob("LIPASR_XC_NOWAIT", None, "set", "probe", "exchange epilogue without its wait (results are wrong; -DLIPASR_PROBES builds only)", "native"),
    Knob("LIPASR_CPU_WORKERS", 16, int, "product", "processes of the CPU baseline", "bench"),
    Knob("LIPASR_SCALER_BATCHES", 1000000, int, "probe", "batches the StandardScaler is fitted on", "bench"),
    Knob("LIPASR_PRE_PARTITION", None, int, "probe", "mfcc_cus of the pre-extracted configurations (unset: no partition)", "bench"),
    Knob("LIPASR_DP_OVERLAP", "0", "0/1", "probe", "1: two gradient buckets around dW_0 (overlap_buckets)", "bench"),
    Knob("LIPASR_MFCC_FUSED", "0", "0/1", "probe", "1: the fused resample -> STFT kernel for every batch", "bench"),
    Knob("LIPASR_MFCC_MASK", None, int, "probe", "stage mask of the extraction plan (64: the round-2 STFT kernel)", "bench"),
    Knob("LIPASR_BENCH_PREWARM_MS", 0, float, "probe", "busy GEMMs for this long before the warm-up steps", "bench"),
    Knob("LIPASR_FORCE_BUILD", "", "0/1", "product", "1: build() recompiles everything", "entry"),
)
_ROWS = {k.name: k for k in TABLE}


def get(name):
    """The variable's value now: the row's default when unset (or empty, for a row without one), int() of it for an int row (a
    value that is no integer raises ValueError), else the string as it stands.  KeyError for a name the table does not have."""
    row = _ROWS[name]
    v = os.environ.get(name)
    if v is None or (v == "" and row.default is None):
        return row.default
    return int(v) if row.parse is int else v
