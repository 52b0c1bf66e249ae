"""ctypes binding of libkirag_sparse.so (include/kirag_sparse.h): exact top-k over a blocked inverted index and the compaction of SPLADE rows.

Built in-tree by ``kirag_amd/csrc/Makefile`` next to libkirag_amd.so and libkirag_late.so, which it neither links nor replaces.  As in ``_lib``: no fallback — a
missing shared object or a failed call raises.  ctypes releases the GIL around every call (``CDLL``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KIRAG_SPARSE_LIB") or os.path.join(_HERE, "libkirag_sparse.so")   # KIRAG_SPARSE_LIB: another build of the library (A/B, the other R)
ABI_VERSION = 1
OK, EINVAL, ENOMEM, ENODEV, EHIP, ERANGE = 0, -22, -12, -19, -5, -34
MAX_K, MAX_QUERIES, MAX_SKIP, MAX_CANDIDATES = 1024, 65535, 64, 1 << 24
BOUND_ENV = "KIRAG_SPARSE_MAX_CANDIDATES"


class KiragSparseError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libkirag_sparse error {code}: {msg}")
        self.code = code


# name -> (restype, argtypes); every symbol include/kirag_sparse.h declares
SIGNATURES = {
    "ks_abi_version": (C.c_int, []),
    "ks_last_error": (C.c_char_p, []),
    "ks_release_scratch": (None, []),
    "ks_block_rows": (C.c_int, []),
    "ks_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_int, C.c_void_p]),
    "ks_count_positive": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ks_compact_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared object (once).  Raises if it is missing — the HIP path is the only path."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (torch's HIP runtime first, as in _lib.load)
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make -C kirag_amd/csrc` (or __graft_entry__.build()). kirag_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the build does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.ks_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"libkirag_sparse ABI {v} != expected {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def block_rows() -> int:
    """R of the loaded build (``KS_BLOCK_ROWS``): the rows of an index block"""
    return int(load().ks_block_rows())


def set_candidate_bound(n: Optional[int]) -> None:
    """Lower the bound of ``ks_search``'s candidate workspace (``KS_MAX_CANDIDATES``) for the calls that follow, ``None`` puts the library's own back.  The
    library reads the environment variable at every call; this is how a test makes the query slicing happen at a small size."""
    if n is None:
        os.environ.pop(BOUND_ENV, None)
    else:
        os.environ[BOUND_ENV] = str(int(n))


def check(rc: int) -> None:
    if rc != 0:
        msg = load().ks_last_error()
        raise KiragSparseError(rc, msg.decode("utf-8", "replace") if msg else "")
