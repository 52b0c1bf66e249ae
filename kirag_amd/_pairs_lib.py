"""ctypes binding of libkirag_pairs.so (include/kirag_pairs.h): the exact sparse score of given (query, row) pairs over a sparse index's forward form.

Built in-tree by ``kirag_amd/csrc/Makefile`` next to libkirag_amd.so, libkirag_late.so and libkirag_sparse.so, none of which it links or replaces.  As in
``_lib``: no fallback — a missing shared object or a failed call raises.  ctypes releases the GIL around every call (``CDLL``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KIRAG_PAIRS_LIB") or os.path.join(_HERE, "libkirag_pairs.so")   # KIRAG_PAIRS_LIB: another build of the library (A/B)
ABI_VERSION = 1
OK, EINVAL, ENOMEM, ENODEV, EHIP = 0, -22, -12, -19, -5
MAX_QUERIES, MAX_PAIRS, MAX_STAGED_PAIRS = 65535, 1 << 24, 1 << 20
BOUND_ENV = "KIRAG_PAIRS_MAX_STAGED"


class KiragPairsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libkirag_pairs error {code}: {msg}")
        self.code = code


# name -> (restype, argtypes); every symbol include/kirag_pairs.h declares
SIGNATURES = {
    "kp_abi_version": (C.c_int, []),
    "kp_last_error": (C.c_char_p, []),
    "kp_release_scratch": (None, []),
    "kp_sparse_dot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
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
    v = lib.kp_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"libkirag_pairs ABI {v} != expected {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def set_staged_bound(n: Optional[int]) -> None:
    """Lower the number of pair records ``kp_sparse_dot`` stages and launches at once (``KP_MAX_STAGED_PAIRS``) for the calls that follow, ``None`` puts the
    library's own back.  The library reads the environment variable at every call; this is how a test makes the slicing happen at a small size."""
    if n is None:
        os.environ.pop(BOUND_ENV, None)
    else:
        os.environ[BOUND_ENV] = str(int(n))


def check(rc: int) -> None:
    if rc != 0:
        msg = load().kp_last_error()
        raise KiragPairsError(rc, msg.decode("utf-8", "replace") if msg else "")
