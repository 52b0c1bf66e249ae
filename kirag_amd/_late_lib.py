"""ctypes binding of libkirag_late.so (include/kirag_late.h): token-vector gather / conversion and MaxSim.

Built in-tree by ``kirag_amd/csrc/Makefile`` next to libkirag_amd.so, which it neither links nor replaces.  As in ``_lib``: no fallback — a missing shared
object or a failed call raises.  ctypes releases the GIL around every call (``CDLL``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KIRAG_LATE_LIB") or os.path.join(_HERE, "libkirag_late.so")   # KIRAG_LATE_LIB: another build of the library (A/B)
ABI_VERSION = 1
OK, EINVAL, ENOMEM, ENODEV, EHIP, ERANGE = 0, -22, -12, -19, -5, -34
REDUCE = {"sum": 0, "mean": 1}
MIN_DIM, MAX_DIM = 32, 2048


class KiragLateError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libkirag_late error {code}: {msg}")
        self.code = code


# name -> (restype, argtypes); every symbol include/kirag_late.h declares
SIGNATURES = {
    "kl_abi_version": (C.c_int, []),
    "kl_last_error": (C.c_char_p, []),
    "kl_release_scratch": (None, []),
    "kl_gather_rows_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "kl_maxsim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                            C.c_void_p, C.c_int, C.c_void_p]),
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
    v = lib.kl_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"libkirag_late ABI {v} != expected {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().kl_last_error()
        raise KiragLateError(rc, msg.decode("utf-8", "replace") if msg else "")
