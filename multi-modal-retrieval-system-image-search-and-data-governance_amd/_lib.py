"""ctypes binding of csrc/libmmr_hip.so (the C ABI in include/mmr.h).

Signatures, constants and the tower struct are read from the header (_header.py), so a new or changed entry point needs no
edit here.  There is deliberately no fallback: if the HIP library is missing or a call fails, the caller gets an
exception -- never a silent CPU/torch path.
"""
import ctypes
import os

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMR_LIB") or os.path.join(_HERE, "csrc", "libmmr_hip.so")   # MMR_LIB: A/B builds

HEADER = _header.load()
_C = HEADER.constants
MMR_F32, MMR_BF16, MMR_F16 = _C["MMR_F32"], _C["MMR_BF16"], _C["MMR_F16"]
_ERRNAMES = {v: n[len("MMR_"):] for n, v in _C.items() if n.startswith("MMR_E")}
globals().update({n[len("MMR_"):]: v for n, v in _C.items() if n.startswith("MMR_P_")})   # mmr_param: P_PATCH_W .. P_COUNT
PROF_CLASSES = {n[len("MMR_PROF_"):].lower(): v for n, v in _C.items() if n.startswith("MMR_PROF_") and n != "MMR_PROF_CLASSES"}


class MMRError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmmr_hip: {_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class TowerCfg(ctypes.Structure):
    _fields_ = HEADER.structs["mmr_tower_cfg"]


def struct_dtype(name: str):
    """numpy view of a struct of mmr.h (descriptor arrays are built as numpy records), field for field from the header"""
    import numpy as np

    S = type(name, (ctypes.Structure,), {"_fields_": HEADER.structs[name]})
    np_of = {ctypes.c_void_p: np.uint64, ctypes.c_int: np.int32, ctypes.c_int64: np.int64}
    names = [n for n, _ in S._fields_]
    return np.dtype({"names": names, "formats": [np_of[t] for _, t in S._fields_],
                     "offsets": [getattr(S, n).offset for n in names], "itemsize": ctypes.sizeof(S)})


_lib = None


def lib():
    """Load the HIP library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes, _) in HEADER.functions.items():
        f = getattr(L, name, None)          # absent from an older A/B library (MMR_LIB): left unbound, its callers raise
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise MMRError(rc, lib().mmr_last_error().decode())


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return MMR_F32
    if dt == torch.bfloat16:
        return MMR_BF16
    if dt == torch.float16:
        return MMR_F16
    raise TypeError(f"libmmr_hip handles float32, bfloat16 and float16 tensors, got {dt}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def prof_enable(on: bool, max_launches: int = 65536):
    check(lib().mmr_prof_enable(int(on), int(max_launches)))


def prof_read():
    """-> {class: (total_ms, launches)} for the launches recorded since prof_enable(True)."""
    out = {}
    for name, cls in PROF_CLASSES.items():
        ms, n, dr = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_longlong()
        check(lib().mmr_prof_read(cls, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(dr)))
        out[name] = (ms.value, n.value)
    out["dropped"] = dr.value
    return out
