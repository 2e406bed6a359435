"""Print what _lib.py binds, as one JSON document: (restype, argtypes) of every function include/mmr.h declares, with
POINTER(...) normalised to c_void_p and an unset argtypes shown as [], and the module-level constants derived from the
header.  Two trees bind the same ABI iff their outputs are equal:

    MMR_LIB=<built libmmr_hip.so> python tools/dump_bindings.py      # in each tree, then diff
"""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmr_amd import _lib, search  # noqa: E402


def tname(t):
    if t is None:
        return "None"
    return "c_void_p" if isinstance(t, type(ctypes.POINTER(ctypes.c_int))) and t is not ctypes.c_char_p else t.__name__


L = _lib.lib()
hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mmr.h")).read(), flags=re.S)
funcs = {}
for name in sorted(set(re.findall(r"\b(mmr_[a-z0-9_]+)\s*\(", hdr))):
    f = getattr(L, name)
    funcs[name] = [tname(f.restype), [tname(a) for a in (f.argtypes or [])]]
consts = {n: getattr(_lib, n) for n in dir(_lib) if re.fullmatch(r"P_[A-Z0-9_]+|MMR_(F32|BF16|F16)", n)}
consts["_ERRNAMES"] = sorted(_lib._ERRNAMES.items())
consts["PROF_CLASSES"] = list(_lib.PROF_CLASSES.items())
consts["TowerCfg"] = [[n, tname(t)] for n, t in _lib.TowerCfg._fields_] + [ctypes.sizeof(_lib.TowerCfg)]
consts["DEEP_K_MAX"], consts["SWEEP_T_MAX"] = search.DEEP_K_MAX, search.SWEEP_T_MAX
print(json.dumps({"functions": funcs, "constants": consts}, indent=1, sort_keys=True))
