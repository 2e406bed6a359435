"""CPU: the bindings are the header's.  _lib.py derives every ctypes signature, every constant and the tower struct from
include/mmr.h (_header.py); these tests hold the bound library to the header, pin a few signatures and all constants by
hand against today's header so that a reader that drops or merges a type fails, exercise the reader on short header strings,
and show that the comparison catches a changed parameter type.  Nothing here launches a kernel."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint, c_uint64, c_void_p

import pytest

from mmr_amd import _header

VP = c_void_p


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


@pytest.fixture(scope="module")
def header_text():
    with open(_header.PATH) as f:
        return f.read()


def mismatches(L, header):
    """The declared functions whose bound (restype, argtypes) are not the header's."""
    return [name for name, (restype, argtypes, _) in header.functions.items()
            if getattr(L, name).restype != restype or getattr(L, name).argtypes != argtypes]


# ------------------------------------------------------------------ every bound signature is the header's

def test_every_bound_signature_is_the_headers(lib):
    L, H = lib.lib(), _header.load()
    assert len(H.functions) >= 70
    missing = [n for n in H.functions if not hasattr(L, n)]
    assert not missing, missing
    for name, (restype, argtypes, names) in H.functions.items():
        f = getattr(L, name)
        assert f.restype == restype, name
        assert f.argtypes == argtypes, name
        assert len(names) == len(argtypes) and all(names), name
    assert mismatches(L, H) == []


def test_signature_pins(lib):
    L = lib.lib()
    want = [VP] * 22
    for i in (3, 4, 6):
        want[i] = c_int
    for i in (5, 12, 13):
        want[i] = c_int64
    want[7], want[8], want[9], want[20] = c_double, c_float, c_float, c_size_t
    assert L.mmr_cosine_range.argtypes == want and L.mmr_cosine_range.restype is c_int

    a = L.mmr_cosine_topk_deep_qmasked.argtypes
    assert len(a) == 25 and [i for i, t in enumerate(a) if t is c_int64] == [7, 14, 16, 17]
    assert len(L.mmr_threshold_sweep_qmasked.argtypes) == 24
    a = L.mmr_hash_cross_join.argtypes
    assert a[1] is c_int64 and a[3] is c_int64 and a[0] is VP and a[2] is VP
    assert L.mmr_prof_read.argtypes == [c_int, VP, VP, VP]
    assert L.mmr_last_error.restype is c_char_p and L.mmr_last_error.argtypes == []
    assert L.mmr_comm_destroy.restype is None and L.mmr_tower_destroy.restype is None
    sizes = [n for n in _header.load().functions if n.endswith("_workspace_bytes")]
    assert len(sizes) >= 11
    for n in sizes:
        assert getattr(L, n).restype is c_size_t, n


# ------------------------------------------------------------------ the reader, on short header strings

def test_reader_skips_comments_that_look_like_code():
    H = _header.parse("/* mmr_fake(int x); a, b (c) */\nint mmr_real(int x);  // mmr_other(int y);\n/* int mmr_more(void); */")
    assert H.functions == {"mmr_real": (c_int, [c_int], ["x"])}


def test_reader_reads_a_declaration_over_three_lines():
    H = _header.parse("size_t mmr_f(int64_t N,\n             const float *a, double t,\n             size_t bytes);\n")
    assert H.functions == {"mmr_f": (c_size_t, [c_int64, VP, c_double, c_size_t], ["N", "a", "t", "bytes"])}


def test_reader_reads_void_lists_and_return_types():
    H = _header.parse("int mmr_a(void);\nconst char *mmr_b(void);\nvoid mmr_c(void *p);\nconst char * mmr_d();")
    assert H.functions == {"mmr_a": (c_int, [], []), "mmr_b": (c_char_p, [], []), "mmr_c": (None, [VP], ["p"]),
                           "mmr_d": (c_char_p, [], [])}


def test_reader_reads_every_pointer_spelling_and_const_position():
    H = _header.parse("int mmr_p(int *out, int * out2, mmr_comm **out3, const float *a, float const *b, const int n, int const m,\n"
                      "          unsigned u, uint32_t v, uint64_t w, long long x, float y, mmr_dtype d, int32_t e);")
    restype, argtypes, names = H.functions["mmr_p"]
    assert restype is c_int
    assert argtypes == [VP, VP, VP, VP, VP, c_int, c_int, c_uint, c_uint, c_uint64, c_int64, c_float, c_int, c_int]
    assert names == ["out", "out2", "out3", "a", "b", "n", "m", "u", "v", "w", "x", "y", "d", "e"]


def test_reader_reads_enums_defines_and_structs():
    H = _header.parse("#ifndef X_H\n#define X_H\n#include <stddef.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
                      "typedef enum { A_ZERO = 0, A_ONE, /* , B = 9 */ A_TWO, } a_t;\n"
                      "enum {\n  E_OK = 0,\n  E_IO = -5,   /* why (x, y) */\n  E_NEXT,\n  E_HEX = 0x10,\n  E_AFTER\n};\n"
                      "#define LIMIT 4096\n#  define OTHER 7 /* seven */\n#define NOT_AN_INT (1 << 3)\n"
                      "typedef struct thing thing;\n"
                      "typedef struct {\n  int kind;   /* 0, 1; or 2 */\n  float eps;\n  const int32_t *a, *b;\n  int32_t H, W;\n} cfg_t;\n"
                      "int mmr_f(thing *t, const cfg_t *c);\n#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert H.constants == {"A_ZERO": 0, "A_ONE": 1, "A_TWO": 2, "E_OK": 0, "E_IO": -5, "E_NEXT": -4, "E_HEX": 16, "E_AFTER": 17,
                           "LIMIT": 4096, "OTHER": 7}
    assert H.structs == {"cfg_t": [("kind", c_int), ("eps", c_float), ("a", VP), ("b", VP), ("H", c_int), ("W", c_int)]}
    assert H.functions == {"mmr_f": (c_int, [VP, VP], ["t", "c"])}


@pytest.mark.parametrize("text, quoted", [
    ("int mmr_f(short x);", "short x"),                              # a type the table does not hold
    ("int mmr_f(unsigned int x);", "unsigned int x"),
    ("short mmr_f(int x);", "short mmr_f"),                          # ... as a return type
    ("float *mmr_f(int x);", "mmr_f"),                               # a pointer return other than const char *
    ("int mmr_f(void (*cb)(int), int x);", "mmr_f"),                 # a function pointer
    ("int mmr_f(int x[4]);", "x[4]"),                                # an array
    ("int mmr_f(int x, ...);", "..."),                               # an ellipsis
    ("int mmr_f(int x);\nint mmr_g(void);\nint mmr_f(int x);", "mmr_f"),   # a symbol declared twice
    ("enum { A = 1, A = 2 };", "A"),
    ("enum { A = 1 << 2 };", "1 << 2"),
    ("typedef struct { short s; } t;", "short s"),
    ("typedef int (*mmr_cb)(int);", "mmr_cb"),                       # anything that is not one of the known forms
    ("static inline int mmr_f(int x) { return x; }", "mmr_f"),
])
def test_reader_refuses_what_it_cannot_read(text, quoted):
    with pytest.raises(ImportError) as e:
        _header.parse(text)
    assert quoted in str(e.value)


def test_a_missing_header_is_an_import_error(tmp_path):
    with pytest.raises(ImportError) as e:
        _header.load(str(tmp_path / "absent.h"))
    assert "absent.h" in str(e.value)


# ------------------------------------------------------------------ failing controls: a changed type is reported

def _edit_declaration(text, func, old, new):
    at = text.index("int %s(" % func)
    end = text.index(";", at)
    assert text.count(old, at, end) == 1, (func, old)
    return text[:at] + text[at:end].replace(old, new) + text[end:]


@pytest.mark.parametrize("func, old, new", [
    ("mmr_cosine_range", "int64_t N", "int N"),
    ("mmr_cosine_range", "double threshold", "float threshold"),
    ("mmr_hash_cross_join", "int64_t M", "int M"),
    ("mmr_cosine_assign", "int64_t amb_cap, int32_t *labels", "int32_t *labels, int64_t amb_cap"),
])
def test_a_changed_parameter_type_is_reported_for_exactly_that_function(lib, header_text, func, old, new):
    changed = _header.parse(_edit_declaration(header_text, func, old, new))
    assert mismatches(lib.lib(), changed) == [func]


# ------------------------------------------------------------------ constants, against today's literals

def test_constant_pins(lib):
    assert (lib.P_PATCH_W, lib.P_QKV_W, lib.P_FC1_C, lib.P_COUNT) == (0, 7, 26, 27)
    assert len([n for n in dir(lib) if n.startswith("P_")]) == 28
    assert lib._ERRNAMES == {-5: "EIO", -22: "EINVAL", -28: "ENOSPC", -95: "ENOTSUP"}
    assert (lib.MMR_F32, lib.MMR_BF16, lib.MMR_F16) == (0, 1, 2)
    assert list(lib.PROF_CLASSES.items()) == [("gemm", 0), ("attention", 1), ("rowwise", 2), ("scan", 3), ("finalize", 4),
                                              ("exact", 5)]
    ints = ("kind", "width", "layers", "heads", "mlp", "tokens", "embed_dim", "image_size", "patch", "vocab")
    assert lib.TowerCfg._fields_ == [(n, c_int) for n in ints] + [("ln_eps", c_float), ("fold_ln", c_int)]
    assert ctypes.sizeof(lib.TowerCfg) == 48
    from mmr_amd import search
    assert search.DEEP_K_MAX == 4096 and search.SWEEP_T_MAX == 1024
    C = _header.load().constants
    assert C["MMR_OK"] == 0 and C["MMR_COMM_ID_BYTES"] == 128 and C["MMR_STATUS_BAD_TOKEN_ID"] == 1 and C["MMR_PROF_CLASSES"] == 6


def test_the_six_pointer_arguments_take_what_their_call_sites_pass():
    """mmr_prof_read, mmr_comm_init and the tower calls were bound with typed pointers; c_void_p takes the same arguments."""
    x, h = ctypes.c_double(), c_void_p()
    for arg in (ctypes.byref(x), ctypes.pointer(x), ctypes.byref(h), 0, 256, None, (ctypes.c_double * 2)(0.1, 0.2)):
        c_void_p.from_param(arg)
