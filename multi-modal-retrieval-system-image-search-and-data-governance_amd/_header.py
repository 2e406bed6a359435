"""Reads include/mmr.h: the ctypes signatures, the integer constants and the struct layouts of the C ABI.

The header is the one statement of the boundary; _lib.py binds what this module reads.  The reader knows the subset of C
the header uses and is strict about it: a declaration it cannot read is an ImportError that quotes it, never a skipped
function and never ctypes' int default.
"""
import collections
import ctypes
import os
import re

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mmr.h")

# every type the ABI passes by value; a parameter or field with a `*` is a c_void_p whatever it points to
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "mmr_dtype": ctypes.c_int,
            "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint,
            "int64_t": ctypes.c_int64, "long long": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": ctypes.c_char_p})

Header = collections.namedtuple("Header", "functions constants structs")
# functions: name -> (restype, [argtypes], [parameter names]); constants: enumerator or #define -> int;
# structs: typedef name -> [(field, ctype)], ready for ctypes.Structure._fields_


def _declarator(text, decl):
    """'const float *x' -> ('x', c_void_p); 'int64_t N' -> ('N', c_int64); 'int' -> ('', c_int)."""
    if re.search(r"[()\[\]]|\.\.\.", text):
        raise ImportError(f"mmr.h: function-pointer, array or variadic parameter `{text.strip()}` in `{decl}`")
    words = [w for w in re.findall(r"\w+", text) if w != "const"]
    if "*" in text:
        return (words[-1] if len(words) > 1 else ""), ctypes.c_void_p
    for ctype, name in ((" ".join(words), ""), (" ".join(words[:-1]), words[-1] if words else "")):
        if ctype in _SCALARS:
            return name, _SCALARS[ctype]
    raise ImportError(f"mmr.h: no ctypes mapping for `{text.strip()}` in `{decl}`")


def _fields(body, decl):
    """The members of a struct body; `int32_t H, W;` and `const int32_t *a, *b;` declare one field per name."""
    out = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        first, *more = member.split(",")
        name, ctype = _declarator(first, decl)
        out.append((name, ctype))
        out += [(m.replace("*", " ").strip(), ctypes.c_void_p if "*" in m else ctype) for m in more]
    return out


def parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants, structs, functions = {}, {}, {}

    def constant(name, value, decl):
        if name in constants:
            raise ImportError(f"mmr.h: `{name}` defined twice (`{decl}`)")
        constants[name] = value

    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+([-+]?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M):
        constant(name, int(value, 0), "#define " + name)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)

    def enum(m):
        decl, value = " ".join(m.group(0).split()), -1
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            im = re.fullmatch(r"(\w+)(?:\s*=\s*([-+]?(?:0[xX][0-9a-fA-F]+|\d+)))?", item)
            if not im:
                raise ImportError(f"mmr.h: cannot read enumerator `{item}` in `{decl}`")
            value = int(im.group(2), 0) if im.group(2) else value + 1
            constant(im.group(1), value, decl)
        return " "

    def struct(m):
        decl = " ".join(m.group(0).split())
        if m.group(2) in structs:
            raise ImportError(f"mmr.h: struct `{m.group(2)}` declared twice")
        structs[m.group(2)] = _fields(m.group(1), decl)
        return " "

    text = re.sub(r"\b(?:typedef\s+)?enum\s*\{([^{}]*)\}\s*\w*\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", " ", text)        # opaque handles
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.*?)\s*\b(\w+)\s*\((.*)\)", decl)
        ret = m and re.sub(r"\s*\*\s*", " *", m.group(1))
        if not m or ret not in _RETURNS:
            raise ImportError(f"mmr.h: cannot read the declaration `{decl}`")
        if m.group(2) in functions:
            raise ImportError(f"mmr.h: `{m.group(2)}` declared twice (`{decl}`)")
        params = [] if m.group(3).strip() in ("", "void") else [_declarator(p, decl) for p in m.group(3).split(",")]
        functions[m.group(2)] = (_RETURNS[ret], [t for _, t in params], [n for n, _ in params])
    return Header(functions, constants, structs)


def load(path=PATH):
    try:
        with open(path) as f:
            return parse(f.read())
    except OSError as e:
        raise ImportError(f"{path}: the C ABI's header cannot be read ({e}); the bindings are derived from it") from e
