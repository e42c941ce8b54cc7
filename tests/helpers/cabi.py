"""The header contract, once: a public header of include/ <=> the loaded library <=> oi_amd.lib's binding table and struct
mirrors.  check_header(header, lib) parses the header (comments stripped) and asserts

  1. the prototypes' names are lib.symbols(header), and the loaded library exports each;
  2. no name stands under two headers of lib.SIGS;
  3. every prototype agrees with its binding in result, argument count and, argument by argument, in kind;
  4. every `typedef struct oi_x_y { ... }` that lib mirrors (as class XY) has the mirror's field names in order, and the
     fields agree in kind; arrays agree in element type and extents;
  5. a type this file does not know fails, it is never skipped.

Kinds: a pointer (oi_stream_t is one) binds as c_void_p, as POINTER of the scalar it points to, or -- and then only so --
as POINTER of the mirror when it points to a mirrored struct; the scalars bind as SCALARS says."""
import ctypes
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include")

SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong}
_TYPE = r"((?:(?:unsigned|signed|long|short|char|int)\b\s*)+|\w+)"


def built_lib():
    """(oi_amd.lib, the loaded handle) of the built library."""
    import __graft_entry__ as ge
    ge.build()
    from oi_amd import lib
    return lib, lib.load()


def read(header):
    with open(os.path.join(INCLUDE, header)) as fh:
        return fh.read()


def _declarators(text, defines):
    """`const float *a, b[N][16]` -> [(name, (base type, pointer depth, extents))]."""
    base, rest = re.fullmatch(_TYPE + r"\s*(.*)", re.sub(r"\b(const|struct)\b", " ", text).strip(), re.S).groups()
    base, out = " ".join(base.split()), []
    for d in rest.split(","):
        m = re.fullmatch(r"([\s*]*)(\w*)\s*((?:\[\s*\w+\s*\]\s*)*)", d.strip())
        assert m, f"cannot parse the declaration {text!r}"
        extents = tuple(int(defines.get(e, e)) for e in re.findall(r"\[\s*(\w+)\s*\]", m.group(3)))
        out.append((m.group(2), ("void", 1, extents) if base == "oi_stream_t" else (base, m.group(1).count("*"), extents)))
    return out


def parse(text):
    """-> (prototypes {name: (result kind, [argument kinds])} in the header's order, structs {name: [(field, kind)]})."""
    defines = {k: v for k, v in re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)\b", text, re.M)}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\}\s*$", " ", text)                       # the brace that closes extern "C"
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        structs[name] = [f for decl in body.split(";") if decl.strip() for f in _declarators(decl, defines)]
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{.*?\}\s*\1\s*;", " ", text, flags=re.S)
    text = re.sub(r"\benum\s+\w+\s*\{.*?\}\s*;", " ", text, flags=re.S)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.*?)\b(oi_\w+)\s*\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"
        ret, name, args = m.groups()
        assert name not in protos, f"{name} is declared twice"
        args = [] if args.strip() in ("", "void") else [_declarators(a, defines)[0][1] for a in args.split(",")]
        # an array parameter is a pointer
        protos[name] = (_declarators(ret + " _", defines)[0][1], [(b, p + len(e), ()) for b, p, e in args])
    return protos, structs


def mirror_of(lib, struct):
    """lib's mirror of `oi_surface_ao_params` is its ctypes.Structure SurfaceAoParams; None when there is none."""
    cls = getattr(lib, "".join(w.capitalize() for w in struct.split("_")[1:]), None) if struct.startswith("oi_") else None
    return cls if isinstance(cls, type) and issubclass(cls, ctypes.Structure) else None


def agrees(kind, ctype, lib):
    """Does the ctypes type bind the declared (base type, pointer depth, extents)?  An unknown type raises."""
    base, ptr, extents = kind
    if extents:
        return (isinstance(ctype, type) and issubclass(ctype, ctypes.Array) and ctype._length_ == extents[0]
                and agrees((base, ptr, extents[1:]), ctype._type_, lib))
    mirror = mirror_of(lib, base)
    assert mirror or base in SCALARS or (ptr and re.fullmatch(r"void|char|unsigned char|u?int(8|16|32|64)_t|oi_\w+", base)), \
        f"unknown type {base!r}"
    if ptr == 0:
        return ctype is (mirror or SCALARS[base])
    if ptr == 1 and mirror:
        return ctype is ctypes.POINTER(mirror)
    if ptr == 1 and base == "char" and ctype is ctypes.c_char_p:
        return True
    return ctype is ctypes.c_void_p or (ptr == 1 and base in SCALARS and ctype is ctypes.POINTER(SCALARS[base]))


def check_header(header, lib, text=None):
    """Asserts the contract of the module docstring for one header (text: the header's text, default the file's).
    -> (the entry names in the header's order, the names of the mirrors checked)."""
    protos, structs = parse(read(header) if text is None else text)
    table = lib.SIGS[header]
    assert sorted(protos) == lib.symbols(header) == sorted(table), sorted(set(protos) ^ set(table))
    L = lib.load()
    for name in protos:
        assert hasattr(L, name), f"{name} declared in include/{header} but not exported"
    seen = {}
    for h, entries in lib.SIGS.items():
        for name in entries:
            assert name not in seen, f"{name} stands under {seen[name]} and {h}"
            seen[name] = h
    for name, (ret, args) in protos.items():
        res, argtypes = table[name]
        assert (res is None) if ret == ("void", 0, ()) else agrees(ret, res, lib), f"{name}: returns {ret}, bound as {res}"
        assert len(args) == len(argtypes), f"{name}: {len(args)} parameters, {len(argtypes)} bound"
        for k, (a, c) in enumerate(zip(args, argtypes)):
            assert agrees(a, c, lib), f"{name}: parameter {k} is {a}, bound as {c}"
    mirrors = []
    for struct, fields in structs.items():
        cls = mirror_of(lib, struct)
        if cls is None:
            continue
        assert [f for f, _ in fields] == [f[0] for f in cls._fields_], f"{struct}: fields {[f for f, _ in fields]}"
        for (f, kind), (_, c) in zip(fields, cls._fields_):
            assert agrees(kind, c, lib), f"{struct}.{f} is {kind}, mirrored as {c}"
        mirrors.append(cls.__name__)
    return list(protos), mirrors
