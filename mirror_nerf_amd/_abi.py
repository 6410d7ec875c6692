"""Reader of include/mnrf.h: the header is the one place where the C ABI of libmnrf_hip.so is written down.

    constants, structs, signatures = parse_header(open("include/mnrf.h").read(), pointees=None)

constants   {"MNRF_SPLIT_F16": 4, ...}: every `#define MNRF_NAME <integer literal>`;
structs     {"MnrfBank": <ctypes.Structure subclass>, ...}: field names and order as in the header, a pointer field is c_void_p;
signatures  {"mnrf_embed": (restype, [argtypes]), ...} by one rule: a scalar is its ctypes scalar; `T* const*` is
            POINTER(c_void_p) (a host array of device pointers); a single-level pointer marked MNRF_HOST is POINTER(T) (host
            memory the call reads or writes); every other pointer -- device memory, `void* stream`, a struct -- is c_void_p.
pointees    a dict the caller hands in, filled in the same pass: {"mnrf_embed": [("float", "float"), None, None, None,
            ("float", "float"), ("void", "void")], ...}: per argument position (element class, declared base type) of a
            single-level device pointer -- the class from POINTEE_CLASS, "struct" for an argument block -- and None for every
            other argument.
Anything the reader does not recognise raises ValueError naming the declaration: it never guesses and never skips."""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float,
           "double": ctypes.c_double, "char": ctypes.c_char, "unsigned char": ctypes.c_ubyte,
           "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
# Element class of a single-level device pointer by its declared base type: which tensor dtypes may stand behind it is
# _lib.CLASS_DTYPES.  "void" takes anything (a stream, a typeless workspace), "struct" is an argument block passed by reference.
POINTEE_CLASS = {"float": "float", "double": "double", "int32_t": "int32", "uint32_t": "int32", "int": "int32",
                 "unsigned": "int32", "unsigned int": "int32", "int64_t": "int64", "uint64_t": "int64",
                 "uint8_t": "byte", "int8_t": "byte", "unsigned char": "byte", "void": "void"}
_INTEGER = re.compile(r"\(?\s*(-?\s*(?:0[xX][0-9a-fA-F]+|\d+))[uU]?\s*\)?")


def _declarator(text, known, what):
    """`[MNRF_HOST] [const] T [* [const] [*]] rest` -> (host, T, pointer depth, rest as tokens)."""
    t = [x for x in re.findall(r"\w+|[^\w\s]", text) if x != "const"]
    host = t[:1] == ["MNRF_HOST"]
    t = t[host:]
    base = t.pop(0) if t else ""
    if base == "unsigned" and t[:1] in (["int"], ["char"]):
        base += " " + t.pop(0)
    if base not in known:
        raise ValueError(f"mnrf.h: unknown type {base!r} in {what!r}")
    depth = 0
    while t[:1] == ["*"]:
        depth += 1
        t.pop(0)
    return host, base, depth, t


def _ctype(host, base, depth, what):
    if depth == 0 and base in SCALARS and not host:
        return SCALARS[base]
    if depth == 1 and host and base in SCALARS:
        return ctypes.POINTER(SCALARS[base])
    if depth == 1 and not host:
        return ctypes.c_void_p
    if depth == 2 and not host:
        return ctypes.POINTER(ctypes.c_void_p)
    raise ValueError(f"mnrf.h: no rule for the type of {what!r}")


def _pointee(host, base, depth, structs, what):
    """(element class, declared base type) of a single-level device pointer, None for anything else."""
    if depth != 1 or host:
        return None
    if base in structs:
        return "struct", base
    if base not in POINTEE_CLASS:
        raise ValueError(f"mnrf.h: no element class for the pointer {what!r}")
    return POINTEE_CLASS[base], base


def _struct(name, body):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        _, base, depth, rest = _declarator(decl, set(SCALARS) | {"void"}, f"{name}: {decl}")
        ctype = _ctype(False, base, depth, f"{name}: {decl}")
        m = re.fullmatch(r"(\w+) \[ (\d+) \]|\w+(?: , \w+)*", " ".join(rest))
        if m is None or (depth and m.group(1) is None and len(rest) > 1):      # (`T* a, b` would make b a scalar)
            raise ValueError(f"mnrf.h: cannot read the field {decl!r} of {name}")
        fields += [(m.group(1), ctype * int(m.group(2)))] if m.group(1) else [(n, ctype) for n in rest[::2]]
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/mnrf.h."})


def parse_header(text, pointees=None):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b", " ", text, flags=re.S | re.M)    # extern "C" { / }
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MNRF_\w+)[ \t]*(.*)$", text, flags=re.M):
        m = _INTEGER.fullmatch(value.strip())
        if m:
            constants[name] = int(m.group(1).replace(" ", ""), 0)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    structs = {}

    def take(m):
        if m.group(2) in structs:
            raise ValueError(f"mnrf.h: {m.group(2)} is defined twice")
        structs[m.group(2)] = _struct(m.group(2), m.group(1))
        return " "
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", take, text)

    known, signatures = set(SCALARS) | {"void"} | set(structs), {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(mnrf_\w+)\s*\((.*)\)", decl, flags=re.S)
        if m is None:
            raise ValueError(f"mnrf.h: neither a prototype nor a struct: {' '.join(decl.split())[:120]!r}")
        ret, name, params = m.groups()
        if name in signatures:
            raise ValueError(f"mnrf.h: {name} is declared twice")
        host, base, depth, rest = _declarator(ret, known, f"{name}: {ret}")
        if rest:
            raise ValueError(f"mnrf.h: cannot read the return type of {name}")
        restype = ctypes.c_char_p if (base, depth) == ("char", 1) else _ctype(host, base, depth, f"{name}: {ret}")
        argtypes, classes = [], []
        for p in ([] if params.strip() == "void" else params.split(",")):
            what = f"{name}({' '.join(p.split())})"
            host, base, depth, rest = _declarator(p, known, what)
            if len(rest) != 1 or not re.fullmatch(r"[A-Za-z_]\w*", rest[0]):
                raise ValueError(f"mnrf.h: a parameter needs exactly one name: {what}")
            argtypes.append(_ctype(host, base, depth, what))
            classes.append(_pointee(host, base, depth, structs, what))
        signatures[name] = (restype, argtypes)
        if pointees is not None:
            pointees[name] = classes
    return constants, structs, signatures
