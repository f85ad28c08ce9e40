"""Reader of include/vppx.h: its prototypes, structs and integer constants as ctypes.  The header is regular C (no function
pointers, arrays or nested parentheses); whatever does not fit the few rules below raises with the declaration's text."""
import ctypes as C
import re
from functools import reduce
from operator import or_
from types import SimpleNamespace

SCALARS = {
    "int": C.c_int, "long": C.c_long, "unsigned": C.c_uint, "unsigned int": C.c_uint, "float": C.c_float, "double": C.c_double,
    "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
}


def _struct_pointer(struct):
    """POINTER(struct) as an argument type that, besides the instance, byref(), arrays and pointers, takes what c_void_p takes
    of addresses -- an int or a c_void_p -- because a `VppxMetrics *` may point into device memory, where no instance lives."""
    base = C.POINTER(struct)

    def from_param(cls, v):
        if isinstance(v, (int, C.c_void_p)):
            v = C.cast(C.c_void_p(v) if isinstance(v, int) else v, base)
        return base.from_param(v)
    return type(base.__name__, (base,), {"from_param": classmethod(from_param)})


def _ctype(text, pointers, decl):
    """Scalars by name, char * as c_char_p, a pointer to one of the header's structs typed, every other pointer c_void_p."""
    base = " ".join(w for w in text.replace("*", " ").split() if w != "const")
    stars = text.count("*")
    if stars == 0 and base in SCALARS:
        return SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in pointers:
        return pointers[base]
    if stars and re.fullmatch(r"\w+", base):
        return C.c_void_p
    raise ValueError(f"include/vppx.h: no ctypes type for {text.strip()!r} in: {decl}")


def _names(item, decl):
    """`int32_t C, Hs, Ws` -> ("int32_t ", ["C", "Hs", "Ws"]); `const void *ptr` -> ("const void *", ["ptr"])."""
    first, *more = (d.strip() for d in item.split(","))
    m = re.fullmatch(r"(.*[\s*])(\w+)", first)
    if not m or not all(re.fullmatch(r"\w+", d) for d in more):
        raise ValueError(f"include/vppx.h: cannot split {item.strip()!r} into type and name in: {decl}")
    return m.group(1), [m.group(2), *more]


def parse(text):
    """The header's text -> .protos {name: (restype, [argtypes])} in header order, .structs {name: ctypes.Structure},
    .constants {name: int}: every enumerator and every `#define NAME <integer>`."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)

    def enum(m):
        value = -1
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            name, _, expr = (p.strip() for p in item.partition("="))
            try:            # implicit, a literal, or earlier enumerators and literals joined with |
                value = reduce(or_, (constants[t] if t in constants else int(t, 0) for t in re.split(r"\s*\|\s*", expr))) if expr else value + 1
            except ValueError:
                raise ValueError(f"include/vppx.h: no integer value for the enumerator: {item}") from None
            constants[name] = value
        return " "
    text = re.sub(r"(?:typedef\s+)?enum\s*\w*\s*\{([^{}]*)\}\s*\w*\s*;", enum, text)

    structs, pointers = {}, {}

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            ctype, names = _names(decl, decl)
            fields += [(n, _ctype(ctype, pointers, decl)) for n in names]
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        pointers[m.group(1)] = _struct_pointer(structs[m.group(1)])
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)

    # every statement left that has a parenthesis is a prototype of ours, or an error: nothing else may name a vppx_ function
    protos = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"(.*[\s*])(vppx_\w+) ?\(([^()]*)\)", stmt)
        if not m:
            raise ValueError(f"include/vppx.h: cannot split the prototype: {stmt}")
        params = [] if m.group(3).strip() == "void" else [_names(p, stmt)[0] for p in m.group(3).split(",")]
        restype = None if m.group(1).strip() == "void" else _ctype(m.group(1), pointers, stmt)
        protos[m.group(2)] = (restype, [_ctype(p, pointers, stmt) for p in params])
    return SimpleNamespace(protos=protos, structs=structs, constants=constants)
