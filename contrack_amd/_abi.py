"""The C headers (include/contrack_hip.h, include/contrack_hip_debug.h) as Python data: the one statement of the ABI that the
binding (_native.py) is built from.  Standard library only; no compiler, no generated file.

The subset of C understood is the one the headers use: #define NAME <integer>, opaque `typedef struct X X;`, struct typedefs of
scalars and pointers, function-pointer typedefs and function declarations over the scalar types below, pointers and those
typedefs.  Anything else raises AbiError with the declaration's text: a header that outgrows the subset stops the import, it is
never bound by guesswork."""
import collections
import ctypes as C
import re

HEADERS = ("contrack_hip.h", "contrack_hip_debug.h")          # in this order: the second uses the types of the first

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
_POINTEES = {"void", "char", "uint8_t"}                        # met behind a pointer only

Abi = collections.namedtuple("Abi", "functions callbacks structs constants")

_DECLARATOR = r"((?:\*\s*(?:const\s*)?)*)"                     # the stars of a declarator, each with its const
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*%s(\w+)?" % _DECLARATOR)
_FIELD = re.compile(r"%s(\w+)" % _DECLARATOR)
_FUNCTION = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*\((.*)\)", re.S)
_CALLBACK = re.compile(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\((.*)\)", re.S)


class AbiError(ValueError):
    pass


def parse(text):
    """header text -> Abi(functions: name -> (restype, argtypes), callbacks: typedef name -> CFUNCTYPE, structs: name -> [(field,
    ctype)], constants: CTK_* name -> int)"""
    abi = Abi({}, {}, {}, {})
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    abi.constants.update((k, int(v)) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CTK_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M))
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M)
    opaque = set()
    text = re.sub(r"typedef\s+struct\s+(\w+)\s+\1\s*;", lambda m: opaque.add(m.group(1)) or "", text)

    def ctype(base, stars, where, ret=False):
        if stars:
            if base not in SCALARS and base not in _POINTEES and base not in opaque and base not in abi.structs:
                raise AbiError("%s: unknown type %r" % (where, base))
            return C.c_char_p if (base, stars) == ("char", 1) else C.c_void_p
        if base == "void" and ret:
            return None
        if base in abi.structs:
            raise AbiError("%s: struct %s passed by value" % (where, base))
        if base not in SCALARS and base not in abi.callbacks:
            raise AbiError("%s: unknown type %r" % (where, base))
        return SCALARS.get(base) or abi.callbacks[base]

    def params(args, where):
        if args.strip() == "void":
            return []
        out = []
        for a in args.split(","):
            m = _PARAM.fullmatch(a.strip())
            if not m:                                          # `...`, an array, a type of several words
                raise AbiError("%s: cannot bind parameter %r" % (where, a.strip()))
            out.append(ctype(m.group(1), m.group(2).count("*"), where))
        return out

    def struct(m):
        name, fields = m.group(1), []
        for line in filter(None, (s.strip() for s in m.group(2).split(";"))):
            head = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", line, re.S)
            for d in head.group(2).split(","):
                f = _FIELD.fullmatch(d.strip())
                if not f:
                    raise AbiError("struct %s: cannot bind field %r" % (name, line))
                fields.append((f.group(2), ctype(head.group(1), f.group(1).count("*"), "struct " + name)))
        abi.structs[name] = fields
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    text = re.sub(r"^\s*\}\s*$", "", text, flags=re.M)          # closes extern "C"

    for stmt in (s.strip() for s in text.split(";")):
        if not stmt:
            continue
        m = _CALLBACK.fullmatch(stmt)
        if m:
            where = "typedef " + m.group(2)
            abi.callbacks[m.group(2)] = C.CFUNCTYPE(ctype(m.group(1), 0, where, ret=True), *params(m.group(3), where))
            continue
        m = _FUNCTION.fullmatch(stmt)
        if not m or stmt.startswith("typedef"):
            raise AbiError("cannot parse the declaration %r" % " ".join(stmt.split()))
        abi.functions[m.group(3)] = (ctype(m.group(1), len(m.group(2)), m.group(3), ret=True), params(m.group(4), m.group(3)))
    return abi
