"""Reader of include/recsys_hip.h, the only specification of the C-ABI: its integer #defines, its
typedef'd structs and its function declarations as ctypes types. It reads the header's own
regular style (named parameters, `T a, b;` runs and `T a[3];` arrays in structs); it is no C
parser, and a declaration it cannot read or type raises instead of being guessed."""
from __future__ import annotations

import ctypes as C
import re

_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float}
_DECLARATOR = r"(\w+)(?:\[(\d+)\])?"                          # name or name[3]
_TYPED = re.compile(r"([^()]*[\s*])" + _DECLARATOR, re.S)    # const T* name[3]


def _ctype(ctype: str, structs: dict, decl: str):
    t = [w for w in ctype.replace("*", " * ").split() if w != "const"]
    if t == ["char", "*"]:
        return C.c_char_p
    if t[-1:] == ["*"]:
        return C.POINTER(structs[t[0]]) if len(t) == 2 and t[0] in structs else C.c_void_p
    if len(t) == 1 and t[0] in _SCALARS:
        return _SCALARS[t[0]]
    raise ValueError(f"{decl}: no ctypes type for {ctype.strip()!r}")


def _struct(cname: str, body: str, structs: dict):
    """rs_some_name { T a, b; U* c[3]; } as the ctypes.Structure subclass SomeName."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        m = _TYPED.fullmatch(first)
        rest = [re.fullmatch(_DECLARATOR, s.strip()) for s in more]
        if not m or not all(rest):
            raise ValueError(f"{cname}: cannot read field {decl!r}")
        t = _ctype(m[1], structs, f"{cname}.{m[2]}")
        for name, n in [m.group(2, 3)] + [r.group(1, 2) for r in rest]:
            fields.append((name, t * int(n) if n else t))
    pyname = "".join(w.capitalize() for w in cname.removeprefix("rs_").split("_"))
    return type(pyname, (C.Structure,), {"_fields_": fields,
                                         "__doc__": f"include/recsys_hip.h {cname}."})


def read_header(text: str):
    """(constants {RS_NAME: int}, structs {C name: ctypes.Structure subclass},
    functions {name: (restype, [argtypes])}), each in the header's order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {n: int(v, 0) for n, v in re.findall(
        r"^[ \t]*#[ \t]*define[ \t]+(RS_\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))\)?[ \t]*$",
        text, re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M)
    structs: dict = {}
    for m in re.finditer(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        structs[m[2]] = _struct(m[2], m[1], structs)
        text = text.replace(m[0], "")
    funcs = {}
    # the one brace left is the one that closes extern "C"
    for decl in filter(None, (d.strip() for d in text.replace("}", "").split(";"))):
        m = re.fullmatch(r"([^()]*[\s*])(\w+)\s*\(([^()]*)\)", decl)
        params = [] if not m or m[3].strip() in ("", "void") else m[3].split(",")
        typed = [_TYPED.fullmatch(p.strip()) for p in params]
        if not m or not all(p and not p[3] for p in typed):
            raise ValueError(f"cannot read declaration {' '.join(decl.split())!r}")
        funcs[m[2]] = (_ctype(m[1], structs, m[2]),
                       [_ctype(p[1], structs, f"{m[2]}({p[2]})") for p in typed])
    return consts, structs, funcs
