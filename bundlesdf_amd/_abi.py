"""Reader of include/nof.h: the header's constants, struct layouts and prototypes as ctypes.

Standard library only; loads nothing. parse_header understands the forms the header uses and refuses
every other one with a ValueError naming the declaration: a wrong guess here would hand the library a
descriptor whose pointers sit at the wrong offsets.
"""
import ctypes
import keyword
import re

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t}

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
# the include guard, the extern "C" guard, includes and integer constants: no other conditional, no pragma
_DIRECTIVE = re.compile(r"#\s*(?:include\b.*|ifndef\s+\w+|ifdef\s+__cplusplus|endif|define\s+\w+"
                        r"|define\s+(NOF_\w+)\s+(%s))" % _INT)
_TOP = re.compile(r"""\s*(?:
      (?P<close>\})
    | typedef\s+struct\s*\{(?P<fields>[^}]*)\}\s*(?P<struct>\w+)\s*;
    | (?:typedef\s+)?enum\s*\{(?P<enum>[^{}]*)\}\s*\w*\s*;
    | (?P<const>const\s+)?(?P<ret>\w+)\b\s*(?P<star>\*?)\s*\b(?P<fn>\w+)\s*\((?P<params>[^(){};]*)\)\s*;
    )""", re.X)
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\b\s*(\**)\s*\b(\w+)")


def _words(s):
    return " ".join(s.split())


def _scalar(name, where):
    if name not in SCALARS:
        raise ValueError(f"nof.h: type '{name}' is not one of {', '.join(SCALARS)}: {_words(where)}")
    return SCALARS[name]


def _fields(body, struct, constants):
    if "{" in body:
        raise ValueError(f"nof.h: nested struct or union: {_words(body)}")
    out = []
    for decl in filter(None, map(str.strip, body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\b\s*(.*)", decl, re.S)
        for d in m[2].split(",") if m else [""]:
            dm = _DECLARATOR.fullmatch(d.strip())
            if not dm:
                raise ValueError(f"nof.h: cannot read this member of {struct}: {_words(decl)}")
            stars, name, dim = dm.groups()
            kind = ctypes.c_void_p if stars else _scalar(m[1], f"{decl} in {struct}")
            if dim is not None:
                if not dim.isdigit() and dim not in constants:
                    raise ValueError(f"nof.h: array size '{dim}' is not defined: {_words(decl)} in {struct}")
                kind = kind * (int(dim) if dim.isdigit() else constants[dim])
            out.append((name + "_" if keyword.iskeyword(name) else name, kind))
    return out


def _enumerators(body, constants):
    value = -1
    for e in filter(None, map(str.strip, body.split(","))):
        m = re.fullmatch(r"(\w+)\s*(?:=\s*(%s))?" % _INT, e)
        if not m:
            raise ValueError(f"nof.h: cannot read this enumerator: {_words(e)}")
        value = int(m[2], 0) if m[2] else value + 1
        constants[m[1]] = value


def _prototype(m):
    what = _words(m.group(0))
    if m["star"]:
        if not m["const"] or m["ret"] != "char":
            raise ValueError(f"nof.h: the only pointer a function may return is const char *: {what}")
        res = ctypes.c_char_p
    else:
        res = None if m["ret"] == "void" else _scalar(m["ret"], what)
    args = []
    params = m["params"].strip()
    for p in [] if params == "void" else params.split(","):
        pm = _PARAM.fullmatch(p.strip())
        if not pm:
            raise ValueError(f"nof.h: cannot read parameter '{_words(p)}' of {what}")
        args.append(ctypes.c_void_p if pm[2] else _scalar(pm[1], what))
    return args, res


def parse_header(text):
    """(constants, structs, functions) of the header text: name -> int, name -> [(field, ctypes type)] in
    the header's order, name -> (argtypes, restype). Every pointer is c_void_p (callers pass byref)."""
    constants, structs, functions = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    lines = text.split("\n")
    for n, line in enumerate(lines):
        if line.lstrip().startswith("#"):
            m = _DIRECTIVE.fullmatch(line.strip())
            if not m:
                raise ValueError(f"nof.h: cannot read this preprocessor line: {_words(line)}")
            if m[1]:
                constants[m[1]] = int(m[2], 0)
            lines[n] = ""
    text, open_braces = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(lines))
    pos = 0
    while text[pos:].strip():
        m = _TOP.match(text, pos)
        if not m or (m["close"] and not open_braces):
            raise ValueError(f"nof.h: cannot read the text at: {_words(text[pos:])[:80]}")
        if m["close"]:
            open_braces -= 1
        elif m["struct"]:
            structs[m["struct"]] = _fields(m["fields"], m["struct"], constants)
        elif m["enum"] is not None:
            _enumerators(m["enum"], constants)
        else:
            functions[m["fn"]] = _prototype(m)
        pos = m.end()
    return constants, structs, functions
