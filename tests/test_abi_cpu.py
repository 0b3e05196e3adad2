"""CPU: the binding bundlesdf_amd/_lib.py derives from include/nof.h. gcc states the layout of every
struct and the value of every constant the reader found; tests/golden/abi_parent.json, recorded from the
last hand-written binding, pins the argument lists gcc cannot state; header snippets pin what the
reader accepts and what it refuses."""
import ctypes
import json
import keyword
import os
import subprocess

import pytest

from bundlesdf_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nof.h")
with open(HEADER) as _f:
    CONSTANTS, STRUCTS, FUNCTIONS = _abi.parse_header(_f.read())


def _mirror(cname):
    """The _lib class of a header struct: nof_frame_covis_desc -> _lib.FrameCovisDesc."""
    from bundlesdf_amd import _lib
    return getattr(_lib, "".join(w.capitalize() for w in cname.removeprefix("nof_").split("_")))


@pytest.fixture(scope="module")
def gcc(tmp_path_factory):
    """One compile of the header: {"S name": [size], "F name field": [offset, size], "C name": [value]}."""
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    for cname, fields in STRUCTS.items():
        src.append(f'  printf("S {cname}=%zu\\n", sizeof({cname}));')
        for f, _ in fields:
            c = f[:-1] if f.endswith("_") and keyword.iskeyword(f[:-1]) else f      # in_ -> in
            src.append(f'  printf("F {cname} {f}=%zu %zu\\n", offsetof({cname}, {c}), sizeof((({cname} *)0)->{c}));')
    src += [f'  printf("C {name}=%lld\\n", (long long)({name}));' for name in CONSTANTS] + ['  return 0;', '}']
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-o", str(d / "layout"), str(d / "layout.c")], check=True)
    out = subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout
    return {key: [int(v) for v in vals.split()] for key, vals in (line.split("=") for line in out.splitlines())}


def test_reader_finds_the_whole_header():
    assert len(STRUCTS) >= 19 and len(FUNCTIONS) >= 78 and len(CONSTANTS) >= 14
    assert [_mirror(c).__name__ for c in "nof_field_desc nof_view_out nof_frame_covis_desc nof_step_params".split()] \
        == ["FieldDesc", "ViewOut", "FrameCovisDesc", "StepParams"]


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_gcc(gcc, cname):
    """Size of the struct, offset and size of every field: ctypes against gcc on the same header."""
    S = _mirror(cname)
    assert issubclass(S, ctypes.Structure) and S._fields_ == STRUCTS[cname]
    assert ctypes.sizeof(S) == gcc[f"S {cname}"][0]
    assert [k for k in gcc if k.startswith(f"F {cname} ")] == [f"F {cname} {f}" for f, _ in S._fields_]
    for f, _ in S._fields_:
        assert [getattr(S, f).offset, getattr(S, f).size] == gcc[f"F {cname} {f}"], f


def test_constants_match_gcc(gcc):
    from bundlesdf_amd import _lib
    for name, value in CONSTANTS.items():
        assert name.startswith("NOF_") and getattr(_lib, name[4:]) == value == gcc[f"C {name}"][0], name
    assert [_lib.MESH_COLOUR_FLAT, _lib.MESH_COLOUR_VERTEX, _lib.MESH_COLOUR_TEXTURE] == [0, 1, 2]
    assert [_lib.FT_SELF, _lib.FT_CROSS, _lib.FT_MAX_LAYERS, _lib.F16, _lib.WS_SECTIONS] == [0, 1, 16, 1, 13]


def _kind(t):
    """A ctypes type as the record states it: None, [name, bytes] or {"array": element, "length": n}."""
    if t is None:
        return None
    if issubclass(t, ctypes.Array):
        return {"array": _kind(t._type_), "length": t._length_}
    return [t.__name__, ctypes.sizeof(t)]


def test_binding_equals_the_parent_record(golden_dir):
    """Every prototype and struct of the last hand-written binding (78 and 19, frozen: later entry points
    are not added to the record) comes out of the reader with the same types in the same order."""
    from bundlesdf_amd import _lib
    with open(os.path.join(golden_dir, "abi_parent.json")) as f:
        record = json.load(f)
    assert len(record["functions"]) == 78 and len(record["structs"]) == 19
    for name, want in record["functions"].items():
        args, res = _lib._SIGNATURES[name]
        assert {"args": [_kind(a) for a in args], "res": _kind(res)} == want, name
    for cname, want in record["structs"].items():
        assert [[f, _kind(t)] for f, t in _mirror(cname)._fields_] == want, cname


def test_a_missing_header_stops_the_binding(monkeypatch, tmp_path):
    from bundlesdf_amd import _lib
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "nof.h"))
    with pytest.raises(RuntimeError, match=str(tmp_path / "nof.h")):
        _lib._bind()


def test_a_long_field_in_the_real_header_is_refused():
    with open(HEADER) as f:
        broken = f.read().replace("    int32_t quads_prebuilt;", "    long quads_prebuilt;")
    with pytest.raises(ValueError, match=r"'long'.*long quads_prebuilt in nof_field_desc"):
        _abi.parse_header(broken)


ACCEPTED = """
#ifndef NOF_H
#define NOF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef enum { NOF_A = 0, NOF_B = 3, NOF_C } nof_kind;   /* NOF_C follows NOF_B */
enum { NOF_X = 0x10 };
#define NOF_N 5
typedef struct {
    const float *a, *b, c;    /* one declaration, mixed stars */
    // a line comment; with a semicolon
    float m[16];
    int32_t k[NOF_N], n;
    const void *in;           /* a Python keyword */
    uint8_t *rows[2];
    size_t bytes;
} nof_thing;
const char *nof_name(void);
void nof_fill(uint32_t n, float *out);
int nof_run(const nof_thing *t, int64_t n,
            double x,    /* a comment between parameters */
            void *stream);
#ifdef __cplusplus
}
#endif
#endif /* NOF_H */
"""


def test_reader_accepts_the_headers_forms():
    p, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    constants, structs, functions = _abi.parse_header(ACCEPTED)
    assert constants == {"NOF_A": 0, "NOF_B": 3, "NOF_C": 4, "NOF_X": 16, "NOF_N": 5}
    assert list(structs) == ["nof_thing"]
    names, kinds = zip(*structs["nof_thing"])
    assert names == ("a", "b", "c", "m", "k", "n", "in_", "rows", "bytes")
    assert kinds[:3] == (p, p, f32) and kinds[5:7] == (i32, p) and kinds[8] is ctypes.c_size_t
    assert [(k._type_, k._length_) for k in (kinds[3], kinds[4], kinds[7])] == [(f32, 16), (i32, 5), (p, 2)]
    assert functions == {"nof_name": ([], ctypes.c_char_p), "nof_fill": ([ctypes.c_uint32, p], None),
                         "nof_run": ([p, ctypes.c_int64, ctypes.c_double, p], ctypes.c_int)}


@pytest.mark.parametrize("text,named", [
    ("typedef struct { long n; } nof_t;", "long n in nof_t"),
    ("typedef struct { bool on; } nof_t;", "bool on in nof_t"),
    ("typedef struct { int32_t a; struct { int32_t b; } c; } nof_t;", "struct { int32_t b"),
    ("typedef struct { union { int32_t b; float f; } u; } nof_t;", "union { int32_t b"),
    ("typedef union { int32_t b; float f; } nof_u;", "typedef union"),
    ("typedef struct { uint32_t flag : 1; } nof_t;", "uint32_t flag : 1"),
    ("typedef struct { void (*done)(int); } nof_t;", "void (*done)(int)"),
    ("typedef struct { float m[4][4]; } nof_t;", "float m[4][4]"),
    ("typedef struct { float m[NOF_MISSING]; } nof_t;", "NOF_MISSING"),
    ("int nof_log(const char *fmt, ...);", "'...' of int nof_log"),
    ("int nof_f(nof_thing by_value);", "'nof_thing'"),
    ("int nof_f(int32_t);", "'int32_t' of int nof_f"),
    ("int nof_f(void (*cb)(int));", "int nof_f(void"),
    ("float *nof_f(void);", "float *nof_f(void)"),
    ("int nof_f(void);\nstatic int leftover;\nint nof_g(void);", "static int leftover"),
    ("}", "}"),
    ("#define NOF_N (1 << 4)", "#define NOF_N (1 << 4)"),
    ("#pragma pack(1)", "#pragma pack(1)"),
    ("#ifdef NOF_WIDE\nint nof_f(void);\n#endif", "#ifdef NOF_WIDE"),
    ("enum { NOF_A = 1 << 2 };", "NOF_A = 1 << 2"),
])
def test_reader_refuses_what_it_does_not_know(text, named):
    with pytest.raises(ValueError) as e:
        _abi.parse_header(text)
    assert named in str(e.value), str(e.value)
