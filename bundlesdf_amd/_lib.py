"""ctypes binding of libnof.so, derived at import from include/nof.h (the C ABI).

Nothing of the header is restated here. _abi.parse_header reads it once and this module makes of it
_SIGNATURES (argtypes and restype of every prototype), one ctypes.Structure per typedef struct under its
name without nof_, in CamelCase (nof_field_desc -> FieldDesc), and one attribute per #define and
enumerator under its name without NOF_ (NOF_FT_CROSS -> FT_CROSS). Every pointer is a c_void_p, a field
named like a Python keyword gets a trailing underscore (in -> in_). The reader refuses what it does not
know (a type outside its scalar table, a nested struct or union, a bit-field, a function pointer, a
variadic prototype, any text it cannot account for) with a ValueError naming the declaration, so a
header this module cannot follow stops the import instead of loading a library with another layout.

torch is imported first so that its bundled HIP runtime (soname
libamdhip64.so.7) is the one libnof.so binds to: one runtime, one set of
streams. There is no CPU fallback anywhere behind this module — a missing or
unloadable library raises immediately.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see module doc)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# NOF_LIB: the timing-ablation build (scripts/ablate.py) only
LIB_PATH = os.environ.get("NOF_LIB") or os.path.join(_HERE, "libnof.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nof.h"))
_LIB = None

_p = ctypes.c_void_p


def _bind():
    """Make the header's constants and structs attributes of this module; return its prototypes."""
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the binding of libnof.so is derived from it "
                           "(there is no hand-written copy to fall back on)")
    with open(HEADER_PATH) as f:
        constants, structs, functions = _abi.parse_header(f.read())
    attrs = [(name.removeprefix("NOF_"), value) for name, value in constants.items()]
    for cname, fields in structs.items():
        name = "".join(w.capitalize() for w in cname.removeprefix("nof_").split("_"))
        doc = f"{cname} of include/nof.h."
        attrs.append((name, type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": doc})))
    for name, value in attrs:
        if name in globals():
            raise RuntimeError(f"{HEADER_PATH}: {name} would replace an attribute of {__name__}")
        globals()[name] = value
    return functions


_SIGNATURES = _bind()


def declared_symbols():
    return list(_SIGNATURES)


def check_field_desc_layout(L, struct=FieldDesc):
    """Raise unless library L was built from the nof_field_desc that `struct` mirrors: a library
    from another header (NOF_LIB, a stale libnof_prev.so / libnof_ablate.so) would read the
    descriptor's pointers from the wrong offsets."""
    fn = getattr(L, "nof_field_desc_size", None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} does not export nof_field_desc_size: it predates this binding's "
                           f"nof_field_desc ({ctypes.sizeof(struct)} bytes) — rebuild it")
    fn.argtypes, fn.restype = _SIGNATURES["nof_field_desc_size"]
    if fn() != ctypes.sizeof(struct):
        raise RuntimeError(f"{LIB_PATH}: nof_field_desc is {fn()} bytes in the library, {ctypes.sizeof(struct)} "
                           "in this binding — rebuild the library from the current include/nof.h")


def lib():
    """Load libnof.so once; raise if it is missing (no fallback) or built from another
    nof_field_desc than FieldDesc mirrors."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m bundlesdf_amd.build` "
                               "(the HIP path has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        check_field_desc_layout(L)
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _LIB = L
    return _LIB


def check(rc, what=""):
    if rc != 0:
        msg = lib().nof_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {msg}" if what else msg)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_of(t):
    """Current HIP stream of tensor t's device (graph-capture safe)."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_device(t, name):
    if not (t.is_cuda):
        raise RuntimeError(f"{name} must be a CUDA tensor")


def require_contiguous(t, name, wording="a contiguous tensor"):
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be {wording}")
