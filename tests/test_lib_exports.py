"""CPU: libnof.so (the C-ABI drop-in) loads and exports every entry point
include/nof.h declares, and the Python binding declares exactly those. No
compute calls are made here (no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "nof.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nof_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def libnof():
    from bundlesdf_amd import build
    build.build()
    from bundlesdf_amd import _lib
    return _lib.lib()


def test_header_symbols_exported(libnof):
    syms = _header_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(libnof, s), f"{s} declared in include/nof.h but not exported"


def test_binding_matches_header():
    from bundlesdf_amd import _lib
    assert sorted(_lib.declared_symbols()) == _header_symbols()


def test_host_only_entry_points(libnof):
    import numpy as np
    from oracle import kernels as K
    sc = np.zeros(16, np.float32)
    res = np.zeros(16, np.uint32)
    libnof.nof_level_params(16, np.float32(0.2), 16, sc.ctypes.data_as(ctypes.c_void_p),
                            res.ctypes.data_as(ctypes.c_void_p))
    osc, ores = K.level_params(16, np.float32(0.2), 16)
    np.testing.assert_array_equal(sc, osc)
    np.testing.assert_array_equal(res, ores)
    assert b"gfx950" in libnof.nof_version()


def test_field_desc_size_matches_loaded_library(libnof):
    """The loaded library's nof_field_desc is the one _lib.FieldDesc mirrors (lib() checks this at
    load); a mirror of another size — a library built from another header, seen from the other
    side — is refused."""
    from bundlesdf_amd import _lib
    assert libnof.nof_field_desc_size() == ctypes.sizeof(_lib.FieldDesc)
    _lib.check_field_desc_layout(libnof)

    class Longer(ctypes.Structure):
        _fields_ = _lib.FieldDesc._fields_ + [("extra", ctypes.c_int32)]

    assert ctypes.sizeof(Longer) != ctypes.sizeof(_lib.FieldDesc)
    with pytest.raises(RuntimeError) as e:
        _lib.check_field_desc_layout(libnof, Longer)
    msg = str(e.value)
    assert _lib.LIB_PATH in msg and str(ctypes.sizeof(Longer)) in msg and str(ctypes.sizeof(_lib.FieldDesc)) in msg


def test_library_without_size_export_is_refused():
    from bundlesdf_amd import _lib

    class NoExport:   # a library older than nof_field_desc_size: the symbol lookup fails
        pass

    with pytest.raises(RuntimeError, match="nof_field_desc_size"):
        _lib.check_field_desc_layout(NoExport())


def test_field_step_refuses_bad_descriptors_before_device_work(libnof):
    """nof_field_step validates the whole descriptor before its first HIP call: a bad one returns
    NOF_EINVAL and names the field on a machine with no GPU (no hang, no crash)."""
    from bundlesdf_amd import _lib
    D = _lib.FieldDesc()
    D.S = 33
    assert libnof.nof_field_step(ctypes.byref(D), None) != 0
    assert b"S=33" in libnof.nof_last_error()
    D = _lib.FieldDesc()
    D.R, D.S, D.N_oct, D.N_dep, D.L, D.C, D.D = 1, 64, 32, 32, 16, 2, 3
    D.bwd_flush = 3
    assert libnof.nof_field_step(ctypes.byref(D), None) != 0
    assert b"bwd_flush 3" in libnof.nof_last_error()
