"""CPU: the opt-in switches of the device mesher (mesh.marching_cubes(backend=...),
trimesh_split / largest_component(backend=...), NerfRunner.extract_mesh(mesher=...)) reject unknown
values before any work, the new entry points of libnof.so validate the volume's shape before any
device work (null device pointers, no GPU needed), and the table the kernels read is the one mesh.py
generates."""
import ctypes

import numpy as np
import pytest

from bundlesdf_amd import mesh as M

EINVAL = 1   # NOF_EINVAL, include/nof.h


def test_unknown_backends_raise():
    vol = np.linspace(-1, 1, 27, dtype=np.float32).reshape(3, 3, 3)
    with pytest.raises(ValueError, match="backend"):
        M.marching_cubes(vol, 0.0, backend="bogus")
    v, f = M.marching_cubes(vol, 0.0, backend="torch")
    v0, f0 = M.marching_cubes(vol, 0.0)
    assert np.array_equal(v, v0) and np.array_equal(f, f0) and len(f) > 0
    m = M.Mesh(v, f)
    with pytest.raises(ValueError, match="backend"):
        M.trimesh_split(m, min_edge=1, backend="bogus")
    with pytest.raises(ValueError, match="backend"):
        M.largest_component(m, backend="bogus")
    assert len(M.trimesh_split(m, min_edge=1, backend="scipy")) == len(M.trimesh_split(m, min_edge=1)) == 1


def test_extract_mesh_rejects_unknown_mesher():
    from bundlesdf_amd.nerf_runner import NerfRunner
    nr = NerfRunner.__new__(NerfRunner)   # the check runs before anything of the runner is touched
    nr.cfg = {}
    with pytest.raises(ValueError, match="mesher"):
        nr.extract_mesh(mesher="bogus")
    nr.cfg = {"mesh_extractor": "bogus"}
    with pytest.raises(ValueError, match="mesher"):
        nr.extract_mesh()


@pytest.mark.parametrize("shape", [(1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 4, 4), (-3, 4, 4),
                                   (895, 895, 894),               # points * 3 >= 2^31
                                   (1 << 30, 1 << 30, 1 << 30),   # the product does not fit 64 bits
                                   (2, 2, 178956971)])            # 4 points over the largest legal 2 x 2 x n
def test_entry_points_reject_bad_shapes(shape):
    from bundlesdf_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_int64(-7)
    calls = {"blocks": lambda: L.nof_marching_cubes_blocks(*shape, ctypes.byref(nb)),
             "count": lambda: L.nof_marching_cubes_count(None, *shape, 0.0, None, None, None, None, None),
             "emit": lambda: L.nof_marching_cubes_emit(None, *shape, 0.0, None, None, None, 0, 0, None, None, None)}
    for name, call in calls.items():
        assert call() == EINVAL, name
        msg = L.nof_last_error().decode()
        assert f"marching_cubes_{name}" in msg and " x ".join(str(n) for n in shape) in msg, msg
    assert nb.value == -7


def test_entry_points_accept_legal_shapes_and_reject_null_pointers():
    from bundlesdf_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_int64(0)
    for shape, want in (((2, 2, 2), 1), ((16, 16, 1), None), ((7, 9, 33), 9), ((2, 2, 178956970), 2796203),
                        ((40, 37, 70), 405)):
        rc = L.nof_marching_cubes_blocks(*shape, ctypes.byref(nb))
        if want is None:
            assert rc == EINVAL
        else:
            assert rc == 0 and nb.value == want == -(-shape[0] * shape[1] * shape[2] // 256), shape
    # a legal shape with null pointers: refused by name, nothing launched
    assert L.nof_marching_cubes_count(None, 4, 4, 4, 0.0, None, None, None, None, None) == EINVAL
    assert "volume is NULL" in L.nof_last_error().decode()
    assert L.nof_marching_cubes_emit(None, 4, 4, 4, 0.0, None, None, None, 0, 0, None, None, None) == EINVAL
    assert "volume is NULL" in L.nof_last_error().decode()
    assert L.nof_marching_cubes_count(None, 4, 4, 4, float("nan"), None, None, None, None, None) == EINVAL
    assert "level" in L.nof_last_error().decode()
    for F, V, word in ((-1, 4, "n_faces"), (1 << 31, 4, "n_faces"), (4, -1, "n_vertices"), (4, 1 << 31, "n_vertices"),
                       (4, 4, "changed is NULL")):
        assert L.nof_mesh_components(None, F, V, None, None, None) == EINVAL
        assert word in L.nof_last_error().decode()


def test_device_table_is_mesh_py_table():
    """The [256,16] table of device_tables decodes back to TRI_COUNT / TRI_TABLE / EDGE_CORNER / EDGE_AXIS."""
    import torch
    t = M.device_tables(torch.device("cpu")).numpy()
    assert t.shape == (256, 16) and t.dtype == np.uint8
    np.testing.assert_array_equal(t[:, 0], M.TRI_COUNT)
    for case in range(256):
        n = int(M.TRI_COUNT[case])
        codes = t[case, 1:].reshape(5, 3)
        edges = M.TRI_TABLE[case, :n]
        np.testing.assert_array_equal(codes[:n] & 7, M.EDGE_CORNER[edges])
        np.testing.assert_array_equal(codes[:n] >> 3, M.EDGE_AXIS[edges])
        assert not codes[n:].any()
