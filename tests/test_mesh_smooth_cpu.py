"""CPU: the host backend ("scipy") of the mesh smoothing functions in bundlesdf_amd/mesh.py against
tests/mesh_smooth_oracle.py, on a tetrahedron, an open grid patch, the tetrahedron with an isolated
vertex and a degenerate face, and a marching-cubes bumpy sphere. Vertices must agree within 1e-12 of
the bounding-box diagonal: the host backend is the same definition, summed by scipy / numpy."""
import os

import numpy as np
import pytest

from bundlesdf_amd import evaluate as E
from bundlesdf_amd import mesh as M
from tests import mesh_smooth_oracle as O

NAMES = sorted(O.FIXTURES)
CLOSED = ["bumpy_sphere", "tetrahedron", "tetrahedron_plus"]


def _mesh(name):
    v, f = O.FIXTURES[name]()
    return M.Mesh(v.copy(), f.copy())


def _close(got, want, ref):
    tol = 1e-12 * O.bbox_diagonal(ref)
    err = float(np.abs(got - want).max())
    print(f"max |got - want| = {err:.3e}, tolerance {tol:.3e}")
    assert got.shape == want.shape and err <= tol


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_on_the_host_is_the_oracles(name):
    v, f = O.FIXTURES[name]()
    rs, cols = M.vertex_adjacency(f, len(v), device="cpu")
    ors, ocols = O.vertex_adjacency(f, len(v))
    assert rs.dtype == cols.dtype and str(rs.dtype) == "torch.int32"
    assert np.array_equal(rs.numpy(), ors) and np.array_equal(cols.numpy(), ocols)
    frs, fids = M.vertex_faces(f, len(v), device="cpu")
    ofrs, ofids = O.vertex_faces(f, len(v))
    assert np.array_equal(frs.numpy(), ofrs) and np.array_equal(fids.numpy(), ofids)


def test_adjacency_rules():
    v, f = O.tetrahedron_plus()
    rs, cols = (t.numpy() for t in M.vertex_adjacency(f, len(v), device="cpu"))
    assert rs.tolist() == [0, 3, 6, 9, 12, 12]          # shared edges once, no self-edge, an empty row
    assert cols[:3].tolist() == [1, 2, 3]
    with pytest.raises(ValueError):
        M.vertex_adjacency([[0, 1, 5]], 5, device="cpu")
    with pytest.raises(ValueError):
        M.vertex_adjacency([[0, -1, 2]], 5, device="cpu")


def test_sphere_fixture_is_what_the_tests_assume():
    v, f = O.bumpy_sphere()
    rs, _ = O.vertex_adjacency(f, len(v))
    deg = np.diff(rs)
    assert (len(v), len(f), int(deg.min()), int(deg.max())) == (1240, 2476, 4, 9)
    e = np.sort(np.asarray(f)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()
    assert O.volume(v, f) > 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("iterations", [1, 3])
def test_filter_laplacian_without_constraint(name, iterations):
    v, f = O.FIXTURES[name]()
    m = M.filter_laplacian(_mesh(name), lamb=0.5, iterations=iterations, volume_constraint=False, backend="scipy")
    _close(m.vertices, O.filter_laplacian(v, f, 0.5, iterations, False), v)


@pytest.mark.parametrize("name", CLOSED)
def test_filter_laplacian_with_constraint(name):
    v, f = O.FIXTURES[name]()
    m = M.filter_laplacian(_mesh(name), lamb=0.5, iterations=3, volume_constraint=True, backend="scipy")
    _close(m.vertices, O.filter_laplacian(v, f, 0.5, 3, True), v)


@pytest.mark.parametrize("name", NAMES)
def test_filter_taubin(name):
    v, f = O.FIXTURES[name]()
    m = M.filter_taubin(_mesh(name), lamb=0.5, nu=0.53, iterations=5, backend="scipy")
    _close(m.vertices, O.filter_taubin(v, f, 0.5, 0.53, 5), v)


def test_isolated_vertex_stays():
    v, _ = O.tetrahedron_plus()
    m = M.filter_laplacian(_mesh("tetrahedron_plus"), iterations=2, volume_constraint=False, backend="scipy")
    assert np.array_equal(m.vertices[4], v[4]) and not np.array_equal(m.vertices[:4], v[:4])


def test_volume_is_kept_with_the_constraint_and_shrinks_without():
    v, f = O.bumpy_sphere()
    vol0 = O.volume(v, f)
    assert abs(M.mesh_volume(v, f, backend="scipy") - vol0) <= 1e-12 * vol0
    assert abs(M.mesh_volume(_mesh("bumpy_sphere"), backend="scipy") - vol0) <= 1e-12 * vol0
    kept = M.filter_laplacian(_mesh("bumpy_sphere"), iterations=10, volume_constraint=True, backend="scipy")
    rel = abs(O.volume(kept.vertices, f) - vol0) / vol0
    print(f"relative volume change with the constraint: {rel:.3e}")
    assert rel <= 1e-12
    vols = [vol0]
    m = _mesh("bumpy_sphere")
    for _ in range(10):
        M.filter_laplacian(m, iterations=1, volume_constraint=False, backend="scipy")
        vols.append(O.volume(m.vertices, f))
    assert all(b < a for a, b in zip(vols, vols[1:]))
    taubin = M.filter_taubin(_mesh("bumpy_sphere"), iterations=10, backend="scipy")
    ratio = O.volume(taubin.vertices, f) / vol0
    print(f"volume ratios after 10 iterations: laplacian {vols[-1] / vol0:.4f}, taubin {ratio:.4f}")
    assert abs(ratio - 1.0) <= 0.01


def test_open_or_inverted_mesh_with_constraint_raises_and_is_left_alone():
    for mesh in (_mesh("grid_patch"), M.Mesh(O.bumpy_sphere()[0].copy(), O.bumpy_sphere()[1][:, [0, 2, 1]].copy())):
        before = mesh.vertices.copy()
        mesh.vertex_normals = np.ones_like(before)
        assert M.mesh_volume(mesh, backend="scipy") < 0
        with pytest.raises(ValueError, match="volume_constraint needs a closed, outward-oriented mesh"):
            M.filter_laplacian(mesh, iterations=3, volume_constraint=True, backend="scipy")
        assert np.array_equal(mesh.vertices, before) and mesh.vertex_normals is not None


def test_zero_iterations_is_the_identity():
    for fn in (M.filter_laplacian, M.filter_taubin):
        m = _mesh("grid_patch")
        before = m.vertices.copy()
        assert fn(m, iterations=0, backend="scipy") is m
        assert np.array_equal(m.vertices, before)


def test_attributes_survive_and_normals_are_cleared():
    m = _mesh("bumpy_sphere")
    n = len(m.vertices)
    m.vertex_colors = np.arange(n * 3, dtype=np.uint32).reshape(n, 3).astype(np.uint8)
    m.vertex_color_counts = np.arange(n, dtype=np.int32)
    m.uv = np.linspace(0, 1, n * 2).reshape(n, 2)
    m.texture = np.zeros((4, 4, 3), np.uint8)
    m.vertex_normals = np.ones((n, 3))
    keep = m.copy()
    faces = m.faces.copy()
    for fn in (M.filter_laplacian, M.filter_taubin):
        assert fn(m, iterations=2, backend="scipy") is m
        assert m.vertex_normals is None and np.array_equal(m.faces, faces)
        assert np.array_equal(m.vertex_colors, keep.vertex_colors) and np.array_equal(m.uv, keep.uv)
        assert np.array_equal(m.vertex_color_counts, keep.vertex_color_counts) and m.texture is not None
        assert not np.array_equal(m.vertices, keep.vertices)


def test_unknown_backend_raises():
    m = _mesh("tetrahedron")
    for call in (lambda: M.filter_laplacian(m, backend="torch"), lambda: M.filter_taubin(m, backend="cuda"),
                 lambda: M.mesh_volume(m, backend=""), lambda: m.compute_vertex_normals(backend="numpy"),
                 lambda: M.postprocess_mesh(m, np.zeros(3), 1.0, backend="trimesh")):
        with pytest.raises(ValueError, match="backend must be"):
            call()


@pytest.mark.parametrize("name", NAMES)
def test_vertex_normals_on_the_host(name):
    v, f = O.FIXTURES[name]()
    m = _mesh(name)
    got = m.compute_vertex_normals(backend="scipy")
    assert got is m.vertex_normals
    want = O.vertex_normals(v, f, *O.vertex_faces(f, len(v)))
    assert np.abs(got - want).max() <= 1e-12
    if name == "tetrahedron_plus":
        assert np.array_equal(got[4], np.zeros(3))
    if name == "bumpy_sphere":
        assert (np.sum(got * v, axis=1) > 0).all()
        assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-15 * 4


def _messy_mesh():
    v, f = O.tetrahedron()
    v = np.concatenate([v, v[:1], [[5.0, 5.0, 5.0]]])              # a duplicate of vertex 0, an unused vertex
    f = np.concatenate([f, [[4, 2, 1]], [[1, 2, 0]], [[0, 0, 1]], [[3, 2, 2]]])   # duplicates and degenerates
    m = M.Mesh(v, f)
    m.vertex_colors = (np.arange(len(v) * 3).reshape(len(v), 3) * 7 % 256).astype(np.uint8)
    return m


def test_trimesh_clean_is_evaluates_clean():
    a, b = _messy_mesh(), _messy_mesh()
    assert M.trimesh_clean(a) is a
    E._clean(b)
    assert len(a.vertices) == 4 and len(a.faces) == 4
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces)
    assert np.array_equal(a.vertex_colors, b.vertex_colors)


def test_postprocess_mesh(tmp_path):
    v, f = O.bumpy_sphere()
    tv, tf = O.tetrahedron()
    sc, tr = 2.5, np.array([0.1, -0.2, 0.3])
    both = M.Mesh(np.concatenate([(v + tr) * sc, (tv * 0.01 + 3.0 + tr) * sc]), np.concatenate([f, tf + len(v)]))
    before = both.vertices.copy()
    out = M.postprocess_mesh(both, tr, sc, out_dir=str(tmp_path / "mesh"), min_edge=100, backend="scipy")
    assert sorted(out) == ["biggest_component", "real_scale", "smoothed"]
    assert np.array_equal(both.vertices, before)                       # it works on a copy
    assert len(out["real_scale"].vertices) == len(v) + 4
    assert np.abs(out["real_scale"].vertices[:len(v)] - v).max() <= 1e-15 * 8
    big = out["biggest_component"]
    assert len(big.vertices) == len(v) and len(big.faces) == len(f)
    want = O.filter_laplacian(big.vertices, big.faces, 0.5, 3, True)
    _close(out["smoothed"].vertices, want, big.vertices)
    assert np.array_equal(out["smoothed"].faces, big.faces)
    assert out["smoothed"].vertex_normals is not None and big.vertex_normals is None
    for name in ("mesh_real_scale.obj", "mesh_biggest_component.obj", "mesh_biggest_component_smoothed.obj"):
        assert os.path.getsize(tmp_path / "mesh" / name) > 0
    with pytest.raises(ValueError, match="no component"):
        M.postprocess_mesh(both, tr, sc, min_edge=10 ** 6, backend="scipy")
