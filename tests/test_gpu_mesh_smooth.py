"""GPU: the mesh smoothing kernels (csrc/mesh_smooth.hip) and their Python side against
tests/mesh_smooth_oracle.py. The adjacency, one Laplacian step, the unconstrained filters and the
vertex-normal sums are compared exactly: the operation order is fixed and contraction is off, so
bit equality is the specification. The volume is held to the worst-case bound of any summation
order, and whatever passes through the device's cbrt to 1e-9 of the bounding-box diagonal."""
import numpy as np
import pytest
import torch

from bundlesdf_amd import _lib
from bundlesdf_amd import mesh as M
from tests import mesh_smooth_oracle as O

pytestmark = pytest.mark.gpu

NAMES = sorted(O.FIXTURES)
CLOSED = ["bumpy_sphere", "tetrahedron", "tetrahedron_plus"]
EPS = 2.0 ** -53


def _mesh(name):
    v, f = O.FIXTURES[name]()
    return M.Mesh(v.copy(), f.copy())


def _dev(a, dev, dtype):
    return torch.from_numpy(np.array(a)).to(dev, dtype).contiguous()


def _step(dev, v, row_start, cols, factor):
    vin = _dev(v, dev, torch.float64)
    out = torch.full_like(vin, float("nan"))
    _lib.check(_lib.lib().nof_mesh_laplacian_step(_lib.ptr(vin), _lib.ptr(row_start), _lib.ptr(cols), len(v), factor,
                                                  _lib.ptr(out), _lib.stream_of(vin)), "mesh_laplacian_step")
    return out.cpu().numpy()


def _volume(dev, v, f):
    L = _lib.lib()
    vd, fd = _dev(v, dev, torch.float64), _dev(f, dev, torch.int32)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.nof_mesh_volume_workspace_bytes(len(f))), dtype=torch.uint8, device=dev)
    _lib.check(L.nof_mesh_volume(_lib.ptr(vd), _lib.ptr(fd), len(f), _lib.ptr(out), _lib.ptr(ws), _lib.stream_of(vd)),
               "mesh_volume")
    return float(out.item())


def _close(got, want, ref, rel=1e-9):
    tol = rel * O.bbox_diagonal(ref)
    err = float(np.abs(got - want).max())
    print(f"max |got - want| = {err:.3e}, tolerance {tol:.3e}")
    assert got.shape == want.shape and err <= tol


@pytest.mark.parametrize("name", NAMES)
def test_vertex_adjacency_is_the_oracles_csr(cuda_device, name):
    v, f = O.FIXTURES[name]()
    rs, cols = M.vertex_adjacency(f, len(v), device=cuda_device)
    assert rs.is_cuda and cols.is_cuda and rs.dtype == torch.int32 and cols.dtype == torch.int32
    ors, ocols = O.vertex_adjacency(f, len(v))
    assert np.array_equal(rs.cpu().numpy(), ors) and np.array_equal(cols.cpu().numpy(), ocols)
    frs, fids = M.vertex_faces(torch.from_numpy(np.array(f)).to(cuda_device), len(v))
    ofrs, ofids = O.vertex_faces(f, len(v))
    assert fids.is_cuda and np.array_equal(frs.cpu().numpy(), ofrs) and np.array_equal(fids.cpu().numpy(), ofids)
    if name == "tetrahedron_plus":      # shared edges once, the self-edge of (0, 0, 1) dropped, an empty row
        assert ors.tolist() == [0, 3, 6, 9, 12, 12]
        with pytest.raises(ValueError):
            M.vertex_adjacency([[0, 1, 5]], 5, device=cuda_device)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("factor", [0.5, -0.5])
def test_one_laplacian_step_is_bit_equal(cuda_device, name, factor):
    v, f = O.FIXTURES[name]()
    rs, cols = M.vertex_adjacency(f, len(v), device=cuda_device)
    got = _step(cuda_device, v, rs, cols, factor)
    want = O.laplacian_step(v, *O.vertex_adjacency(f, len(v)), factor)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, v)
    if name == "tetrahedron_plus":
        assert np.array_equal(got[4], v[4])


@pytest.mark.parametrize("name", NAMES)
def test_volume_within_the_summation_bound_and_reproducible(cuda_device, name):
    """|device - fsum| <= 4 F 2^-53 sum |term| / 6: F - 1 additions in any order err by at most
    (F - 1) 2^-53 sum |term| to first order, and the factor 4 covers the higher orders and the
    rounding of the division."""
    v, f = O.FIXTURES[name]()
    terms = O.volume_terms(v, f)
    want = O.volume(v, f)
    got = _volume(cuda_device, v, f)
    bound = 4 * len(f) * EPS * float(np.abs(terms).sum()) / 6.0
    print(f"volume {got!r} against {want!r}: off by {abs(got - want):.3e}, bound {bound:.3e}")
    assert abs(got - want) <= bound
    assert _volume(cuda_device, v, f) == got
    assert M.mesh_volume(v, f, backend="hip") == got
    assert _volume(cuda_device, v, f[:0]) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_scale_to_volume(cuda_device, name):
    """The rescale is v * cbrt(target / now) per coordinate; the device's cbrt may differ from numpy's
    in the last place, which moves a coordinate by 2^-52 of itself: 4 * 2^-53 |v| allows it."""
    v, _ = O.FIXTURES[name]()
    L = _lib.lib()
    for target, now, bad in ((2.0, 3.0, 0), (-2.0, -3.0, 0), (2.0, -3.0, 1), (2.0, 0.0, 1), (0.0, 3.0, 1),
                             (float("nan"), 1.0, 1), (float("inf"), 1.0, 1)):
        vd = _dev(v, cuda_device, torch.float64)
        vols = torch.tensor([target, now], dtype=torch.float64, device=cuda_device)
        flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        _lib.check(L.nof_mesh_scale_to_volume(_lib.ptr(vd), len(v), _lib.ptr(vols[0:]), _lib.ptr(vols[1:]),
                                              _lib.ptr(flag), _lib.stream_of(vd)), "mesh_scale_to_volume")
        want, want_flag = O.scale_to_volume(v, target, now)
        assert int(flag.item()) == want_flag == bad
        got = vd.cpu().numpy()
        if bad:
            assert np.array_equal(got, v)
        else:
            assert (np.abs(got - want) <= 4 * EPS * np.abs(want)).all()


@pytest.mark.parametrize("name", CLOSED)
def test_filter_laplacian_with_constraint(cuda_device, name):
    v, f = O.FIXTURES[name]()
    m = M.filter_laplacian(_mesh(name), lamb=0.5, iterations=3, volume_constraint=True, backend="hip")
    _close(m.vertices, O.filter_laplacian(v, f, 0.5, 3, True), v)
    assert m.vertex_normals is None


@pytest.mark.parametrize("name", NAMES)
def test_filter_taubin(cuda_device, name):
    v, f = O.FIXTURES[name]()
    m = M.filter_taubin(_mesh(name), iterations=10, backend="hip")
    want = O.filter_taubin(v, f, 0.5, 0.5, 10)
    _close(m.vertices, want, v)
    assert np.array_equal(m.vertices, want)      # no cbrt on this path: the same bits


@pytest.mark.parametrize("name", NAMES)
def test_filter_laplacian_without_constraint_is_bit_equal(cuda_device, name):
    v, f = O.FIXTURES[name]()
    m = _mesh(name)
    m.vertex_colors = np.zeros((len(v), 3), np.uint8)
    m.vertex_normals = np.ones((len(v), 3))
    assert M.filter_laplacian(m, lamb=0.5, iterations=3, volume_constraint=False, backend="hip") is m
    assert np.array_equal(m.vertices, O.filter_laplacian(v, f, 0.5, 3, False))
    assert m.vertex_normals is None and m.vertex_colors is not None and np.array_equal(m.faces, f)
    same = _mesh(name)
    assert np.array_equal(M.filter_laplacian(same, iterations=0, backend="hip").vertices, v)


def test_volume_is_kept_on_the_sphere(cuda_device):
    v, f = O.bumpy_sphere()
    vol0 = O.volume(v, f)
    m = M.filter_laplacian(_mesh("bumpy_sphere"), iterations=3, volume_constraint=True, backend="hip")
    rel = abs(O.volume(m.vertices, f) - vol0) / vol0
    print(f"relative volume change: {rel:.3e}")
    assert rel <= 1e-12


def test_non_positive_volume_raises_and_leaves_the_mesh(cuda_device):
    v, f = O.bumpy_sphere()
    for mesh in (M.Mesh(v.copy(), f[:, [0, 2, 1]].copy()), _mesh("grid_patch")):
        before = mesh.vertices.copy()
        mesh.vertex_normals = np.ones_like(before)
        assert M.mesh_volume(mesh, backend="hip") < 0
        with pytest.raises(ValueError, match="volume_constraint needs a closed, outward-oriented mesh"):
            M.filter_laplacian(mesh, iterations=3, volume_constraint=True, backend="hip")
        assert np.array_equal(mesh.vertices, before) and mesh.vertex_normals is not None


@pytest.mark.parametrize("name", NAMES)
def test_vertex_normals(cuda_device, name):
    """The sums before normalisation are bit-equal by construction (fixed order, no contraction); they
    are checked through the normalised result: s / len with IEEE sqrt and division is what numpy
    computes too, and if the device's sqrt or division rounded differently each component would move
    by at most 3 * 2^-53 of a unit vector, so 4 * 2^-53 per component is asserted. On the MI355X the
    result was bit-equal on every fixture."""
    v, f = O.FIXTURES[name]()
    m = _mesh(name)
    got = m.compute_vertex_normals(backend="hip")
    assert got is m.vertex_normals and got.shape == (len(v), 3)
    want = O.vertex_normals(v, f, *O.vertex_faces(f, len(v)))
    err = float(np.abs(got - want).max())
    print(f"max |normal - oracle| = {err:.3e}; bit-equal: {np.array_equal(got, want)}")
    assert err <= 4 * EPS
    host = _mesh(name).compute_vertex_normals(backend="scipy")
    assert np.abs(got - host).max() <= 4 * EPS
    if name == "tetrahedron_plus":
        assert np.array_equal(got[4], np.zeros(3))
    if name == "bumpy_sphere":
        assert (np.sum(got * v, axis=1) > 0).all()


def test_entry_points_refuse_bad_arguments(cuda_device):
    L = _lib.lib()
    t = torch.zeros(12, dtype=torch.float64, device=cuda_device)
    i = torch.zeros(8, dtype=torch.int32, device=cuda_device)
    p, st = _lib.ptr, _lib.stream_of(t)
    assert L.nof_mesh_laplacian_step(p(t), p(i), p(i), 4, 0.5, p(t), st) != 0
    assert b"distinct" in L.nof_last_error()
    assert L.nof_mesh_laplacian_step(p(t), p(i), p(i), -1, 0.5, p(t[6:]), st) != 0
    assert L.nof_mesh_laplacian_step(p(t), p(i), p(i), 2, float("nan"), p(t[6:]), st) != 0
    assert L.nof_mesh_volume(p(t), p(i), 1 << 30, p(t), p(t), st) != 0
    assert L.nof_mesh_volume(p(t), p(i), 1, None, p(t), st) != 0
    assert L.nof_mesh_scale_to_volume(p(t), 4, p(t), p(t), None, st) != 0
    assert L.nof_mesh_vertex_normals(p(t), p(i), p(i), p(i), 4, None, st) != 0
    torch.cuda.synchronize()


def test_postprocess_mesh_hip_matches_scipy(cuda_device, tmp_path):
    v, f = O.bumpy_sphere()
    tv, tf = O.tetrahedron()
    sc, tr = 2.5, np.array([0.1, -0.2, 0.3])
    both = M.Mesh(np.concatenate([(v + tr) * sc, (tv * 0.01 + 3.0 + tr) * sc]), np.concatenate([f, tf + len(v)]))
    a = M.postprocess_mesh(both, tr, sc, out_dir=str(tmp_path), min_edge=100, backend="hip")
    b = M.postprocess_mesh(both, tr, sc, min_edge=100, backend="scipy")
    for key in ("real_scale", "biggest_component", "smoothed"):
        assert np.array_equal(a[key].faces, b[key].faces)
        _close(a[key].vertices, b[key].vertices, b[key].vertices)
    assert len(a["smoothed"].vertices) == len(v)
    assert np.abs(a["smoothed"].vertex_normals - b["smoothed"].vertex_normals).max() <= 1e-9
    assert (tmp_path / "mesh_biggest_component_smoothed.obj").stat().st_size > 0
