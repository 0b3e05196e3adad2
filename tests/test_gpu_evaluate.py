"""GPU: bundlesdf_amd.evaluate against tests/nearest_oracle.py. `nearest` is compared exactly — indices
equal and distances equal as float64 bits, over every query — on the seeded cases whose fairness
tests/test_evaluate_cpu.py checks; the metrics, the correspondence sums, the ICP, the surface sampler
and the mesh leg are held to bounds derived in each test."""
import functools
import math

import numpy as np
import pytest
import torch

from bundlesdf_amd import evaluate as E
from bundlesdf_amd import mesh as M
from tests import nearest_oracle as O

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", O.CASES)
def test_nearest_is_exact(cuda_device, name):
    c = O.case(name)
    want_d, want_i = O.expected(name)
    grid = E.PointGrid(c["cloud"], cell=c["cell"], device=cuda_device)
    dist, index = E.nearest(c["queries"], grid, transforms=c["T"], max_dist=c["max_dist"])
    assert dist.dtype == torch.float64 and index.dtype == torch.int32 and dist.is_cuda and index.is_cuda
    assert tuple(dist.shape) == want_d.shape == tuple(index.shape)
    got_d, got_i = dist.cpu().numpy(), index.cpu().numpy()
    print(name, "dims", grid.dims.tolist(), "cell", grid.cell, "index mismatches", int((got_i != want_i).sum()),
          "dist mismatches", int((_bits(got_d) != _bits(want_d)).sum()))
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d))
    if name == "n3000_tiny_cell":
        assert int(np.prod(grid.dims)) > 100 * len(c["cloud"])       # many empty rings
    if name == "n3000_huge_cell":
        assert grid.dims.tolist() == [1, 1, 1]
    if name == "planar":
        assert grid.dims[1] == 1 and grid.dims[0] > 1 and grid.dims[2] > 1
    if name == "duplicates":
        assert (got_i[:100] == want_i[:100]).all() and len(np.unique(got_i[:100])) == 1
    if name == "max_dist":
        assert 0.4 < (got_i < 0).mean() < 0.6 and np.isinf(got_d[got_i < 0]).all()


def test_nearest_takes_points_and_a_single_transform(cuda_device):
    """A raw cloud (the grid is built inside), device tensors as input, and one 4x4 -> [Q]."""
    c = O.case("batched")
    T = c["T"][2]
    want_d, want_i = O.nearest(c["queries"], c["cloud"], T)
    dist, index = E.nearest(torch.from_numpy(c["queries"]).to(cuda_device), torch.from_numpy(c["cloud"]).to(cuda_device),
                            transforms=T)
    assert tuple(dist.shape) == (len(c["queries"]),)
    assert np.array_equal(index.cpu().numpy(), want_i) and np.array_equal(_bits(dist.cpu().numpy()), _bits(want_d))
    with pytest.raises(ValueError, match="empty"):
        E.PointGrid(np.zeros((0, 3)), device=cuda_device)
    d0, i0 = E.nearest(np.zeros((0, 3)), c["cloud"])
    assert tuple(d0.shape) == (0,) and tuple(i0.shape) == (0,)


def test_point_grid_cell_rules(cuda_device):
    cloud = O.case("n3000")["cloud"]
    g = E.PointGrid(cloud, device=cuda_device)
    ext = cloud.max(0) - cloud.min(0)
    assert g.cell == pytest.approx(2 * (np.prod(ext) / 3000) ** (1 / 3), rel=1e-12)
    g = E.PointGrid(cloud, cell=1e-4, device=cuda_device)          # 2e4^3 cells asked for: the edge grows
    assert g.cell > 1e-4 and (1 << 21) < int(np.prod(g.dims)) <= (1 << 24)
    ids = g.cell_ids.cpu().numpy()
    assert np.array_equal(np.sort(ids), np.arange(3000))
    assert np.array_equal(g.cell_points.cpu().numpy(), cloud[ids])


@functools.lru_cache(maxsize=None)
def _pose_case():
    rng = np.random.default_rng(30)
    model = rng.uniform(-0.12, 0.12, (700, 3))
    gt = np.stack([O.rigid(rng.normal(0, 1, 3), rng.uniform(-0.5, 0.5, 3) + [0, 0, 0.8]) for _ in range(5)])
    pred = np.stack([g @ O.rigid(rng.normal(0, 0.15, 3), rng.normal(0, 0.02, 3)) for g in gt])
    return model, pred, gt


def test_adi_and_add_match_the_reference_formulation(cuda_device):
    """The oracle transforms both clouds and searches gt in pred, as the reference; the device searches
    inv(pred) gt m in the model. Bound: 1e-12 * max(1, max |coordinate|) — a rigid transform in f64
    rounds by a few tens of ulps of the coordinate magnitude (about 1e-14 at 1 m) and the factor 100
    covers the host-side inverse."""
    model, pred, gt = _pose_case()
    coord = max(np.abs(O._homo(T, model)).max() for T in list(pred) + list(gt))
    tol = 1e-12 * max(1.0, coord)
    want_s = np.array([O.adds(p, g, model) for p, g in zip(pred, gt)])
    want_a = np.array([O.add(p, g, model) for p, g in zip(pred, gt)])
    got_s, got_a = E.adi_err(pred, gt, model), E.add_err(pred, gt, model)
    print("ADD-S err", np.abs(got_s - want_s).max(), "ADD err", np.abs(got_a - want_a).max(), "tol", tol)
    assert got_s.shape == (5,) and got_s.dtype == np.float64 and got_a.shape == (5,)
    assert np.abs(got_s - want_s).max() <= tol
    assert np.abs(got_a - want_a).max() <= tol
    assert (want_s > 1e-3).all() and (want_a > want_s).all()          # the case is not degenerate
    one_s, one_a = E.adi_err(pred[3], gt[3], model), E.add_err(pred[3], gt[3], model)
    assert isinstance(one_s, float) and isinstance(one_a, float)
    assert abs(one_s - want_s[3]) <= tol and abs(one_a - want_a[3]) <= tol


def test_evaluate_poses(cuda_device):
    model, pred, gt = _pose_case()
    off = O.rigid([0.2, 0.1, -0.4], [0.3, -0.1, 0.2])      # the prediction lives in another object frame
    out = E.evaluate_poses(pred @ off, gt, model)
    al = pred @ np.linalg.inv(pred[0]) @ gt[0]
    want_s = np.array([O.adds(p, g, model) for p, g in zip(al, gt)])
    want_a = np.array([O.add(p, g, model) for p, g in zip(al, gt)])
    np.testing.assert_allclose(out["ADDS"], want_s, rtol=0, atol=1e-11)
    np.testing.assert_allclose(out["ADD"], want_a, rtol=0, atol=1e-11)
    assert out["ADD"][0] <= 1e-11 and out["ADDS"][0] <= 1e-11        # frame 0 is aligned onto the ground truth
    assert out["ADDS_AUC"] == pytest.approx(E.compute_auc(want_s) * 100, abs=1e-8)
    assert out["ADD_AUC"] == pytest.approx(E.compute_auc(want_a) * 100, abs=1e-8)
    assert 0 < out["ADD_AUC"] <= out["ADDS_AUC"] <= 100


def test_chamfer_matches_oracle(cuda_device):
    a, b = O.case("n3000")["cloud"], O.case("n3000")["queries"]
    want = O.chamfer(a, b)
    got = E.chamfer_distance_between_clouds_mutual(a, b)
    print("chamfer", got, want, abs(got - want) / want)
    assert abs(got - want) <= 1e-13 * want          # a mean of exact distances: only the summation order differs
    assert got == E.chamfer_distance_between_clouds_mutual(b, a)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_correspondence_moments(cuda_device, n):
    """Two runs give the same bits; each sum is within n * 2^-52 * sum |term| of math.fsum (any order
    of n additions errs by at most (n - 1) ulp-halves of the running magnitude)."""
    rng = np.random.default_rng(40 + n)
    src, tgt = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (300, 3))
    T = O.rigid(rng.normal(0, 0.4, 3), rng.normal(0, 0.1, 3))
    index = rng.integers(0, 300, n).astype(np.int32)
    if n > 1:
        index[rng.random(n) < 0.3] = -1
    dist = rng.uniform(0, 0.5, n)
    dev = [torch.from_numpy(x).to(cuda_device) for x in (src, tgt, index, dist)]
    got = E.correspondence_moments(*dev, transform=T)
    again = E.correspondence_moments(*dev, transform=T)
    assert np.array_equal(_bits(got), _bits(again))
    want, mag = O.moments(src, T, tgt, index, dist)
    print(n, "worst err / bound", (np.abs(got - want) / np.maximum(n * 2.0 ** -52 * mag, 1e-300)).max())
    assert got[0] == (index >= 0).sum()
    assert (np.abs(got - want) <= n * 2.0 ** -52 * mag).all()
    ident, ident_mag = O.moments(src, None, tgt, index, dist)           # no transform: the identity
    assert (np.abs(E.correspondence_moments(*dev) - ident) <= n * 2.0 ** -52 * ident_mag).all()


def test_icp_recovers_a_known_offset(cuda_device):
    """A 2000-point cloud and its copy moved by 3 degrees and 5 mm: noise-free, so the truth is a fixed
    point; Kabsch in f64 leaves about 1e-13 and the 1e-9 margin covers stopping on the relative
    thresholds."""
    tgt = np.random.default_rng(20).uniform(-0.1, 0.1, (2000, 3))
    axis = np.array([1.0, 2.0, -1.5])
    t = np.array([0.003, -0.0035, 0.002])
    truth = O.rigid(axis / np.linalg.norm(axis) * np.deg2rad(3.0), t * (0.005 / np.linalg.norm(t)))
    src = O.transform(np.linalg.inv(truth), tgt)
    r = E.icp_point_to_point(src, tgt, 0.02)
    print("icp", r["iterations"], r["fitness"], r["inlier_rmse"], np.abs(r["transformation"] - truth).max())
    assert np.abs(r["transformation"] - truth).max() <= 1e-9
    assert r["fitness"] == 1.0
    assert 1 <= r["iterations"] <= 30 and r["inlier_rmse"] <= 1e-9
    again = E.icp_point_to_point(src, tgt, 0.02)
    assert np.array_equal(_bits(again["transformation"]), _bits(r["transformation"]))
    assert again["inlier_rmse"] == r["inlier_rmse"] and again["iterations"] == r["iterations"]
    none = E.icp_point_to_point(src + 5.0, tgt, 0.02)                  # nothing within reach: no update
    assert none["fitness"] == 0.0 and none["iterations"] == 0 and np.array_equal(none["transformation"], np.eye(4))


def test_sample_surface(cuda_device):
    """Two triangles with areas 3 : 1 in different planes; 40 000 samples."""
    V = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0],            # area 3, plane z = 0
                  [5, 0, 0], [5, 1, 0], [5, 0, 2.0]])         # area 1, plane x = 5
    mesh = M.Mesh(V, np.array([[0, 1, 2], [3, 4, 5]]))
    pts, face = E.sample_surface(mesh, 40000, seed=3, device=cuda_device)
    assert tuple(pts.shape) == (40000, 3) and pts.dtype == torch.float64 and pts.is_cuda
    p, f = pts.cpu().numpy(), face.cpu().numpy()
    share = (f == 0).mean()
    print("share on the large triangle", share)
    assert abs(share - 0.75) <= 5 * math.sqrt(0.75 * 0.25 / 40000)
    for k in (0, 1):
        a, b, c = V[mesh.faces[k]]
        q = p[f == k] - a
        # barycentric coordinates by least squares; coordinates are O(1), so 1e-12 is thousands of ulps
        uv, res = np.linalg.lstsq(np.stack([b - a, c - a], 1), q.T, rcond=None)[:2]
        n = np.cross(b - a, c - a)
        assert np.abs(q @ n / np.linalg.norm(n)).max() <= 1e-12            # in the plane
        assert (uv >= -1e-12).all() and (uv.sum(0) <= 1 + 1e-12).all()    # inside the triangle
        # and spread over it: the mean barycentric coordinate of a uniform sample is 1/3 (sd 0.236 / sqrt(n))
        assert np.abs(uv.mean(1) - 1 / 3).max() <= 5 * 0.236 / math.sqrt(len(q))
    pts2, face2 = E.sample_surface(mesh, 40000, seed=3, device=cuda_device)
    assert torch.equal(pts, pts2) and torch.equal(face, face2)
    pts3, _ = E.sample_surface(mesh, 40000, seed=4, device=cuda_device)
    assert not torch.equal(pts, pts3)


def test_evaluate_mesh_on_a_sphere(cuda_device):
    """A marching-cubes sphere (radius 0.08 m at the origin) with a small blob 0.25 m away, against points
    on the analytic sphere."""
    voxel = 0.005
    ax = np.arange(-0.1, 0.3 + 1e-9, voxel)
    X, Y, Z = np.meshgrid(ax, ax[:41], ax[:41], indexing="ij")
    sdf = np.minimum(np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.08, np.sqrt((X - 0.25) ** 2 + Y ** 2 + Z ** 2) - 0.02)
    v, f = M.marching_cubes(torch.from_numpy(sdf.astype(np.float32)).to(cuda_device), 0.0, backend="hip")
    mesh = M.Mesh(v * voxel + ax[0], f)
    blob = mesh.vertices[:, 0] > 0.15
    n_sphere = len(np.unique(mesh.vertices[~blob], axis=0))
    assert blob.sum() > 50 and n_sphere > 1000
    g = np.random.default_rng(50).normal(size=(20000, 3))
    gt = 0.08 * g / np.linalg.norm(g, axis=1, keepdims=True)
    out = E.evaluate_mesh(mesh, gt, voxel=voxel, n_samples=30000, seed=1, backend="hip")
    print("chamfer cm", out["chamfer_cm"], "icp", out["icp"]["fitness"], out["icp"]["inlier_rmse"],
          out["icp"]["iterations"])
    kept = out["component"]
    assert len(kept.vertices) == n_sphere and kept.vertices[:, 0].max() < 0.1     # the blob is gone
    assert math.isfinite(out["chamfer_cm"]) and out["chamfer_cm"] / 100 < voxel
    assert out["icp"]["fitness"] > 0.99
    ref = E.evaluate_mesh(mesh, gt, voxel=voxel, n_samples=30000, seed=1, backend="scipy")
    assert np.array_equal(ref["component"].vertices, kept.vertices)
    assert np.array_equal(ref["component"].faces, kept.faces)
    assert ref["chamfer_cm"] == out["chamfer_cm"]
    assert len(mesh.vertices) == len(v)                                  # the input mesh is untouched
