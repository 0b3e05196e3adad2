"""GPU: the HIP mesher (nof_marching_cubes_count / _emit -> mesh.marching_cubes_device) and the HIP
component labelling (nof_mesh_components -> mesh.component_labels) against the code they must
reproduce: mesh.marching_cubes(backend="torch") run on the CPU, and scipy's connected_components.
Every comparison is exact (vertices as float32 bits) and over all vertices and faces."""
import functools
import os

import numpy as np
import pytest
import torch

from bundlesdf_amd import mesh as M

pytestmark = pytest.mark.gpu


def _noise(shape, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(key, level=0.0):
    """(volume, CPU torch-backend vertices, faces) of a named volume; shared, never modified."""
    vol = _VOLUMES[key]()
    v, f = M.marching_cubes(torch.from_numpy(vol), level, backend="torch")
    return vol, v, f


def _bumpy_sphere():
    ax = np.linspace(-1, 1, 48)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.6 + 0.15 * np.sin(7 * X) * np.sin(7 * Y) * np.sin(7 * Z)).astype(np.float32)


def _two_spheres():
    xs = np.linspace(-1, 1, 40)
    X, Y, Z = np.meshgrid(xs, xs, xs, indexing="ij")
    big = np.sqrt((X + 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.45
    small = np.sqrt((X - 0.6) ** 2 + Y ** 2 + Z ** 2) - 0.2
    return np.minimum(big, small)      # float64, as test_split_and_largest_component passes it


def _plane_at_level():
    """Noise with the whole plane j = 4 exactly at the level 0.25, and a second plane of exact zeros."""
    vol = _noise((9, 10, 11), seed=3)
    vol[6, :, :] = 0.0
    vol[:, 4, :] = 0.25
    return vol


def _ends_at_level():
    """Every second point along k holds the level itself and its neighbours are below it: on those
    crossing edges v0 == level (t = 0) or v1 == level (t = 1)."""
    vol = -np.abs(_noise((6, 7, 12), seed=4)) - 0.1
    vol[:, :, ::2] = 0.0
    vol[3:, :, :] = np.abs(vol[3:, :, :]) + 0.5    # and an ordinary crossing between i = 2 and i = 3
    vol[3:, :, 1::2] = 0.0
    return vol.astype(np.float32)


_VOLUMES = {"noise24": lambda: _noise((24, 24, 24)), "noise_7_9_33": lambda: _noise((7, 9, 33)),
            "noise_40_37_70": lambda: _noise((40, 37, 70)), "bumpy48": _bumpy_sphere, "two_spheres": _two_spheres,
            "plane_at_level": _plane_at_level, "ends_at_level": _ends_at_level}


def _assert_same_mesh(got, want):
    (gv, gf), (wv, wf) = got, want
    assert gv.shape == wv.shape and gf.shape == wf.shape, (gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(np.asarray(gv, np.float32).view(np.uint32), np.asarray(wv, np.float32).view(np.uint32))
    assert np.array_equal(np.asarray(gv, np.float64), np.asarray(wv, np.float64))   # float32 values, widened
    assert np.array_equal(gf, wf)


def _check(key, level, dev):
    vol, v, f = _oracle(key, level)
    assert len(v) > 0 and len(f) > 0
    dv, df = M.marching_cubes_device(torch.from_numpy(vol).to(dev), level)
    assert dv.is_cuda and df.is_cuda and dv.dtype == torch.float32 and df.dtype == torch.int32
    _assert_same_mesh((dv.cpu().numpy(), df.cpu().numpy().astype(np.int64)), (v, f))
    gv, gf = M.marching_cubes(vol, level, backend="hip")        # the numpy surface: float64 / int64 as today
    assert gv.dtype == v.dtype == np.float64 and gf.dtype == f.dtype == np.int64
    _assert_same_mesh((gv, gf), (v, f))
    return v, f


def test_all_256_cases(cuda_device):
    vol, v, f = _oracle("noise24")
    inside = vol < 0
    case = np.zeros((23, 23, 23), np.int64)
    for c in range(8):
        dx, dy, dz = M._CORNERS[c]
        case |= inside[dx:23 + dx, dy:23 + dy, dz:23 + dz].astype(np.int64) << c
    assert len(np.unique(case)) == 256
    assert (len(v), len(f)) == (20016, 39273)
    _check("noise24", 0.0, cuda_device)


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("key", ["noise_7_9_33", "noise_40_37_70"])
def test_non_cubic_block_straddling(cuda_device, key, level):
    """(40, 37, 70) is 103,600 points: 405 blocks, rows that are no multiple of the wave, a multi-block
    scan. The CPU oracle gives 2,842 vertices / 4,996 faces for (7, 9, 33) at level 0 (generator seed 0)."""
    v, f = _check(key, level, cuda_device)
    assert len(v) > 2000 and len(f) > 4000


def test_values_equal_to_level(cuda_device):
    vol, v, f = _oracle("plane_at_level", 0.25)
    assert (vol == 0.25).sum() >= 9 * 11
    _check("plane_at_level", 0.25, cuda_device)
    _check("plane_at_level", 0.0, cuda_device)
    vol, v, f = _oracle("ends_at_level", 0.0)
    frac = v - np.floor(v)
    assert (frac == 0).all(1).sum() > 100          # vertices that sit on a grid point: t was 0 or 1
    _check("ends_at_level", 0.0, cuda_device)


def test_smooth_field_closed_surface(cuda_device):
    _check("bumpy48", 0.0, cuda_device)
    v, f = M.marching_cubes(_oracle("bumpy48")[0], 0.0, backend="hip")
    assert len(f) > 1000
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    assert (cnt == 2).all()
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    assert (dcnt == 1).all()
    P = v * (2.0 / 47) - 1
    n = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
    assert (np.sum(n * P[f].mean(1), 1) > 0).mean() > 0.99


def test_level_outside_range_and_smallest_volume(cuda_device):
    vol = np.abs(_noise((5, 6, 7))) + 0.5
    for level in (0.0, 2.0):
        with pytest.raises(ValueError) as cpu:
            M.marching_cubes(vol, level, backend="torch")
        with pytest.raises(ValueError) as hip:
            M.marching_cubes(vol, level, backend="hip")
        assert str(hip.value) == str(cpu.value) == "Surface level must be within volume data range."
    one = np.ones((2, 2, 2), np.float32)
    one[1, 0, 1] = -1.0
    want = M.marching_cubes(one, 0.0, backend="torch")
    got = M.marching_cubes(one, 0.0, backend="hip")
    assert got[0].shape == (3, 3) and got[1].shape == (1, 3)
    _assert_same_mesh(got, want)
    # the level inside the range, no edge crossed (every value equal to the level: nothing is below it)
    flat = np.zeros((3, 4, 5), np.float32)
    want = M.marching_cubes(flat, 0.0, backend="torch")
    got = M.marching_cubes(flat, 0.0, backend="hip")
    assert got[0].shape == want[0].shape == (0, 3) and got[1].shape == want[1].shape == (0, 3)
    assert got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype


# ---------------------------------------------------------------- components
def _scipy_labels(faces, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.asarray(faces)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)
    return connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)[1]


def _reversed_strip(n_tri=300):
    """A strip of n_tri triangles (t, t + 1, t + 2) numbered from the far end, plus two loose vertices."""
    n = n_tri + 2
    t = np.arange(n_tri)
    faces = (n - 1) - np.stack([t, t + 1, t + 2], 1)
    verts = np.stack([np.arange(n + 2) * 0.5, (np.arange(n + 2) % 2).astype(float), np.zeros(n + 2)], 1)
    return verts, faces


def _component_meshes():
    _, v, f = _oracle("two_spheres")
    yield "two_spheres", v, f, 2
    _, v, f = _oracle("noise24")
    yield "noise24", v, f, 169
    v, f = _reversed_strip()
    yield "strip", v, f, 3


def _same_parts(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert np.array_equal(p.vertices, q.vertices) and np.array_equal(p.faces, q.faces)
        for name in ("vertex_colors", "vertex_normals", "vertex_color_counts"):
            assert np.array_equal(getattr(p, name), getattr(q, name)), name


def test_components_match_scipy(cuda_device):
    for name, v, f, n_comp in _component_meshes():
        n = len(v)
        want = _scipy_labels(f, n)
        assert want.max() + 1 == n_comp, (name, want.max() + 1)
        lab = M.component_labels(f, n)
        assert lab.is_cuda and lab.dtype == torch.int32 and lab.shape == (n,)
        lab = lab.cpu().numpy()
        roots, rank = np.unique(lab, return_inverse=True)
        assert np.array_equal(rank.reshape(-1), want), name
        assert np.array_equal(roots, [np.flatnonzero(want == c)[0] for c in range(n_comp)]), name   # the lowest vertex
        if name == "noise24":
            assert np.bincount(want).max() == 18860
        rng = np.random.default_rng(5)
        mesh = M.Mesh(v, f)
        mesh.vertex_colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        mesh.vertex_normals = rng.normal(size=(n, 3))
        mesh.vertex_color_counts = rng.integers(0, 9, n).astype(np.int32)
        for min_edge in (10, 1000):
            ref = M.trimesh_split(mesh, min_edge=min_edge, backend="scipy")
            got = M.trimesh_split(mesh, min_edge=min_edge, backend="hip")
            assert len(ref) == int((np.bincount(want) >= min_edge).sum())
            _same_parts(got, ref)
        ref, got = M.largest_component(mesh.copy(), backend="scipy"), M.largest_component(mesh.copy(), backend="hip")
        assert (ref is None) == (got is None)
        if ref is not None:
            _same_parts([got], [ref])
    # a mesh without faces, and a corner outside the mesh
    assert np.array_equal(M.component_labels(np.zeros((0, 3), np.int64), 5).cpu().numpy(), np.arange(5))
    with pytest.raises(ValueError):
        M.component_labels(np.array([[0, 1, 5]]), 5)


# ---------------------------------------------------------------- NerfRunner
@functools.lru_cache(maxsize=None)
def _trained():
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(3, seed=1)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=60, N_rand=1024,
                         num_levels=16, amp=True, mesh_resolution=0.006)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    return nr


def test_runner_extract_mesh_hip_equals_torch(cuda_device, tmp_path):
    nr = _trained()
    want = nr.extract_mesh(voxel_size=0.006)
    got = nr.extract_mesh(voxel_size=0.006, mesher="hip")
    assert want is not None and len(want.faces) > 100
    assert got.vertices.dtype == want.vertices.dtype and got.faces.dtype == want.faces.dtype
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.faces, want.faces)
    assert np.array_equal(nr.extract_mesh(voxel_size=0.006, mesher="torch").faces, want.faces)
    with pytest.raises(ValueError):
        nr.extract_mesh(voxel_size=0.006, mesher="bogus")
    m, sigma, q = nr.extract_mesh(voxel_size=0.008, return_sigma=True, mesher="hip")
    m0, sigma0, q0 = nr.extract_mesh(voxel_size=0.008, return_sigma=True)
    assert np.array_equal(m.vertices, m0.vertices) and np.array_equal(m.faces, m0.faces)
    assert np.array_equal(sigma, sigma0) and torch.equal(q, q0) and sigma.ndim == 3
    # the i_mesh hook (train() calls _hook_mesh; called here on one field, since two trainings differ in
    # their low bits) follows cfg['mesh_extractor']: the same two files, byte for byte
    files = {}
    try:
        for mesher in ("torch", "hip", None):
            d = tmp_path / str(mesher)
            os.makedirs(d)
            nr.cfg["save_dir"] = str(d)
            if mesher is None:
                nr.cfg.pop("mesh_extractor")
            else:
                nr.cfg["mesh_extractor"] = mesher
            nr._hook_mesh()
            names = sorted(os.listdir(d))
            g = nr.global_step
            assert names == [f"step_{g:07d}_mesh_normalized_space.obj", f"step_{g:07d}_mesh_real_world.obj"]
            files[mesher] = [open(d / n, "rb").read() for n in names]
            assert all(len(b) > 1000 for b in files[mesher])
    finally:
        nr.cfg.pop("mesh_extractor", None)
        nr.cfg.pop("save_dir", None)
    assert files["hip"] == files["torch"] == files[None]


def test_extraction_leaves_the_training_state_alone(cuda_device):
    """A captured training step after extract_mesh(mesher="hip") gives the loss it gives without the
    extraction: the step is replayed from the same restored state both times (its loss terms are a forward
    from that state, summed in a fixed order), and the extraction changes no tensor of the trainer."""
    nr = _trained()
    fs = nr.trainer
    ids = torch.arange(512, dtype=torch.int32, device=cuda_device)
    fs.graph_step_ids(ids)
    torch.cuda.synchronize()
    snap = {k: v.clone() for k, v in vars(fs).items() if torch.is_tensor(v)}
    graphs, step = fs._graphs, fs.global_step
    host = {k: v for k, v in vars(fs).items() if isinstance(v, (int, float, bool))}

    def restore():
        for k, v in snap.items():
            getattr(fs, k).copy_(v)
        for k, v in host.items():
            setattr(fs, k, v)
        torch.cuda.synchronize()

    plain = fs.graph_step_ids(ids)["loss_terms"].clone()
    restore()
    again = fs.graph_step_ids(ids)["loss_terms"].clone()
    assert torch.equal(again[:6], plain[:6])            # the restored state replays to the same bits
    restore()
    mesh = nr.extract_mesh(voxel_size=0.006, mesher="hip")
    parts = M.trimesh_split(mesh, min_edge=10, backend="hip")
    torch.cuda.synchronize()
    assert mesh is not None and len(mesh.faces) > 100 and len(parts) >= 1
    for k, v in snap.items():
        # frags / bias are the packed copy of the MLP in P: query_sdf repacks them from the current P (either
        # mesher), and every step's prologue repacks them before it reads them
        assert k in ("frags", "bias") or torch.equal(getattr(fs, k), v), k
    assert fs._graphs is graphs and fs.global_step == step
    after = fs.graph_step_ids(ids)["loss_terms"].clone()
    assert fs._graphs is graphs
    assert torch.isfinite(after[:4]).all() and torch.equal(after[:6], plain[:6])
