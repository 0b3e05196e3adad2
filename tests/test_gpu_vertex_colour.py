"""GPU: nof_vertex_color_accumulate and NerfRunner.mesh_vertex_color_from_train_images against the
restatements of tests/vertex_colour_oracle.py: the brute-force one (no search window) bit for bit —
nearest pixel, distance, f64 sums, counts — and the reference's cKDTree lines in the final uint8
colours. Fixture: the 20^3 marching-cubes sphere (840 vertices) seen by three 64x48 cameras, one of
them near (windows up to ~12 pixels at radius 0.06, clipped by the image border), a 90 % mask."""
import json
import os

import numpy as np
import pytest
import torch

from tests import vertex_colour_oracle as VC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PARITY = {}


def _record(key, **figures):
    _PARITY[key] = {k: float(v) for k, v in figures.items()}
    print(key, _PARITY[key])
    if os.environ.get("NOF_WRITE_PARITY"):
        path = os.path.join(ROOT, os.environ["NOF_WRITE_PARITY"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _dev(a, dtype, dev):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)   # a copy: the fixture is read-only


class _Device:
    """One frame's arrays on the device and the accumulators of a vertex set."""

    def __init__(self, dev, V):
        self.dev = dev
        self.V = _dev(V, np.float32, dev).reshape(-1, 3)
        n = len(self.V)
        self.sum = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.nearest = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.dist = torch.full((n,), -7.0, dtype=torch.float64, device=dev)

    def frame(self, zbuf, mask, colors, cam_in_ob, ob_in_cam, radius, min_depth=VC.MIN_DEPTH, H=VC.H, W=VC.W):
        from bundlesdf_amd import _lib
        zb = _dev(np.asarray(zbuf).view(np.int64), np.int64, self.dev)
        m = _dev(mask, np.uint8, self.dev).reshape(-1)
        col = _dev(colors, np.float32, self.dev)
        c, o = np.ascontiguousarray(cam_in_ob, np.float64), np.ascontiguousarray(ob_in_cam, np.float64)
        _lib.check(_lib.lib().nof_vertex_color_accumulate(
            _lib.ptr(zb), H, W, _lib.ptr(m), min_depth, _lib.ptr(col), c.ctypes.data_as(_lib._p),
            o.ctypes.data_as(_lib._p), VC.K.ctypes.data_as(_lib._p), _lib.ptr(self.V) if len(self.V) else None,
            len(self.V), radius, _lib.ptr(self.sum), _lib.ptr(self.count), _lib.ptr(self.nearest), _lib.ptr(self.dist),
            _lib.stream_of(self.sum)), "vertex_color_accumulate")
        torch.cuda.synchronize()
        return self.nearest.cpu().numpy(), self.dist.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("radius", VC.RADII)
def test_three_frames_match_brute_force_and_kdtree(cuda_device, radius):
    from bundlesdf_amd import _lib
    fx, ref = VC.fixture(), VC.fixture_reference(radius)
    d = _Device(cuda_device, fx["V"])
    Fc = torch.as_tensor(fx["mesh"].faces, device=cuda_device)
    for fr, (bn, bd) in zip(fx["frames"], ref["brute"]):
        # the z-buffer the product would search is the oracle's, bit for bit
        zb = torch.empty(VC.H * VC.W, dtype=torch.int64, device=cuda_device)
        _lib.check(_lib.lib().nof_raster_faces(_lib.ptr(d.V), _lib.ptr(Fc), len(Fc),
                                               fr["ob_in_cam"].ctypes.data_as(_lib._p), VC.K.ctypes.data_as(_lib._p),
                                               VC.H, VC.W, 0.1, VC.ZFAR, _lib.ptr(zb), _lib.stream_of(zb)))
        assert np.array_equal(zb.cpu().numpy().view(np.uint64), fr["zbuf"])
        near, dist = d.frame(zb.cpu().numpy(), fr["mask"], fr["colors"], fr["cam_in_ob"], fr["ob_in_cam"], radius)
        assert np.array_equal(near, bn)
        assert _same_bits(dist, bd)
    count = d.count.cpu().numpy()
    assert _same_bits(d.sum.cpu().numpy(), ref["brute_sum"])
    assert np.array_equal(count, ref["brute_count"])
    assert np.array_equal(count, ref["kdtree_count"])
    assert np.array_equal(VC.finish(d.sum.cpu().numpy(), count), ref["kdtree_rgb"])
    share, multi = np.mean(count > 0), np.mean(count > 1)
    _record(f"fixture/radius{radius}", coloured_share=share, multi_frame_share=multi)
    assert 0.25 <= share <= 0.8 and multi >= 0.05   # accept, reject and the multi-frame mean all taken


def test_product_loop_matches_kdtree(cuda_device):
    """texture.vertex_colors_from_images (raster + accumulate per frame, final divide) on the fixture."""
    from bundlesdf_amd.texture import vertex_colors_from_images
    fx, ref = VC.fixture(), VC.fixture_reference(0.02)
    fr = fx["frames"]
    rgb, count = vertex_colors_from_images(fx["mesh"].vertices, fx["mesh"].faces,
                                           [f["colors"].reshape(VC.H, VC.W, 3).copy() for f in fr],
                                           [f["mask"].copy() for f in fr], [f["cam_in_ob"] for f in fr], VC.K, VC.H, VC.W,
                                           VC.MIN_DEPTH, VC.ZFAR, 0.02, device=cuda_device)
    assert rgb.dtype == np.uint8 and count.dtype == np.int32
    assert np.array_equal(count, ref["kdtree_count"]) and np.array_equal(rgb, ref["kdtree_rgb"])
    assert (rgb[count == 0] == 0).all()


def _brute(V, fr, radius, mask=None, zbuf=None, times=1):
    mask = fr["mask"] if mask is None else mask
    zbuf = fr["zbuf"] if zbuf is None else zbuf
    idx, pts = VC.candidates(zbuf, VC.H, VC.W, mask, VC.MIN_DEPTH, fr["cam_in_ob"], VC.K)
    s, c = np.zeros((len(V), 3)), np.zeros(len(V), np.int32)
    for _ in range(times):
        near, dist = VC.brute_frame(V, idx, pts, fr["colors"], radius, s, c)
    return near, dist, s, c


def test_edge_cases(cuda_device):
    fx = VC.fixture()
    fr = fx["frames"][2]                      # the near camera
    radius = 0.06
    # 37 vertices (no multiple of a wave), two of them moved: one behind the camera, one far outside the image
    V = fx["V"][::22][:37].copy()
    assert len(V) == 37
    eye = np.asarray(VC.EYES[2])
    V[5] = (eye * 1.5).astype(np.float32)                                   # behind: the camera looks at the origin
    V[9] = (fr["cam_in_ob"] @ np.array([40.0, 0.0, 1.0, 1.0]))[:3].astype(np.float32)   # u = 60 * 40 + 31.5
    cam = (fr["ob_in_cam"] @ np.r_[V[5].astype(np.float64), 1.0])
    assert cam[2] < 0
    near_b, dist_b, s_b, c_b = _brute(V, fr, radius)
    assert near_b[5] == -1 and near_b[9] == -1 and (near_b >= 0).sum() >= 5
    d = _Device(cuda_device, V)
    near, dist = d.frame(fr["zbuf"], fr["mask"], fr["colors"], fr["cam_in_ob"], fr["ob_in_cam"], radius)
    assert np.array_equal(near, near_b) and _same_bits(dist, dist_b)
    assert _same_bits(d.sum.cpu().numpy(), s_b) and np.array_equal(d.count.cpu().numpy(), c_b)
    # second call: the kernel accumulates
    d.frame(fr["zbuf"], fr["mask"], fr["colors"], fr["cam_in_ob"], fr["ob_in_cam"], radius)
    _, _, s2, c2 = _brute(V, fr, radius, times=2)
    assert _same_bits(d.sum.cpu().numpy(), s2) and np.array_equal(d.count.cpu().numpy(), c2)
    assert np.array_equal(c2, 2 * c_b) and _same_bits(s2, 2 * s_b)
    # all-zero mask, and a z-buffer with no face: nothing matches, the sums stay as they are
    before = d.sum.cpu().numpy().copy()
    for kw in (dict(mask=np.zeros_like(fr["mask"])), dict(zbuf=np.full(VC.H * VC.W, VC.EMPTY, np.uint64))):
        near, dist = d.frame(kw.get("zbuf", fr["zbuf"]), kw.get("mask", fr["mask"]), fr["colors"], fr["cam_in_ob"],
                             fr["ob_in_cam"], radius)
        assert (near == -1).all() and np.isposinf(dist).all()
        assert _same_bits(d.sum.cpu().numpy(), before) and np.array_equal(d.count.cpu().numpy(), c2)
    # no vertices: success, nothing launched
    e = _Device(cuda_device, np.zeros((0, 3), np.float32))
    near, dist = e.frame(fr["zbuf"], fr["mask"], fr["colors"], fr["cam_in_ob"], fr["ob_in_cam"], radius)
    assert near.shape == (0,) and dist.shape == (0,)


def test_runner_vertex_colours_from_train_images(cuda_device, tmp_path):
    """End to end as test_gpu_runner.py::test_texture_from_train_images sets it up. The restatement's
    z-buffers are nof_raster_faces' (pinned bit for bit against oracle.texture.raster above and in
    test_gpu_texture.py): the Python rasteriser would take minutes on this mesh at 640x480."""
    from bundlesdf_amd import _lib
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    from bundlesdf_amd.texture import _cvcam_in_obs
    seq = SY.make_sequence(3, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=100, N_rand=2048,
                         num_levels=16, amp=True)
    cfg.update(save_dir=str(tmp_path), mesh_resolution=0.006, mesh_vertex_attributes=True,
               mesh_vertex_color_source="train_images")
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = nr.extract_mesh(voxel_size=0.006)
    assert nr.mesh_vertex_color_from_train_images(mesh) is mesh
    rgb, count = mesh.vertex_colors, mesh.vertex_color_counts
    n = len(mesh.vertices)
    assert rgb.dtype == np.uint8 and rgb.shape == (n, 3) and count.dtype == np.int32 and count.shape == (n,)
    # the cKDTree restatement on the same mesh, poses and images
    sc, H, W = cfg["sc_factor"], nr.H, nr.W
    K = np.ascontiguousarray(nr.K, np.float64)
    V = torch.as_tensor(mesh.vertices.astype(np.float32), device=cuda_device)
    Fc = torch.as_tensor(mesh.faces, device=cuda_device)
    zb = torch.empty(H * W, dtype=torch.int64, device=cuda_device)
    ks, kc = np.zeros((n, 3)), np.zeros(n, np.int32)
    for i, cam_in_ob in enumerate(_cvcam_in_obs(nr)):
        ob_in_cam = np.ascontiguousarray(np.linalg.inv(cam_in_ob))
        _lib.check(_lib.lib().nof_raster_faces(_lib.ptr(V), _lib.ptr(Fc), len(Fc), ob_in_cam.ctypes.data_as(_lib._p),
                                               K.ctypes.data_as(_lib._p), H, W, 0.1, cfg["far"] * sc, _lib.ptr(zb),
                                               _lib.stream_of(zb)))
        idx, pts = VC.candidates(zb.cpu().numpy(), H, W, np.asarray(nr.masks[i]).reshape(H, W).astype(bool),
                                 0.1 * sc, cam_in_ob, K)
        VC.kdtree_frame(mesh.vertices, idx, pts, np.asarray(nr.images[i], np.float32).reshape(-1, 3), 0.002 * sc, ks, kc)
    assert np.array_equal(count, kc)
    assert np.array_equal(rgb, VC.finish(ks, kc))
    assert (count >= 2).any()
    _record("runner/100steps_voxel0.006", vertices=n, coloured_share=np.mean(count > 0),
            multi_frame_share=np.mean(count > 1))
    # fill_from_network changes exactly the vertices no frame coloured, to the network's colours
    net = nr.mesh_vertex_color_from_network(mesh.copy()).vertex_colors
    filled = nr.mesh_vertex_color_from_train_images(mesh.copy(), fill_from_network=True)
    assert np.array_equal(filled.vertex_color_counts, count)
    assert np.array_equal(filled.vertex_colors[count > 0], rgb[count > 0])
    assert np.array_equal(filled.vertex_colors[count == 0], net[count == 0])
    # the i_mesh hook with the train-image source writes coloured vertices
    nr._hook_mesh()
    lines = open(tmp_path / f"step_{nr.global_step:07d}_mesh_normalized_space.obj").read().split("\n")
    v = [ln for ln in lines if ln.startswith("v ")]
    assert len(v) > 0 and all(len(ln.split()) == 7 for ln in v)
    assert nr.mesh.vertex_color_counts is not None and len(nr.mesh.vertex_color_counts) == len(v)
