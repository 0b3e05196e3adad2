"""GPU: nof_render_mesh (bundlesdf_amd.mesh_render) against tests/mesh_render_oracle.py on the shared
48x64 scene: depth, face and mask bit for bit against oracle.texture.raster's keys and against
nof_raster_faces run once per pose; rgb and normal exactly against the f64 restatement of the shade
step in every colour mode, lit and unlit; the same bytes for every small_max_pixels, on a second
call and for a single pose; the ModelRendererOffscreen shim; NerfRunner.render_mesh on a trained
runner's own mesh against its frames."""
import numpy as np
import pytest
import torch

from tests import mesh_render_oracle as MR

pytestmark = pytest.mark.gpu
KEYS = ("depth", "face", "mask", "rgb", "normal")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


@pytest.fixture(scope="module")
def renderer(cuda_device):
    from bundlesdf_amd.mesh_render import MeshRenderer
    return MeshRenderer(MR.scene()["mesh"], MR.K, MR.H, MR.W, znear=MR.ZNEAR, zfar=MR.ZFAR, device=cuda_device)


@pytest.fixture(scope="module")
def batch(renderer):
    """The three poses in one call, colour 'vertex', default threshold."""
    return _host(renderer.render(MR.scene()["poses"], colour="vertex"))


def test_depth_face_mask_match_the_raster_oracle_and_k_raster(renderer, batch, cuda_device):
    from bundlesdf_amd import _lib
    from bundlesdf_amd.mesh_render import SMALL_MAX_PIXELS
    s = MR.scene()
    ids, mesh = s["ids"], s["mesh"]
    assert batch["depth"].shape == (3, MR.H, MR.W) and batch["depth"].dtype == np.float32
    assert batch["face"].dtype == np.int32 and batch["mask"].dtype == bool and batch["rgb"].dtype == np.uint8
    zb = torch.empty(MR.H * MR.W, dtype=torch.int64, device=cuda_device)
    for b, (T, keys) in enumerate(zip(s["poses"], s["keys"])):
        hit = keys != MR.EMPTY
        depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0)).reshape(MR.H, MR.W)
        face = np.where(hit, (keys & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32).reshape(MR.H, MR.W)
        assert np.array_equal(batch["depth"][b].view(np.uint32), depth)
        assert np.array_equal(batch["face"][b], face)
        assert np.array_equal(batch["mask"][b], hit.reshape(MR.H, MR.W))
        Tc = np.ascontiguousarray(T)
        _lib.check(_lib.lib().nof_raster_faces(_lib.ptr(renderer.V), _lib.ptr(renderer.F), len(renderer.F),
                                               Tc.ctypes.data_as(_lib._p), MR.K.ctypes.data_as(_lib._p), MR.H, MR.W,
                                               MR.ZNEAR, MR.ZFAR, _lib.ptr(zb), _lib.stream_of(zb)))
        assert np.array_equal(zb.cpu().numpy().view(np.uint64), keys)
        assert ids["duplicate"] not in batch["face"][b] and ids["zero_area"] not in batch["face"][b]
    # not vacuous (all from the oracle, on the host)
    face0 = MR.reference(0, "vertex", False)[1]
    assert (face0 >= 0).sum() > 300 and ids["original"] in face0 and ids["near"] not in face0
    box = MR.box_pixels(mesh.vertices, mesh.faces, s["poses"][0], MR.K, MR.H, MR.W, MR.ZNEAR)
    assert (box > SMALL_MAX_PIXELS).sum() >= 2 and ((box > 0) & (box <= SMALL_MAX_PIXELS)).sum() >= 50
    assert box[ids["quad"]].tolist() == [MR.H * MR.W] * 2           # larger than the screen: the box is clamped
    from oracle import texture as TX
    quad_alone = TX.raster(mesh.vertices, mesh.faces[ids["quad"]], s["poses"][0], MR.K, MR.H, MR.W, MR.ZNEAR, MR.ZFAR)
    assert (quad_alone != MR.EMPTY).all()                            # the quad covers every pixel on its own,
    on_sphere, on_quad = np.isin(face0, ids["sphere"]), np.isin(face0, ids["quad"])
    assert on_sphere.sum() > 300 and on_quad.sum() > 300             # the sphere hides some of it and leaves the rest
    face1 = MR.reference(1, "vertex", False)[1]
    assert 50 < np.isin(face1, ids["sphere"]).sum() and np.isin(face1[:, -1], ids["sphere"]).any()   # cut by the border
    # everything off-screen: all misses
    assert (s["keys"][2] == MR.EMPTY).all() and (batch["face"][2] == -1).all()
    for k in ("depth", "mask", "rgb", "normal"):
        assert not batch[k][2].any()


@pytest.mark.parametrize("mode,shade,normals", [("vertex", False, True), ("flat", False, True), ("texture", False, True),
                                                ("vertex", True, True), ("flat", True, True), ("texture", True, True),
                                                ("vertex", True, False)])
def test_rgb_and_normal_equal_the_oracle(renderer, cuda_device, mode, shade, normals):
    from bundlesdf_amd.mesh_render import MeshRenderer
    s = MR.scene()
    r = renderer
    if not normals:                       # the face-normal path
        m = s["mesh"].copy()
        m.vertex_normals = None
        r = MeshRenderer(m, MR.K, MR.H, MR.W, znear=MR.ZNEAR, zfar=MR.ZFAR, device=cuda_device)
    out = _host(r.render(s["poses"], colour=mode, shade=shade))
    for b in range(3):
        depth, face, rgb, normal = MR.reference(b, mode, shade, normals)
        assert np.array_equal(out["face"][b], face) and np.array_equal(_bits(out["depth"][b]), _bits(depth))
        assert np.array_equal(out["rgb"][b], rgb), (b, np.abs(out["rgb"][b].astype(int) - rgb).max())
        assert np.array_equal(_bits(out["normal"][b]), _bits(normal))
    hit = out["mask"][0]
    n = np.linalg.norm(out["normal"][0][hit].astype(np.float64), axis=1)
    v, u = np.nonzero(hit)
    ray = np.stack([(u - MR.K[0, 2]) / MR.K[0, 0], (v - MR.K[1, 2]) / MR.K[1, 1], np.ones(len(u))], 1)
    assert np.abs(n - 1).max() < 1e-6 and ((out["normal"][0][hit] * ray).sum(1) <= 1e-6).all()   # unit, towards the camera


def test_auto_colour_picks_texture_then_vertex_then_flat(renderer, cuda_device):
    from bundlesdf_amd.mesh_render import MeshRenderer
    s = MR.scene()
    assert np.array_equal(renderer.render(s["poses"][0])["rgb"].cpu().numpy(), MR.reference(0, "texture", False)[2])
    m = s["mesh"].copy()
    m.texture = None
    r = MeshRenderer(m, MR.K, MR.H, MR.W, znear=MR.ZNEAR, zfar=MR.ZFAR, device=cuda_device)
    assert np.array_equal(r.render(s["poses"][0])["rgb"].cpu().numpy(), MR.reference(0, "vertex", False)[2])
    with pytest.raises(ValueError, match="texture"):
        r.render(s["poses"][0], colour="texture")
    m.vertex_colors = None
    r = MeshRenderer(m, MR.K, MR.H, MR.W, znear=MR.ZNEAR, zfar=MR.ZFAR, device=cuda_device)
    assert np.array_equal(r.render(s["poses"][0])["rgb"].cpu().numpy(), MR.reference(0, "flat", False)[2])


@pytest.mark.parametrize("small_max_pixels", [0, 2 ** 30])
def test_every_threshold_gives_the_same_bytes(renderer, batch, small_max_pixels):
    """0: every face through the wave kernel; 2^30: every face through its own lane; `batch`: the default."""
    out = _host(renderer.render(MR.scene()["poses"], colour="vertex", small_max_pixels=small_max_pixels))
    assert _same(out, batch)


def test_second_call_and_single_pose_give_the_same_bytes(renderer, batch):
    poses = MR.scene()["poses"]
    assert _same(_host(renderer.render(poses, colour="vertex")), batch)
    one = _host(renderer.render(poses[0], colour="vertex"))
    assert one["depth"].shape == (MR.H, MR.W) and one["rgb"].shape == (MR.H, MR.W, 3)
    assert _same(one, {k: v[0] for k, v in batch.items()})
    from bundlesdf_amd.mesh_render import render_mesh
    shot = _host(render_mesh(MR.scene()["mesh"], torch.as_tensor(poses[1]), MR.K, MR.H, MR.W, znear=MR.ZNEAR,
                             zfar=MR.ZFAR, colour="vertex"))
    assert _same(shot, {k: v[1] for k, v in batch.items()})


def test_model_renderer_offscreen_merges_by_nearest_depth(cuda_device, tmp_path):
    from bundlesdf_amd.compat.offscreen_renderer import ModelRendererOffscreen
    from bundlesdf_amd.mesh import Mesh
    from bundlesdf_amd.mesh_render import render_mesh
    rng = np.random.default_rng(3)
    v, f = MR.icosphere(1, 0.2)
    a = Mesh(v, f)
    a.vertex_colors = rng.integers(1, 256, (len(v), 3)).astype(np.uint8)
    a.export(str(tmp_path / "a.obj"))
    a = Mesh.load(str(tmp_path / "a.obj"))             # what the renderer reads: six decimals
    b = Mesh(v * 1.5, f)
    b.vertex_colors = rng.integers(1, 256, (len(v), 3)).astype(np.uint8)
    Ta, Tb = np.eye(4), np.eye(4)
    Ta[:3, 3], Tb[:3, 3] = [-0.1, 0.0, 0.8], [0.15, 0.05, 1.1]
    mr = ModelRendererOffscreen([str(tmp_path / "a.obj")], MR.K, MR.H, MR.W, zfar=2)
    mr.add_mesh(b)
    color, depth = mr.render([Ta, Tb])
    assert color.dtype == np.uint8 and color.shape == (MR.H, MR.W, 3)
    assert depth.dtype == np.float32 and depth.shape == (MR.H, MR.W)
    ra = _host(render_mesh(a, Ta, MR.K, MR.H, MR.W, zfar=2.0))
    rb = _host(render_mesh(b, Tb, MR.K, MR.H, MR.W, zfar=2.0))
    a_wins = ra["mask"] & (~rb["mask"] | (ra["depth"] <= rb["depth"]))
    b_wins = rb["mask"] & ~a_wins
    assert (ra["mask"] & rb["mask"]).sum() > 20 and (a_wins & rb["mask"]).sum() > 20 and b_wins.sum() > 50
    assert np.array_equal(depth, np.where(a_wins, ra["depth"], np.where(b_wins, rb["depth"], 0)).astype(np.float32))
    assert np.array_equal(color, np.where(a_wins[..., None], ra["rgb"], np.where(b_wins[..., None], rb["rgb"], 0)))
    assert (depth[~(ra["mask"] | rb["mask"])] == 0).all()
    colors, depths = mr.renderBatch([[Ta, Tb], [Tb, Ta]])
    assert colors.shape == (2, MR.H, MR.W, 3) and depths.shape == (2, MR.H, MR.W)
    assert np.array_equal(colors[0], color) and np.array_equal(depths[0], depth)
    mr.clear_meshes()
    color, depth = mr.render([])
    assert not color.any() and not depth.any()


def test_runner_mesh_coincides_with_its_frames(cuda_device):
    """NerfRunner.render_mesh on the synthetic runner's own mesh (100 steps, quarter-size frames, voxel
    size s = 6 mm, the largest component as bundlesdf.py:748-759 keeps it) against the frames.

    Bounds, from the scene and not from a run. Marching cubes places every vertex on a grid edge of
    a cell the surface crosses, so a mesh of a field that has the analytic surface as its zero set
    lies within one voxel diagonal d = sqrt(3) s of it; the training error of the field itself
    (test_extract_mesh_after_training: a median of under 2 mm) is inside that allowance at s = 6 mm.
      depth   along a pixel ray the mesh is met within d of the frame's depth except at grazing
              angles and silhouette pixels, which a median ignores: median |render - frame| over
              pixels valid in both <= d * sc_factor (depths are in normalised units).
      IoU     a surface moved by at most d moves the silhouette by at most r = ceil(f d / z_min)
              pixels, f the focal length of the quarter-size frames and z_min the smallest observed
              depth (metres). With M the frame's mask, the mesh's silhouette S then holds M eroded
              by r and lies in M dilated by r, so IoU(S, M) = |S and M| / |S or M| >= |erode_r M| /
              |dilate_r M|. Both are counted here on the CPU from the frame's analytic mask (a
              (2r+1)^2 square), per frame."""
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.evaluate import mesh_frame_agreement
    from bundlesdf_amd.mesh import largest_component
    from bundlesdf_amd.nerf_runner import NerfRunner
    s = 0.006
    seq = SY.make_sequence(3, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=100, N_rand=2048,
                         num_levels=16, amp=True, down_scale_ratio=4)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = largest_component(nr.extract_mesh(voxel_size=s))
    assert mesh is not None
    sc, far = cfg["sc_factor"], cfg["far"] * cfg["sc_factor"]
    out = nr.render_mesh(mesh)
    assert out["depth"].shape == (3, nr.H, nr.W) and out["rgb"].shape == (3, nr.H, nr.W, 3)
    one = nr.render_mesh(mesh, frame_ids=1, metres=True)
    assert one["depth"].shape == (nr.H, nr.W) and np.array_equal(one["face"], out["face"][1])
    assert np.allclose(one["depth"], out["depth"][1] / np.float32(sc), rtol=1e-6, atol=0)
    obs_depth = torch.as_tensor(np.asarray(nr.depths, np.float32)[..., 0])
    obs_mask = torch.as_tensor(np.asarray(nr.masks)[..., 0] > 0)
    agree = mesh_frame_agreement(out["depth"], out["mask"], obs_depth, obs_mask, far)
    # the bounds
    d = np.sqrt(3.0) * s
    valid = obs_mask & (obs_depth > 0) & (obs_depth <= far)
    z_min = float(obs_depth[valid].min()) / sc
    r = int(np.ceil(nr.K[0, 0] * d / z_min))
    m = valid[:, None].float()
    grown = torch.nn.functional.max_pool2d(m, 2 * r + 1, stride=1, padding=r)[:, 0]
    shrunk = 1 - torch.nn.functional.max_pool2d(1 - m, 2 * r + 1, stride=1, padding=r)[:, 0]
    iou_min = shrunk.sum((1, 2)) / grown.sum((1, 2))
    print(f"voxel diagonal {d * 1e3:.2f} mm = {d * sc:.4f} normalised, rim {r} px, IoU bounds {iou_min.tolist()}; "
          f"IoU {agree['iou'].tolist()}, median |depth diff| {agree['depth_median'].tolist()}, mean "
          f"{agree['depth_mean'].tolist()}, pixels {agree['count'].tolist()}")
    assert (valid.sum((1, 2)) > 200).all() and (iou_min > 0.3).all() and r <= 6      # the bounds say something
    assert (agree["count"] > 200).all()
    assert (agree["depth_median"] <= d * sc).all()
    assert (agree["iou"] >= iou_min.double()).all()
