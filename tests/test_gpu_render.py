"""GPU: the forward-only render (nof_render_rays -> FusedStep.render_rays -> NerfRunner.render_images and
the train() hooks) against the CPU render oracle (tests/render_oracle.py).

Tolerances are the existing forward ones of test_gpu_step.py (fp32: z rtol 1e-6 / atol 2e-6, validity
equal, raw rtol 1e-4 / atol 2e-5, rgb rtol 1e-4 / atol 1e-5; amp: raw rtol 1e-2 / atol 2e-3, rgb rtol
2e-3 / atol 1e-4). The depth rule is checked without any tolerance against the rule applied on the host
to the call's own sdf and z."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import nerf_step as NS
from tests import render_oracle as RO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = {False: dict(z=dict(rtol=1e-6, atol=2e-6), raw=dict(rtol=1e-4, atol=2e-5), rgb=dict(rtol=1e-4, atol=1e-5)),
       True: dict(z=dict(rtol=1e-6, atol=2e-6), raw=dict(rtol=1e-2, atol=2e-3), rgb=dict(rtol=2e-3, atol=1e-4))}
BIAS = "sigma_net.2.bias"


@functools.lru_cache(maxsize=None)
def _g4(amp):
    g = np.load(os.path.join(GOLDEN, "train_step_amp.npz" if amp else "train_step.npz"))
    cfg = json.loads(str(g["cfg_json"]))
    P = {"embeddings": g["emb0"], "pose": g["pose0"]}
    P.update({k: g["w0_" + k] for k in NS.MLP_KEYS})
    meta = (g["offsets"], float(np.log2(g["per_level_scale"][0])), cfg["base_res"])
    return dict(cfg=cfg, P=P, meta=meta, batch=g["batch"], c2w=g["c2w"], occ=g["occ"])


def _oracle(c, P, amp, batch=None):
    return RO.render(P, c["batch"] if batch is None else batch, c["c2w"], c["occ"], c["cfg"], c["meta"], amp=amp)


@functools.lru_cache(maxsize=None)
def _shifted(amp):
    """G4 with the table x 3000 and sigma_net.2.bias[0] lowered by the oracle's median sdf: most rays cross
    zero. Returns (params, the oracle's render of them); shared, never modified."""
    c = _g4(amp)
    P = dict(c["P"], embeddings=c["P"]["embeddings"] * 3000)
    b = P[BIAS].copy()
    b[0] -= np.median(_oracle(c, P, amp)["sdf"])
    P[BIAS] = b
    return P, _oracle(c, P, amp)


def _fused(dev, c, P, amp, batch=None):
    from bundlesdf_amd.fused import FusedStep
    from tests.test_gpu_step import _build
    cfg = c["cfg"]
    enc, net, pa = _build(dev, cfg, P["embeddings"], {k: P[k] for k in NS.MLP_KEYS}, P["pose"], cfg["num_levels"],
                          cfg["log2_hashmap_size"], cfg["finest_res"])
    pool = torch.from_numpy(c["batch"] if batch is None else batch).to(dev)
    return FusedStep(cfg, pool, torch.from_numpy(c["c2w"]), torch.from_numpy(c["occ"]), enc, net, pa, amp=amp)


def _render(fs, R=None, **kw):
    R = fs.pool.shape[0] if R is None else R
    out = fs.render_rays(torch.arange(R, dtype=torch.int32, device=fs.dev), samples=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_forward(got, ref, amp):
    """z, validity, sdf and rgb within the forward tolerances. Unperturbed sampling puts the first
    sample of many rays exactly on a face of the box (|x| = 1 to the last bit: G4 has 56 such samples
    of 18,432), where a z inside its tolerance decides |x| <= 1 either way; on those samples (the
    oracle's `edge`: closer to a face than the z tolerance moves a point, under 1 % of the samples)
    validity may differ, and where it does the sdf is that of the other branch and is not compared.
    Everywhere else validity is equal and every sdf is compared; rgb is compared on every ray."""
    t = TOL[amp]
    np.testing.assert_allclose(got["z"], ref["z"], **t["z"])
    edge = ref["edge"]
    assert edge.mean() < 0.01, int(edge.sum())
    np.testing.assert_array_equal(got["valid"][~edge], ref["valid"][~edge])
    same = got["valid"] == ref["valid"]
    print(f"on-face samples {int(edge.sum())}, validity decided the other way on {int((~same).sum())}")
    np.testing.assert_allclose(got["sdf"][same], ref["sdf"][same], **t["raw"])
    np.testing.assert_allclose(got["rgb"], ref["rgb"], **t["rgb"])


def _check_depth_exact(got, far_sc):
    """depth == the rule of render_images :602-610 on the call's own sdf and z, bit for bit."""
    want, inds, empty = RO.depth_rule(got["sdf"], got["z"], far_sc)
    assert got["depth"].dtype == np.float32
    np.testing.assert_array_equal(got["depth"], want)
    return inds, empty


@pytest.mark.parametrize("amp", [False, True])
def test_render_matches_oracle_g4(cuda_device, amp):
    c = _g4(amp)
    got = _render(_fused(cuda_device, c, c["P"], amp))
    ref = _oracle(c, c["P"], amp)
    _check_forward(got, ref, amp)
    # that field's sdf is ~0.164 everywhere: every ray is empty
    far_sc = np.float32(c["cfg"]["far"] * c["cfg"]["sc_factor"])
    assert ref["empty"].all() and (got["depth"] == far_sc).all()
    _check_depth_exact(got, far_sc)
    # validity is decided on exactly the z the call returns: transform_pts in float32 on the host, with
    # the trainer's own tf, gives the same mask bit for bit
    fs = _fused(cuda_device, c, c["P"], amp)
    fs.render_rays(torch.arange(1, device=cuda_device))
    tf = fs.tf_buf.cpu().numpy().reshape(-1, 4, 4)[c["batch"][:, 8].astype(int)]
    p = c["batch"][:, None, :3] * got["z"][:, :, None]
    x = ((tf[:, None, :3, 0] * p[..., 0:1] + tf[:, None, :3, 1] * p[..., 1:2]) + tf[:, None, :3, 2] * p[..., 2:3]) \
        + tf[:, None, :3, 3]
    assert x.dtype == np.float32
    np.testing.assert_array_equal(got["valid"], (np.abs(x) <= 1).all(-1))


@pytest.mark.parametrize("amp", [False, True])
def test_render_depth_rule_exact_on_crossing_field(cuda_device, amp):
    c = _g4(amp)
    P, ref = _shifted(amp)
    got = _render(_fused(cuda_device, c, P, amp))
    _check_forward(got, ref, amp)
    inds, empty = _check_depth_exact(got, c["cfg"]["far"] * c["cfg"]["sc_factor"])
    tiles = set((inds[~empty] // 32).tolist())
    print(f"crossing rays {int((~empty).sum())}, empty {int(empty.sum())}, first-crossing tiles "
          f"{np.bincount(inds[~empty] // 32).tolist()}")
    assert len(tiles) >= 3 and empty.sum() >= 1, (tiles, int(empty.sum()))


def test_render_depth_matches_oracle_depth_fp32(cuda_device):
    """fp32 end to end: depth equals the oracle's within the z tolerance on every ray the oracle finds
    well-conditioned (no sample up to and including its first crossing pair — every sample of an empty ray —
    with |sdf| inside the raw tolerance |sdf| <= 1e-4 |sdf| + 2e-5, where another rounding may flip a sign):
    at most 4 of the 96 rays are ill-conditioned (the oracle alone sets aside 3). A ray is also set aside
    when one of its on-face samples (the oracle's `edge`, see _check_forward) up to that pair was decided
    the other way by the device: that sample then carries the sigma net's output on a zero encoding, of
    either sign. There are at most as many such rays as such samples (3 on this case), so at most 3 + 3 = 6
    rays are set aside in all — two more than the issue's 4, which did not count on-face samples; every
    other ray is compared."""
    c = _g4(False)
    P, ref = _shifted(False)
    got = _render(_fused(cuda_device, c, P, False))
    s = ref["sdf"]
    near0 = np.abs(s) <= 1e-4 * np.abs(s) + 2e-5
    upto = np.where(ref["empty"], s.shape[1], ref["inds"] + 2)
    ill = np.array([near0[r, :upto[r]].any() for r in range(len(s))])
    flipped = got["valid"] != ref["valid"]
    assert not flipped[~ref["edge"]].any()
    flip = np.array([flipped[r, :upto[r]].any() for r in range(len(s))])
    print(f"ill-conditioned rays set aside: {int(ill.sum())}; rays with an on-face sample decided the other "
          f"way: {int(flip.sum())} ({int(flipped.sum())} samples)")
    # the issue's bound on its own criterion (4), and no more rays set aside in all than observed (3 + 3)
    assert ill.sum() <= 4 and flip.sum() <= flipped.sum() and ill.sum() + flip.sum() <= 6
    keep = ~ill & ~flip
    np.testing.assert_allclose(got["depth"][keep], ref["depth"][keep], **TOL[False]["z"])


@pytest.mark.parametrize("amp", [False, True])
def test_render_zero_field_reads_first_sample(cuda_device, amp):
    c = _g4(amp)
    P = dict(c["P"])
    w, b = P["sigma_net.2.weight"].copy(), P[BIAS].copy()
    w[0] = 0
    b[0] = 0
    P["sigma_net.2.weight"], P[BIAS] = w, b
    got = _render(_fused(cuda_device, c, P, amp))
    assert (got["sdf"] == 0).all()
    np.testing.assert_array_equal(got["depth"], got["z"][:, 0])
    _check_depth_exact(got, c["cfg"]["far"] * c["cfg"]["sc_factor"])


def _seam_case(amp, pair):
    """A field / batch on which the ORACLE's first crossing of some ray is the pair (pair, pair + 1): the
    bias is put midway between that ray's sdf[pair + 1] and the nearest of sdf[:pair + 1], on a ray whose
    sdf[pair + 1] lies outside the range of the samples before it. For the pair (127, 128) across the two
    sample groups the rays' depth column is moved 1.2 back: the around-depth group then starts behind the
    occupied voxels, where no octree sample is near it (on the measured depth the octree samples bracket
    every around-depth sample, and no bias can put the first crossing there)."""
    c = _g4(amp)
    P, _ = _shifted(amp)
    batch = c["batch"].copy()
    if pair == 127:
        batch[:, 6] += 1.2
    s = _oracle(c, P, amp, batch)["sdf"]
    head, nb = s[:, :pair + 1], s[:, pair + 1]
    gap = np.maximum(head.min(1) - nb, nb - head.max(1))
    r = int(gap.argmax())
    assert gap[r] > 0, "no ray of the case can have its first crossing at this pair"
    mid = 0.5 * (nb[r] + (head[r].min() if nb[r] < head[r].min() else head[r].max()))
    P = dict(P)
    b = P[BIAS].copy()
    b[0] -= mid
    P[BIAS] = b
    ref = _oracle(c, P, amp, batch)
    assert not ref["empty"][r] and ref["inds"][r] == pair, (r, ref["inds"][r])
    return c, P, batch, ref, r, float(gap[r])


@pytest.mark.parametrize("pair", [31, 127])
@pytest.mark.parametrize("amp", [False, True])
def test_render_depth_rule_at_tile_seams(cuda_device, amp, pair):
    c, P, batch, ref, r, gap = _seam_case(amp, pair)
    got = _render(_fused(cuda_device, c, P, amp, batch))
    inds, empty = _check_depth_exact(got, c["cfg"]["far"] * c["cfg"]["sc_factor"])
    print(f"pair {pair} amp {amp}: oracle ray {r} (gap {gap:.2e}); device first crossing of that ray {inds[r]}, "
          f"rays with it at the pair {int(((inds == pair) & ~empty).sum())}")
    if not amp:   # the gap is two orders above the fp32 raw tolerance: the device takes the same pair
        assert not empty[r] and inds[r] == pair
        assert got["depth"][r] == got["z"][r, pair]
    elif gap / 2 > 8 * 2.0 ** -14:
        # amp: the bias sits gap / 2 from the nearest sdf on either side. These sdf are fp16 Linear outputs
        # below 0.125 in magnitude, where fp16 steps by 2^-14; the device's MFMA chain and the oracle round
        # their fp16 hidden activations at different points, which moves an output by a few such steps
        # (test_gpu_step records this as raw_fp16_ulps) — with the margin above 8 steps the device must find
        # the first crossing of that ray at the same pair
        assert not empty[r] and inds[r] == pair and got["depth"][r] == got["z"][r, pair]


@pytest.mark.parametrize("amp", [False, True])
def test_render_chunking_shapes_and_repeat(cuda_device, amp):
    c = _g4(amp)
    P, _ = _shifted(amp)
    fs = _fused(cuda_device, c, P, amp)
    a, b, a2 = _render(fs, chunk=96), _render(fs, chunk=40), _render(fs, chunk=96)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], a2[k], err_msg=k)
    one = _render(fs, R=1)
    for k in a:
        np.testing.assert_array_equal(one[k], a[k][:1], err_msg=k)
    none = fs.render_rays(torch.zeros(0, dtype=torch.int32, device=cuda_device), samples=True)
    assert none["rgb"].shape == (0, 3) and none["depth"].shape == (0,) and none["z"].shape == (0, 192)
    plain = fs.render_rays(torch.arange(96, device=cuda_device))
    assert set(plain) == {"rgb", "depth"}
    np.testing.assert_array_equal(plain["rgb"].cpu().numpy(), a["rgb"])
    np.testing.assert_array_equal(plain["depth"].cpu().numpy(), a["depth"])
    # ids order: a permutation of the rays permutes the result
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(0))
    shuf = fs.render_rays(perm.to(cuda_device))
    np.testing.assert_array_equal(shuf["rgb"].cpu().numpy(), a["rgb"][perm.numpy()])
    np.testing.assert_array_equal(shuf["depth"].cpu().numpy(), a["depth"][perm.numpy()])


@pytest.mark.parametrize("amp", [False, True])
def test_render_frame_features_matches_oracle(cuda_device, amp):
    from bundlesdf_amd.grid import GridEncoder
    from tests.test_gpu_step import _ff_case, _ff_fused
    cfg, seq, batch, occ, _, mlp_w, emb, pose, offs, ff = _ff_case(R=96)
    cfg = dict(cfg, amp=amp)
    fs, _ = _ff_fused(cuda_device, cfg, seq, batch, occ, mlp_w, emb, pose, ff, amp=amp)
    got = _render(fs)
    P = {"embeddings": emb, "pose": pose, "features": ff}
    P.update(mlp_w)
    meta = (offs, float(np.log2(GridEncoder(3, 16, 2, 16, 19, 512).per_level_scale)), 16)
    ref = RO.render(P, batch, np.asarray(seq["poses"], np.float32), occ, cfg, meta, amp=amp)
    assert got["z"].shape[1] == 320
    _check_forward(got, ref, amp)
    assert np.abs(ref["rgb"]).max() > 0.1   # the colour net took part
    _check_depth_exact(got, cfg["far"] * cfg["sc_factor"])


def test_render_hashed_levels_matches_oracle(cuda_device):
    from tests.test_gpu_step import _build, _scene_case
    from bundlesdf_amd.fused import FusedStep
    cfg, seq, batch, occ, _, mlp_w, emb, pose, offs = _scene_case(seed=7, R=96, log2T=19, finest=512)
    enc, net, pa = _build(cuda_device, cfg, emb, mlp_w, pose, 16, 19, 512)
    c2w = np.asarray(seq["poses"], np.float32)
    fs = FusedStep(cfg, torch.from_numpy(batch).to(cuda_device), torch.from_numpy(c2w), torch.from_numpy(occ), enc,
                   net, pa, amp=False)
    got = _render(fs)
    P = {"embeddings": emb, "pose": pose}
    P.update(mlp_w)
    ref = RO.render(P, batch, c2w, occ, cfg, (offs, float(np.log2(enc.per_level_scale)), 16))
    _check_forward(got, ref, False)
    _check_depth_exact(got, cfg["far"] * cfg["sc_factor"])


STATE = ("P", "M", "V", "Gbuf", "G16", "scale", "tracker", "found_inf", "adam_t", "step_dev", "loss_acc")


@pytest.mark.parametrize("amp", [False, True])
def test_render_leaves_training_state_and_graph_alone(cuda_device, amp):
    c = _g4(amp)
    fs = _fused(cuda_device, c, c["P"], amp)
    ids = torch.arange(96, dtype=torch.int32, device=cuda_device)
    for _ in range(5):
        fs.graph_step_ids(ids)
    torch.cuda.synchronize()
    snap = {k: getattr(fs, k).clone() for k in STATE if getattr(fs, k) is not None}
    graphs, gid, step = fs._graphs, id(fs._graphs), fs.global_step
    ptrs = {k: getattr(fs, k).data_ptr() for k in ("rays", "ids", "workspace")}
    out = fs.render_rays(ids, samples=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out["rgb"]).all()
    for k, v in snap.items():
        assert torch.equal(getattr(fs, k), v), k
    assert fs._graphs is graphs and id(fs._graphs) == gid and fs.global_step == step and fs._R == 96
    assert ptrs == {k: getattr(fs, k).data_ptr() for k in ptrs}
    loss = fs.graph_step_ids(ids)["loss_terms"][:4].sum()
    assert fs._graphs is graphs and torch.isfinite(loss)


def test_render_equals_debug_step_forward_fp32(cuda_device):
    """render_rays against the training forward's own composite (step(debug=True, perturb=False): the debug
    instances of k_encode / k_colour and k_ray_final) on the same parameters; the debug step runs on a
    second trainer, so its Adam update does not matter. Both take the tile sums with the same half-wave
    reductions and add the tiles in tile order, so the two agree to the last bits (1e-6 absolute)."""
    c = _g4(False)
    P, _ = _shifted(False)
    ids = torch.arange(96, dtype=torch.int32, device=cuda_device)
    dbg = _fused(cuda_device, c, P, False).step(ids=ids, debug=True, perturb=False)["dbg"]
    got = _render(_fused(cuda_device, c, P, False))
    assert np.abs(got["rgb"]).max() > 0.1
    np.testing.assert_allclose(got["rgb"], dbg["rgb"].cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["sdf"], dbg["raw"][..., 3].cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(got["z"], dbg["z"].cpu().numpy())


# ---------------------------------------------------------------- NerfRunner
def _runner(n_step, **over):
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(3, seed=1)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=n_step, N_rand=1024,
                         num_levels=16, amp=True, **over)
    return NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                      build_octree_pcd=seq["octree_pts"]), seq


def test_render_images_before_and_after_training(cuda_device, tmp_path):
    nr, seq = _runner(60, save_dir=str(tmp_path), mesh_resolution=0.008)
    H, W = nr.H, nr.W
    far = nr.cfg["far"] * nr.cfg["sc_factor"]

    def errs(frame):
        rgb, depth, mask, gt_rgb, gt_depth, extras = nr.render_images(frame)
        assert rgb.shape == gt_rgb.shape == (H, W, 3) and rgb.dtype == gt_rgb.dtype == np.float64
        assert depth.shape == gt_depth.shape == (H, W) and depth.dtype == gt_depth.dtype == np.float64
        assert mask.shape == (H, W, 3) and mask.dtype == np.uint8
        n = int((nr.rays[:, 8] == frame).sum())
        assert set(extras) == {"z_vals", "sdf", "valid_samples"} and extras["sdf"].shape == (n, 192)
        good = (mask[..., 0] == 255)
        assert good.sum() > 100 and set(np.unique(mask)) <= {0, 255}
        # rendered colour exactly where the ground truth has colour — on the rays with a measured depth: a
        # ray whose depth is beyond far (the dilated mask's background rays) has all-zero weights and
        # renders 0, as raw2outputs makes it (:1160-1163)
        lit = gt_rgb.any(-1)
        np.testing.assert_array_equal(rgb.any(-1)[lit], (gt_depth <= far)[lit])
        assert (gt_depth <= far)[lit].sum() > 1000
        assert not rgb.any(-1)[~(gt_depth > 0)].any()   # nothing outside the frame's ray pixels
        return np.abs(rgb - gt_rgb)[good].mean(), depth, gt_depth, good

    e0, d0, gd, good = errs(1)
    assert (d0[good] == np.float32(far)).all()   # initialisation: no sign change, every ray reads far
    loss = nr.train()["loss_terms"][:4].sum()
    assert torch.isfinite(loss)
    e1, d1, gd, good = errs(1)
    hit = good & (d1 != np.float32(far))
    print(f"render_images: mean |rgb - gt| {e0:.4f} -> {e1:.4f}; median |depth - gt| "
          f"{np.median(np.abs(d0 - gd)[good]):.4f} -> {np.median(np.abs(d1 - gd)[hit]) if hit.any() else -1:.4f} "
          f"({int(hit.sum())} of {int(good.sum())} type-0 rays non-empty)")
    assert e1 < e0
    assert hit.any() and np.median(np.abs(d1 - gd)[hit]) < np.median(np.abs(d0 - gd)[good])
    with pytest.raises(NotImplementedError):
        nr.render_images(0, cur_rays=nr.rays[:4])
    z = nr.render_images(7)   # no such frame in the pool: zero images
    assert not z[0].any() and not z[1].any() and not z[2].any() and z[5]["sdf"].shape == (0, 192)
    # the i_mesh output on this field, whose rendered depths just showed zero crossings (hit.any()): marching
    # cubes must find the surface, so both meshes are written and self.mesh is set
    assert nr.mesh is None
    nr._hook_mesh()
    g = nr.global_step
    assert {f"step_{g:07d}_mesh_normalized_space.obj", f"step_{g:07d}_mesh_real_world.obj"} <= set(os.listdir(tmp_path))
    assert nr.mesh is not None and len(nr.mesh.faces) > 100 and np.abs(nr.mesh.vertices).max() <= 1 + 1e-6
    # a render between two train() calls leaves the trainer usable
    nr.N_iters = 1
    assert torch.isfinite(nr.train()["loss_terms"][:4].sum())


def test_train_hooks_write_the_periodic_outputs(cuda_device, tmp_path):
    class Run:
        def __init__(self):
            self.artifacts, self.scalars = [], []

        def add_artifact(self, p):
            self.artifacts.append(os.path.basename(p))

        def log_scalar(self, k, v, step):
            self.scalars.append((k, step))

    nr, seq = _runner(20, i_img=10, i_pose=10, i_weights=10, i_mesh=20, i_print=10, save_dir=str(tmp_path),
                      mesh_resolution=0.008)
    nr._run = Run()
    out = nr.train()
    assert torch.isfinite(out["loss_terms"][:4].sum()) and nr.global_step == 21
    names = set(os.listdir(tmp_path))
    for g in (10, 20):
        assert f"image_step_{g:07d}.png" in names and f"step_{g:07d}_optimized_poses.txt" in names
    assert "model_latest.pth" in names and not any("0000000" in n or "0000005" in n for n in names)
    png = open(tmp_path / "image_step_0000020.png", "rb").read()
    import struct
    w, h = struct.unpack(">II", png[16:24])
    rows = len({0, 1, 2})   # 3 frames: every frame is a validation frame (:768-773)
    assert (h, w) == (rows * nr.H, 5 * nr.W)
    poses = np.loadtxt(tmp_path / "step_0000020_optimized_poses.txt")
    assert poses.shape == (4 * 3, 4) and np.isfinite(poses).all()
    ck = torch.load(tmp_path / "model_latest.pth", weights_only=False)
    assert ck["global_step"] == 20
    # i_mesh = 20: after 20 steps the field already has a zero level set (5,880 faces observed), so both
    # meshes of :823-841 are written, registered as artifacts, and self.mesh is set; nothing at g = 10
    meshes = {"step_0000020_mesh_normalized_space.obj", "step_0000020_mesh_real_world.obj"}
    assert meshes <= names and meshes <= set(nr._run.artifacts)
    assert not any("0000010_mesh" in n for n in names)
    assert nr.mesh is not None and len(nr.mesh.faces) > 100
    from bundlesdf_amd.mesh import Mesh
    vn = np.array([ln.split()[1:4] for ln in open(tmp_path / "step_0000020_mesh_normalized_space.obj")
                   if ln.startswith("v ")], np.float64)
    vw = np.array([ln.split()[1:4] for ln in open(tmp_path / "step_0000020_mesh_real_world.obj")
                   if ln.startswith("v ")], np.float64)
    assert isinstance(nr.mesh, Mesh) and vn.shape == vw.shape == nr.mesh.vertices.shape
    np.testing.assert_allclose(vn, nr.mesh.vertices, atol=1e-5)
    # the real-world mesh is the normalised one over sc_factor, moved rigidly (mesh_to_real_world + pose offset)
    dn, dw = np.linalg.norm(vn - vn[0], axis=1), np.linalg.norm(vw - vw[0], axis=1)
    assert np.abs(vn).max() <= 1 + 1e-5 and dn.max() > 0.1
    np.testing.assert_allclose(dw, dn / nr.cfg["sc_factor"], atol=1e-5)
    assert {s for _, s in nr._run.scalars} == {0, 10, 20} and "image_step_0000010.png" in nr._run.artifacts
    assert {"step_0000010_optimized_poses.txt", "step_0000020_optimized_poses.txt"} <= set(nr._run.artifacts)


def test_train_without_hooks_is_what_it_was(cuda_device):
    """Every i_* key at 999999, and a runner without the keys. The actual check is the stub: every _hook_*
    is replaced by pytest.fail, so train() may not call one in either configuration — with no hook called,
    train() runs exactly the step loop it ran before. The loss comparison cannot be the issue's "bit for bit"
    over the whole run: two runs of one unchanged trainer already differ in the low bits after a few steps
    (the table gradient is summed with float atomics, whose order is free). So the first step's loss terms
    (a forward from identical parameters, summed in a fixed order) are compared bit for bit, and the 21st
    step's only within AMP_LOSS_TOL of test_gpu_step.py, as a sanity check that both ran the same schedule."""
    from tests.test_gpu_step import AMP_LOSS_TOL
    res = []
    for drop in (False, True):
        outs = []
        for n_iters in (1, 21):
            nr, _ = _runner(20)
            if drop:
                for k in ("i_print", "i_img", "i_weights", "i_mesh", "i_pose"):
                    nr.cfg.pop(k)
            for k in ("weights", "img", "print", "mesh", "pose"):
                setattr(nr, "_hook_" + k, lambda out, k=k: pytest.fail(f"hook {k} ran"))
            nr.N_iters = n_iters
            outs.append(nr.train()["loss_terms"].clone())
        res.append(outs)
    assert torch.equal(res[0][0], res[1][0]), (res[0][0], res[1][0])
    np.testing.assert_allclose(res[0][1][:4].cpu().numpy(), res[1][1][:4].cpu().numpy(), rtol=AMP_LOSS_TOL)
