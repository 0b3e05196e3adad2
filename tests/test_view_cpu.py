"""CPU: the free-camera ray convention (bundlesdf_amd/view.py) against the ray pool's direction columns,
the surface-render restatement (tests/view_oracle.py) on an analytic sphere, and the C ABI's declarations."""
import os
import re

import numpy as np
import torch

from bundlesdf_amd.view import view_rays
from tests import view_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_rays_reproduce_the_pool_directions():
    """The pool's columns 0-2 at the pool rays' own pixels (recovered as render_images places them). The
    golden pool is the reference's: float64 arithmetic rounded once to float32, against two float32
    roundings here (subtract, divide) — at most 2 ulp of a value of magnitude <= max(|x|, 1)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ray_pool.npz"))
    pool, K = g["pool"], g["K"]
    H, W = g["images"].shape[1:3]
    X = pool[:, :3].astype(np.float64)
    X[:, [1, 2]] = -X[:, [1, 2]]
    p = (K @ X.T).T
    uv = (p / p[:, 2:3]).round().astype(int)[:, :2]
    for f in range(g["poses"].shape[0]):
        sel = pool[:, 8] == f
        assert sel.sum() > 1000
        r = view_rays(g["poses"][f], K, H, W, pixels=uv[sel])
        want = pool[sel, :3]
        got = r["dir_cam"].numpy()
        assert got.dtype == np.float32
        assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.maximum(np.abs(want), 1.0))
        # the world direction is a unit vector and the origin the pose's translation
        assert np.abs(np.linalg.norm(r["dir"].numpy().astype(np.float64), axis=1) - 1).max() < 1e-6
        assert np.array_equal(r["origin"].numpy(), g["poses"][f][:3, 3].astype(np.float32))
    full = view_rays(g["poses"][0], K, H, W)
    assert full["dir"].shape == (H * W, 3) and np.array_equal(full["pixels"].numpy(), np.arange(H * W))
    idx = uv[pool[:, 8] == 0]
    assert torch.equal(full["dir"][idx[:, 1] * W + idx[:, 0]], view_rays(g["poses"][0], K, H, W, pixels=idx)["dir"])


def _sphere_case(step, max_steps, n_refine=8, H=24, W=32):
    c2w = np.eye(4)
    c2w[:3, 3] = [0.05, -0.02, 3.0]           # outside the box, looking down -z at the sphere
    K = np.array([[40.0, 0, (W - 1) / 2], [0, 40.0, (H - 1) / 2], [0, 0, 1]])
    radius = 0.5
    occ = np.ones((8, 8, 8), np.uint8)
    out = VO.render(c2w, K, H, W, occ, 24, lambda p: p.double().norm(dim=1).float() - radius,
                    normal_fn=lambda p: p, step=step, max_steps=max_steps, n_refine=n_refine)
    o, d = out["origin"].double(), out["dir"].double()
    b = (d * o).sum(1)
    disc = b * b - ((o * o).sum() - radius ** 2)
    chord = 2 * torch.sqrt(disc.clamp_min(0))
    t_true = -b - torch.sqrt(disc.clamp_min(0))
    return out, disc, chord, t_true


def test_oracle_finds_the_analytic_sphere():
    for step, max_steps in ((0.05, 512), (0.011, 512), (0.001, 16)):
        out, disc, chord, t_true = _sphere_case(step, max_steps)
        hit, se = out["hit"], out["step_eff"].double()
        assert (out["cnt"] > 0).all()
        if max_steps == 512:
            assert int(out["ns"].max()) > 32                            # more than one tile of samples
        else:
            assert (se > step).all() and int(out["ns"].max()) <= 17     # the widened step is in use
        must = chord > se
        assert must.sum() > 50 and (disc < 0).sum() > 50
        assert hit[must].all()                  # a chord longer than the step holds a sample
        assert not hit[disc < 0].any()          # rays that pass the sphere by
        err = (out["t"].double() - t_true).abs()[hit]
        assert (err <= (se * 2.0 ** -8)[hit]).all(), float(err.max())
        assert (out["index"][hit] > 0).all()    # the camera is outside: always a bracket
        # depth = t |v_z|, normal = the unit gradient (radial on a sphere), misses all zero
        assert torch.equal(out["depth"], torch.where(hit, out["t"] * out["vz"], torch.zeros(())))
        x = out["origin"][None] + out["t"][:, None] * out["dir"]
        assert ((out["normal"] - x / 0.5).abs()[hit] < 1e-3).all()
        for k in ("t", "depth", "normal", "rgb"):
            assert not out[k][~hit].any()


def test_oracle_camera_inside_the_surface_takes_the_first_sample():
    c2w = np.eye(4)
    c2w[:3, 3] = [0.03, 0.04, 0.2]            # inside the sphere (off the voxel faces): sample 0 is non-positive
    K = np.array([[4.0, 0, 1.0], [0, 4.0, 1.0], [0, 0, 1]])
    out = VO.render(c2w, K, 3, 3, np.ones((8, 8, 8), np.uint8), 24, lambda p: p.norm(dim=1) - 0.5, step=0.05)
    assert out["hit"].all() and (out["index"] == 0).all()
    # the first interval's entry is clamped to the camera: t_0 = 0 + 0.5 step
    assert np.array_equal(out["t"].numpy(), np.full(9, np.float32(0.5) * np.float32(0.05), np.float32))


def test_render_view_is_declared_and_bound():
    from bundlesdf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nof.h")).read()
    for name in ("nof_render_view", "nof_render_view_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.declared_symbols()
    for struct in ("nof_view_desc", "nof_view_out"):
        assert re.search(r"\}\s*" + struct + r"\s*;", header), struct
    assert len(_lib._SIGNATURES["nof_render_view"][0]) == 4
