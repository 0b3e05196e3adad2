"""GPU: bundlesdf_amd.frames (csrc/frame_maps.hip, include/nof.h group 10) against tests/
frame_maps_oracle.py. Every stage is checked on the kernel's own previous-stage output (return_stages),
so a one-ulp difference in one stage can never flip a threshold in the next.

What is exact and what is not. Kernel and oracle do the same IEEE float64 +, -, x, / and sqrt in the
same order on the same float32 inputs, without contraction, so erode, the geometry stage, the lift and
the covisibility counts are compared bit for bit. The bilateral pass calls exp, which neither side
rounds correctly. Its decisions are still exact: n, the sum of at most (2 r + 1)^2 = 289 float32
values within a few binades (24-bit significands, a sum below 2^9 times the largest: 33 bits, well
inside float64's 53), hence mean = S / n (one rounded division) and which taps pass |x - mean| < band.
Its output s / sw differs between the two sides only through exp: each weight by a few double ulps
(2^-52 relative), each of the two sums of at most 289 terms by at most 289 x 2^-53 relative on top, the
quotient by one more rounding: below 2^-42 relative in all, against half a float32 ulp at 2^-25
relative. The two float64 results therefore lie within 2^-42 of each other and their float32 roundings
are the same or adjacent: the test asks for at most 1 float32 ulp at every pixel.
"""
import json
import os

import numpy as np
import pytest
import torch

from bundlesdf_amd import frames as F
from tests import frame_maps_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _np(t):
    return t.cpu().numpy()


def _scene_run(dev):
    """One prepare_frames run on the scene with its stages, shared by the tests (read-only)."""
    if "scene" not in _CACHE:
        sc = O.scene()
        maps = F.prepare_frames(sc["depth"], sc["K"], sc["mask"], return_stages=True, device=dev)
        torch.cuda.synchronize()
        _CACHE["scene"] = (sc, maps)
    return _CACHE["scene"]


def _ulps(a, b):
    """Distance in float32 steps between two float32 arrays of one sign pattern (depths are >= 0)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _check_stages(depth, K, mask, maps, p):
    """Each stage of maps (with stages) against the oracle on the kernel's own previous stage."""
    N = 1 if np.ndim(depth) == 2 else len(depth)
    shape3 = (N,) + tuple(np.shape(depth)[-2:])
    e = _np(maps.stages["eroded"]).reshape(shape3)
    _same(e, O.erode(np.reshape(depth, shape3), p["zfar"], p["depth_min"], p["erode_radius"], p["erode_diff"],
                     p["erode_ratio"]), "erode")
    prev = e
    assert len(maps.stages["bilateral"]) == p["bilateral_passes"]
    for k, b in enumerate(maps.stages["bilateral"]):
        b = _np(b).reshape(shape3)
        want, _ = O.bilateral_pass(prev, p["zfar"], p["depth_min"], p["bilateral_radius"], p["sigma_d"], p["sigma_r"],
                                   p["bilateral_band"])
        assert ((b == 0) == (want == 0)).all(), k
        assert (b >= 0).all() and np.isfinite(b).all()
        worst = int(_ulps(b, want).max())
        print(f"bilateral pass {k}: worst {worst} ulp, {int((b != want).sum())} of {b.size} pixels differ")
        assert worst <= 1, (k, worst)
        prev = b
    d, pts, nrm, nv = O.geometry(prev, K, None if mask is None else np.reshape(mask, shape3), p["depth_min"], p["z_diff"],
                                 p["edge_angle_deg"])
    got_d = _np(maps.depth).reshape(shape3)
    _same(got_d, d, "depth")
    _same(_np(maps.points).reshape(shape3 + (3,)), pts, "points")
    _same(_np(maps.normals).reshape(shape3 + (3,)), nrm, "normals")
    _same(_np(maps.n_valid).reshape(N), nv, "n_valid")
    return got_d


def test_scene_stage_by_stage(cuda_device):
    sc, maps = _scene_run(cuda_device)
    assert maps.depth.shape == (3, O.H, O.W) and maps.points.shape == (3, O.H, O.W, 3) and maps.n_valid.shape == (3,)
    assert O.H % F.TILE[0] and O.W % F.TILE[1] and O.H > 2 * F.TILE[0] and O.W > 2 * F.TILE[1]
    _check_stages(sc["depth"], sc["K"], sc["mask"], maps, O.DEFAULTS)
    nv = _np(maps.n_valid)
    assert nv[2] == 0 and (nv[:2] > 500).all()


def test_scene_properties(cuda_device):
    from bundlesdf_amd import handoff
    sc, maps = _scene_run(cuda_device)
    depth, points, normals = _np(maps.depth), _np(maps.points), _np(maps.normals)
    for f in range(3):
        _same(points[f], _np(handoff.depth2xyzmap(depth[f], sc["K"][f], device=cuda_device)), f"depth2xyzmap {f}")
    gone = depth == 0
    assert ((points == 0).all(-1) == gone).all()
    assert (normals[gone] == 0).all()
    length = np.linalg.norm(normals.astype(np.float64), axis=-1)
    has = length > 0
    assert has.sum() > 500 and (np.abs(length[has] - 1) <= 3 * 2.0 ** -24).all()      # three float32 roundings
    assert (depth[sc["mask"] == 0] == 0).all()
    assert np.array_equal(_np(maps.n_valid), (~gone).reshape(3, -1).sum(1))


def test_composition_and_determinism(cuda_device):
    sc, maps = _scene_run(cuda_device)
    e = F.erode_depth(sc["depth"], device=cuda_device)
    b, passes = F.bilateral_depth(e, return_passes=True)
    g = F.depth_geometry(b, sc["K"], sc["mask"])
    again = F.prepare_frames(torch.from_numpy(sc["depth"]).to(cuda_device), torch.from_numpy(sc["K"]),
                             torch.from_numpy(sc["mask"]), return_stages=True)
    torch.cuda.synchronize()
    for other in (g, again):
        for k in ("depth", "points", "normals", "n_valid"):
            _same(_np(getattr(other, k)), _np(getattr(maps, k)), k)
    _same(_np(e), _np(maps.stages["eroded"]), "eroded")
    _same(_np(again.stages["eroded"]), _np(maps.stages["eroded"]), "eroded again")
    for k in range(2):
        _same(_np(passes[k]), _np(maps.stages["bilateral"][k]), f"pass {k}")
        _same(_np(again.stages["bilateral"][k]), _np(maps.stages["bilateral"][k]), f"pass {k} again")


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3)])
def test_single_small_frames(cuda_device, shape):
    rng = np.random.default_rng(sum(shape))
    d = (0.5 + rng.uniform(-0.0004, 0.0004, shape)).astype(np.float32)
    K = np.array([[50.0, 0.0, shape[1] / 2], [0.0, 55.0, shape[0] / 2], [0.0, 0.0, 1.0]])
    maps = F.prepare_frames(d, K, return_stages=True, device=cuda_device)
    assert maps.depth.shape == shape and maps.points.shape == shape + (3,) and maps.n_valid.shape == ()
    got = _check_stages(d, K, None, maps, O.DEFAULTS)
    assert (got > 0).all()
    if shape == (3, 3):
        n = _np(maps.normals)
        assert (n[1, 1] != 0).any() and (np.delete(n.reshape(9, 3), 4, 0) == 0).all()      # the one interior pixel
    else:
        assert (_np(maps.normals) == 0).all()


@pytest.mark.parametrize("over", [dict(erode_radius=0), dict(bilateral_radius=0), dict(erode_radius=8, bilateral_radius=8),
                                  dict(bilateral_passes=0), dict(bilateral_passes=1), dict(mask=None),
                                  dict(erode_ratio=0.5, bilateral_band=0.05, z_diff=0.005, edge_angle_deg=25.0, zfar=0.6)],
                         ids=["erode_r0", "bilateral_r0", "r8_on_5x5", "passes0", "passes1", "no_mask", "other_thresholds"])
def test_radii_passes_and_mask(cuda_device, over):
    sc = O.scene()
    depth, K, mask = sc["depth"], sc["K"], sc["mask"]
    if over.get("erode_radius") == 8:
        depth, mask = np.ascontiguousarray(depth[:, 10:15, 20:25]), np.ascontiguousarray(mask[:, 10:15, 20:25])
        over = dict(over, erode_diff=0.05)
    if "mask" in over:
        over = dict(over)
        mask = over.pop("mask")
    p = dict(O.DEFAULTS, **over)
    maps = F.prepare_frames(depth, K, mask, return_stages=True, device=cuda_device, **over)
    _check_stages(depth, K, mask, maps, p)
    if over.get("bilateral_passes") == 0:
        assert maps.stages["bilateral"] == []


def _lifted(dev, **gates):
    sc, maps = _scene_run(dev)
    key = ("lift",) + tuple(sorted(gates.items()))
    if key not in _CACHE:
        pf, ps, uv_a, uv_b = O.match_rows(sc, _np(maps.depth))
        kw = dict(gates, poses=sc["poses"]) if gates else {}
        got = F.lift_matches(maps, pf, uv_a, uv_b, ps, **kw)
        want = O.lift(_np(maps.points), _np(maps.normals), pf, ps, uv_a, uv_b, **kw)
        _CACHE[key] = (got, want, (pf, ps, uv_a, uv_b))
    return _CACHE[key]


@pytest.mark.parametrize("gates", [{}, dict(max_dist=0.25), dict(max_normal_deg=40.0), dict(max_dist=0.25, max_normal_deg=40.0)],
                         ids=["plain", "dist", "normal", "both"])
def test_lift_matches_the_oracle(cuda_device, gates):
    got, want, (pf, ps, uv_a, uv_b) = _lifted(cuda_device, **gates)
    valid = _np(got.valid)
    assert valid.dtype == bool and np.array_equal(valid, want[4])
    for k, name in enumerate(("pts_a", "pts_b", "normals_a", "normals_b")):
        _same(_np(getattr(got, name)), want[k], name)
    assert 0 < valid.sum() < len(valid)
    assert np.array_equal(_np(got.pair_start), ps) and np.array_equal(_np(got.pair_frames), pf)
    if not gates:
        # match_rows plants its special coordinates from row 10 on, alternately in uv_a and uv_b: (-0.5, 5) rounds to
        # u = -1, (5, -0.5) to v = -1, (5, H - 0.5) to v = H, then NaN, +inf, -inf, 1e300 and (-3, -3)
        assert not valid[[12, 16, 18, 20, 21, 22, 23, 29]].any()
        sc, maps = _scene_run(cuda_device)
        if valid[10]:                              # (10.5, 7.5) is pixel (11, 8), not numpy's (10, 8)
            assert _np(got.pts_a)[10, 2] == _np(maps.depth)[0, 8, 11]
    else:
        plain = _np(_lifted(cuda_device)[0].valid)
        assert (valid <= plain).all() and valid.sum() < plain.sum()


def test_lift_compact_and_ransac(cuda_device):
    from bundlesdf_amd.ransac import ransac_pairs
    got, want, (pf, ps, uv_a, uv_b) = _lifted(cuda_device)
    c = got.compact()
    keep = want[4]
    for k, name in enumerate(("pts_a", "pts_b", "normals_a", "normals_b")):
        _same(_np(getattr(c, name)), want[k][keep], name)
    csum = np.concatenate([[0], np.cumsum(keep)])
    assert np.array_equal(_np(c.pair_start), csum[ps]) and _np(c.pair_start).dtype == np.int32
    assert np.array_equal(_np(c.rows), np.flatnonzero(keep)) and _np(c.valid).all() and len(c.valid) == keep.sum()
    res = ransac_pairs(c.pts_a, c.pts_b, c.pair_start, c.normals_a, c.normals_b, inlier_dist=0.05, n_trials=64,
                       refit=False)
    torch.cuda.synchronize()
    assert res.inlier.shape == (int(keep.sum()),) and res.n_inliers.shape == (3,)
    assert _np(res.n_inliers)[0] == 0


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_covisibility_counts(cuda_device, stride):
    sc, maps = _scene_run(cuda_device)
    pairs = [(a, b) for a in range(3) for b in range(3)]
    ratio, counts = F.covisibility(maps, sc["poses"], pairs, stride=stride)
    want_ratio, want = O.covisibility(_np(maps.points), _np(maps.normals), sc["poses"], pairs, stride=stride)
    assert counts.dtype == torch.int32 and ratio.dtype == torch.float64
    assert np.array_equal(_np(counts), want), (stride, _np(counts), want)
    _same(_np(ratio), want_ratio, "ratio")
    c = _np(counts)
    assert (c[6:] == 0).all() and (_np(ratio)[6:] == 0).all()          # frame 2 has no valid pixel
    assert (c[:6, 1] > 0).all() and (c[:, 0] <= c[:, 1]).all()
    empty_ratio, empty = F.covisibility(maps, sc["poses"], np.zeros((0, 2), np.int64), stride=stride)
    assert empty.shape == (0, 2) and empty_ratio.shape == (0,)


def test_plane_is_fully_visible_from_itself(cuda_device):
    d, K = O.plane_scene()
    maps = F.prepare_frames(d, K, device=cuda_device)
    n = _np(maps.normals)[0, 1:-1, 1:-1]
    assert np.array_equal(n, np.broadcast_to(np.float32([0, 0, -1]), n.shape))
    for stride in (1, 2):
        ratio, counts = F.covisibility(maps, np.eye(4)[None], [(0, 0)], stride=stride)
        c = _np(counts)[0]
        # border pixels have no normal: the visited pixels are the strided ones inside rows 1 .. 7, columns 1 .. 9
        interior = len([v for v in range(0, 9, stride) if 1 <= v <= 7]) * len([u for u in range(0, 11, stride) if 1 <= u <= 9])
        assert c[0] == c[1] == interior, (stride, c, interior)
        assert abs(float(ratio[0]) - 1.0) < 1e-8


def test_call_on_another_stream(cuda_device):
    """Every call launches on the caller's current stream and waits for nothing: issued on a side stream
    and synchronised there alone, the results are the bytes of the default-stream run."""
    sc, maps = _scene_run(cuda_device)
    got0, _, (pf, ps, uv_a, uv_b) = _lifted(cuda_device)
    pairs = [(0, 1), (1, 0)]
    ratio0, counts0 = F.covisibility(maps, sc["poses"], pairs)
    torch.cuda.synchronize()
    depth = torch.from_numpy(sc["depth"]).to(cuda_device)
    mask = torch.from_numpy(sc["mask"]).to(cuda_device)
    s = torch.cuda.Stream(device=cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        m = F.prepare_frames(depth, sc["K"], mask)
        lifted = F.lift_matches(m, pf, uv_a, uv_b, ps)
        ratio, counts = F.covisibility(m, sc["poses"], pairs)
    s.synchronize()
    for k in ("depth", "points", "normals", "n_valid"):
        _same(_np(getattr(m, k)), _np(getattr(maps, k)), k)
    _same(_np(lifted.pts_a), _np(got0.pts_a), "pts_a")
    _same(_np(lifted.valid), _np(got0.valid), "valid")
    _same(_np(counts), _np(counts0), "counts")


def test_hand_over_to_the_pose_graph(cuda_device):
    """MeshRenderer depth of the synthetic mesh at 3 known poses -> prepare_frames -> optimize_poses (dense
    term only) from the true poses: finite poses and dense correspondences at every linearisation. The
    drift from the true poses is recorded in profiles/r18/frame_maps.json by scripts/frame_maps.py with
    this same function; no bound is derived for it, so it is printed and not asserted."""
    from scripts.frame_maps import hand_over
    res = hand_over(cuda_device)
    print("hand-over:", json.dumps(res))
    assert res["poses_finite"]
    assert all(c > 0 for c in res["dense_correspondences"]) and len(res["dense_correspondences"]) == res["n_outer"] + 1
    assert all(v > 0 for v in res["n_valid"])
