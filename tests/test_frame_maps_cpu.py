"""CPU: the frame-map oracle (tests/frame_maps_oracle.py) on its own scene, and the validation of
bundlesdf_amd.frames, which raises before any device work."""
import ctypes

import numpy as np
import pytest
import torch

from tests import frame_maps_oracle as O


def test_plane_normals_are_exact():
    """Fronto-parallel plane: row_dir = (0, a, 0), col_dir = (b, 0, 0), (0,a,0) x (b,0,0) = (0,0,-ab), and
    sqrt((ab)^2) = |ab| exactly, so every interior normal is (0,0,-1) and n . P/|P| = -z/|P|, far from
    sin(10 deg): nothing is edge-filtered."""
    d, K = O.plane_scene()
    br = {}
    depth, points, normals, n_valid = O.geometry(d, K, branches=br)
    assert np.array_equal(normals[0, 1:-1, 1:-1], np.broadcast_to(np.float32([0, 0, -1]), (7, 9, 3)))
    assert (normals[0, 0] == 0).all() and (normals[0, :, 0] == 0).all()
    assert br["edge_drop"] == 0 and n_valid[0] == d.size and np.array_equal(depth, d)


def test_every_branch_fires_on_the_scene():
    sc = O.scene()
    br = {}
    out = O.prepare(sc["depth"], sc["K"], sc["mask"], branches=br)
    for name in ("erode_centre_drop", "erode_ratio_drop", "erode_keep", "bilateral_empty", "bilateral_hole_fill",
                 "bilateral_band_reject", "normal_row_central", "normal_row_forward", "normal_row_backward",
                 "normal_row_none", "normal_col_central", "normal_col_forward", "normal_col_backward", "normal_col_none",
                 "normal_flip", "edge_drop", "zero_normal_keep", "mask_drop"):
        assert br[name] > 0, name
    e, b = out["eroded"], out["bilateral"][-1]
    p = sc["planted"]
    for name in ("speckle", "beyond_zfar", "below_min", "negative", "nan", "inf", "hole"):
        for f, v, u in p[name]:
            assert e[f, v, u] == 0, (name, f, v, u)          # the erode pass drops each planted defect
    for f, v, u in p["hole"]:
        assert b[f, v, u] > 0.1                               # and the bilateral passes fill the single holes
    assert np.isfinite(out["depth"]).all() and np.isfinite(out["points"]).all() and np.isfinite(out["normals"]).all()
    assert out["n_valid"][2] == 0 and (out["n_valid"][:2] > 500).all()
    assert (out["depth"][sc["mask"] == 0] == 0).all()
    assert ((out["points"] == 0).all(-1) == (out["depth"] == 0)).all()
    length = np.linalg.norm(out["normals"].astype(np.float64), axis=-1)
    assert (np.abs(length[length > 0] - 1) < 1e-6).all()


def test_round_is_half_away_from_zero():
    x = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 3.49, -3.51, 0.49999999999999994, -0.49999999999999994, 7.0])
    assert O.c_round(x).tolist() == [1.0, -1.0, 2.0, 3.0, -3.0, 3.0, -4.0, 0.0, -0.0, 7.0]
    assert np.round(2.5) == 2.0                               # what numpy does instead


def test_relative_poses_restated():
    from bundlesdf_amd import frames as F
    sc = O.scene()
    pairs = [(a, b) for a in range(3) for b in range(3)]
    T = F.relative_poses(sc["poses"], pairs)
    for q, (a, b) in enumerate(pairs):
        assert T[q].tobytes() == O.relative_pose(sc["poses"][a], sc["poses"][b]).tobytes()
        assert np.allclose(T[q], np.linalg.inv(sc["poses"][b]) @ sc["poses"][a], atol=1e-15)


def _cpu_maps(n=2, h=6, w=7):
    from bundlesdf_amd import frames as F
    return F.FrameMaps(depth=torch.zeros(n, h, w), points=torch.zeros(n, h, w, 3), normals=torch.zeros(n, h, w, 3),
                       n_valid=torch.zeros(n, dtype=torch.int32), K=np.eye(3))


def test_wrappers_validate_before_device_work():
    """No device here: each of these must raise ValueError, not reach the library."""
    from bundlesdf_amd import frames as F
    d = np.full((2, 6, 7), 0.5, np.float32)
    K = np.array([[100.0, 0, 3], [0, 100.0, 3], [0, 0, 1]])
    skew = K.copy()
    skew[0, 1] = 0.5
    bad = [lambda: F.prepare_frames(np.zeros(5, np.float32), K),
           lambda: F.prepare_frames(np.zeros((1, 2, 3, 4), np.float32), K),
           lambda: F.prepare_frames(d, np.eye(4)),
           lambda: F.prepare_frames(d, np.stack([K] * 3)),
           lambda: F.prepare_frames(d, skew),
           lambda: F.depth_geometry(d, skew),
           lambda: F.prepare_frames(d, K, mask=np.ones((2, 6, 8), np.uint8)),
           lambda: F.prepare_frames(d, K, erode_radius=9),
           lambda: F.prepare_frames(d, K, bilateral_radius=9),
           lambda: F.prepare_frames(d, K, bilateral_radius=-1),
           lambda: F.prepare_frames(d, K, bilateral_passes=-1),
           lambda: F.prepare_frames(d, K, sigma_d=0.0),
           lambda: F.prepare_frames(d, K, z_diff=float("nan")),
           lambda: F.erode_depth(d, radius=9),
           lambda: F.bilateral_depth(d, radius=9),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1]], np.zeros((4, 2)), np.zeros((3, 2))),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1], [1, 0]], np.zeros((4, 2)), np.zeros((4, 2))),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1], [1, 0]], np.zeros((4, 2)), np.zeros((4, 2)), [0, 2, 3]),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1], [1, 0]], np.zeros((4, 2)), np.zeros((4, 2)), [0, 3, 2, 4]),
           lambda: F.lift_matches(_cpu_maps(), [[0, 2]], np.zeros((4, 2)), np.zeros((4, 2))),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1]], np.zeros((4, 3)), np.zeros((4, 3))),
           lambda: F.lift_matches(_cpu_maps(), [[0, 1]], np.zeros((4, 2)), np.zeros((4, 2)), max_dist=0.1),
           lambda: F.covisibility(_cpu_maps(), np.tile(np.eye(4), (2, 1, 1)), [[0, 1]], stride=-2),
           lambda: F.covisibility(_cpu_maps(), np.tile(np.eye(4), (2, 1, 1)), [[0, 1]], stride=0),
           lambda: F.covisibility(_cpu_maps(), np.tile(np.eye(4), (3, 1, 1)), [[0, 1]]),
           lambda: F.covisibility(_cpu_maps(), np.tile(np.eye(4), (2, 1, 1)), [[0, 2]])]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} did not raise")


def test_library_refuses_bad_descriptors_before_device_work():
    """Each group-10 entry point returns NOF_EINVAL and names the field on a machine with no GPU."""
    from bundlesdf_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes first
    for fn, desc, setup, word in (
            (L.nof_frame_erode, _lib.FrameErodeDesc, dict(N=1, H=4, W=4, radius=9), b"radius=9"),
            (L.nof_frame_erode, _lib.FrameErodeDesc, dict(N=0, H=4, W=4), b"N=0"),
            (L.nof_frame_erode, _lib.FrameErodeDesc, dict(N=1, H=4, W=4, radius=1), b"in is NULL"),
            (L.nof_frame_bilateral, _lib.FrameBilateralDesc, dict(N=1, H=4, W=0), b"W=0"),
            (L.nof_frame_bilateral, _lib.FrameBilateralDesc, dict(N=1, H=4, W=4, radius=2, in_=one, out=one), b"same buffer"),
            (L.nof_frame_geometry, _lib.FrameGeometryDesc, dict(N=1, H=4, W=4, depth_in=one), b"K is NULL"),
            (L.nof_frame_geometry, _lib.FrameGeometryDesc, dict(N=70000, H=40000, W=4), b"N=70000"),
            (L.nof_frame_lift_matches, _lib.FrameLiftDesc, dict(N=1, H=4, W=4, P=0), b"P=0"),
            (L.nof_frame_lift_matches, _lib.FrameLiftDesc, dict(N=1, H=4, W=4, P=1, M=2, gate_dist=1), b"poses is NULL"),
            (L.nof_frame_covisibility, _lib.FrameCovisDesc, dict(N=1, H=4, W=4, Q=1, stride=0), b"stride=0")):
        D = desc()
        for k, v in setup.items():
            setattr(D, k, v)
        assert fn(ctypes.byref(D), None) != 0
        assert word in L.nof_last_error(), (word, L.nof_last_error())
    assert L.nof_frame_erode(None, None) != 0 and b"desc is NULL" in L.nof_last_error()
