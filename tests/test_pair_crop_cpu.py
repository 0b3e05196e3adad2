"""CPU: the host half of bundlesdf_amd.pairs (rotate_image_transform, pair_transforms, invert_affine, the
refusals) against values worked out by hand from the reference's source, and tests/pair_crop_oracle.py
against brute force and an exact case. Nothing here launches a kernel."""
import numpy as np
import pytest

from tests import pair_crop_oracle as O


def _P():
    from bundlesdf_amd import pairs
    return pairs


def _rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rx(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _pose(R, t=(0.1, -0.2, 0.7)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _apply(tf, u, v):
    return np.array([tf[0, 0] * u + tf[0, 1] * v + tf[0, 2], tf[1, 0] * u + tf[1, 1] * v + tf[1, 2]])


# ---- ROI oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(O.roi_masks()))
def test_roi_oracle_against_brute_force(name):
    m = O.roi_masks()[name]
    assert m.shape == (37, 53)
    roi, count = O.mask_roi(m[None])
    want_roi, want_n = O.mask_roi_brute(m)
    assert tuple(roi[0]) == want_roi and int(count[0]) == want_n
    assert roi.dtype == np.int32 and count.dtype == np.int32


def test_roi_oracle_known_values():
    m = O.roi_masks()
    roi, count = O.mask_roi(np.stack([m["empty"], m["full"], m["corner_br"], m["blobs"]]))
    assert roi.tolist() == [[53, -1, 37, -1], [0, 52, 0, 36], [52, 52, 36, 36], [5, 46, 3, 30]]
    assert count.tolist() == [0, 37 * 53, 1, 6 * 6 + 11 * 14]


# ---- rotate_image_transform ------------------------------------------------------------------------------

def test_rotate_image_transform_without_rotation_is_a_translation():
    """Utils.cpp:417-443 with rot = 0, H = 480, W = 640: the centre (320, 240) goes to the origin, the corners
    span 640 x 480, side = 640, and the re-centring adds (320, 320): u' = u, v' = v + 80."""
    tf = _P().rotate_image_transform(480, 640, 0.0)
    np.testing.assert_array_equal(tf, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 80.0], [0.0, 0.0, 1.0]]))


def test_rotate_image_transform_quarter_turn_keeps_the_corners_inside():
    H, W = 480, 640
    tf = _P().rotate_image_transform(H, W, np.pi / 2)
    side = 640                                                     # the turned image spans 480 x 640
    np.testing.assert_allclose(tf[:2, :2], [[0.0, -1.0], [1.0, 0.0]], atol=1e-15)
    for u, v in [(0, 0), (W, 0), (0, H), (W, H)]:
        p = _apply(tf, u, v)
        assert (p >= -1e-9).all() and (p <= side + 1e-9).all(), (u, v, p)
    np.testing.assert_allclose(_apply(tf, W / 2, H / 2), [side / 2, side / 2], atol=1e-12)


# ---- pair_transforms -------------------------------------------------------------------------------------

def test_pair_transforms_translation_only_pair():
    P = _P()
    roi = np.array([[50, 230, 40, 160], [80, 260, 60, 180]])
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # R^T R is the identity exactly
    poses = np.stack([_pose(quarter), _pose(quarter, (0.4, 0.0, 0.6))])
    tf_a, tf_b, valid = P.pair_transforms(roi, poses, [(0, 1)], 480, 640, out_size=400, margin=10)
    assert valid.tolist() == [True]
    # WA = 230 - 50 + 20 = 200, HA = 160 - 40 + 20 = 140, the same for B: max_dim = 200, both scales 400 / 200
    np.testing.assert_array_equal(tf_a[0], [[2.0, 0.0, -80.0], [0.0, 2.0, -60.0], [0.0, 0.0, 1.0]])
    np.testing.assert_array_equal(_apply(tf_a[0], 40, 30), [0.0, 0.0])
    np.testing.assert_array_equal(_apply(tf_a[0], 50, 40), [20.0, 20.0])
    # B: identical poses, so rot = 0 and rotate_image_transform shifts v by 80 before the box is taken
    np.testing.assert_array_equal(tf_b[0][:2, :2], [[2.0, 0.0], [0.0, 2.0]])
    np.testing.assert_array_equal(_apply(tf_b[0], 80, 60), [20.0, 20.0])
    np.testing.assert_array_equal(_apply(tf_b[0], 260, 180), [380.0, 260.0])


@pytest.mark.parametrize("theta", [20.0, -75.0, 140.0])
def test_pair_transforms_rotated_pair(theta):
    """Poses that differ by Rz(theta) about the camera axis: R_b = R_a Rz(theta), so R_BA = R_a^T R_b =
    Rz(theta), rot = theta, and getRotateImageTransform's block [[cos, -sin], [sin, cos]] turns B's pixels
    by +theta: the linear part of tf_b is s [[cos, -sin], [sin, cos]]."""
    from scipy.spatial.transform import Rotation
    P = _P()
    Ra = _rz(31.0) @ _rx(-50.0)
    poses = np.stack([_pose(Ra), _pose(Ra @ _rz(theta), (0.3, 0.0, 0.5))])
    R_BA = poses[0][:3, :3].T @ poses[1][:3, :3]
    want_rot = Rotation.from_matrix(R_BA).as_rotvec()[2]
    assert abs(P.rotation_about_axis_z(R_BA) - want_rot) <= 1e-12
    assert abs(want_rot - np.radians(theta)) <= 1e-12
    roi = np.array([[200, 420, 150, 330], [180, 400, 120, 260]])
    margin = 10
    tf_a, tf_b, valid = P.pair_transforms(roi, poses, [(0, 1)], 480, 640, out_size=400, margin=margin)
    assert valid.all()
    L = tf_b[0][:2, :2]
    s = np.sqrt(L[0, 0] ** 2 + L[1, 0] ** 2)
    c, sn = np.cos(np.radians(theta)), np.sin(np.radians(theta))
    np.testing.assert_allclose(L, s * np.array([[c, -sn], [sn, c]]), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(tf_b[0][2], [0.0, 0.0, 1.0])
    # The turned ROI's bounding box starts at margin s on both axes. Its longer side e is scaled by s =
    # 400 / trunc(e + 2 margin), so it ends at s (e + 2 margin) - margin s: 400 - margin s, plus what the
    # truncation of WB / HB to an integer cut off, which is less than one source pixel = s crop pixels.
    ub0, ub1, vb0, vb1 = roi[1]
    pts = np.array([_apply(tf_b[0], u, v) for u in (ub0, ub1) for v in (vb0, vb1)])
    lo, hi = pts.min(0), pts.max(0)
    np.testing.assert_allclose(lo, [margin * s, margin * s], rtol=0, atol=1e-9)
    longer = int(np.argmax(hi - lo))
    assert 400 - margin * s - 1e-9 <= hi[longer] < 400 - margin * s + s
    assert hi[1 - longer] <= hi[longer]
    # A is not turned, and its longer side (WA = 240) fills the crop too
    sa = tf_a[0][0, 0]
    assert abs(sa - 400.0 / 240.0) <= 1e-12
    np.testing.assert_array_equal(tf_a[0][:2, :2], [[sa, 0.0], [0.0, sa]])


def test_out_of_plane_rotation_takes_the_rotation_vectors_z_not_the_yaw():
    """A 30 degree tilt about x combined with 40 degrees about z: rot is the z component of the rotation
    vector of R_BA, which is not 40 degrees."""
    from scipy.spatial.transform import Rotation
    P = _P()
    R_BA = _rx(30.0) @ _rz(40.0)
    want = Rotation.from_matrix(R_BA).as_rotvec()[2]
    got = P.rotation_about_axis_z(R_BA)
    assert abs(got - want) <= 1e-12
    assert abs(got - np.radians(40.0)) > 1e-2
    # and it is what pair_transforms turns B by
    poses = np.stack([_pose(np.eye(3)), _pose(R_BA)])
    roi = np.array([[200, 420, 150, 330], [180, 400, 120, 260]])
    _, tf_b, _ = P.pair_transforms(roi, poses, [(0, 1)], 480, 640)
    assert abs(np.arctan2(tf_b[0][1, 0], tf_b[0][0, 0]) - want) <= 1e-12


def test_rotation_about_axis_z_beyond_a_half_turn_of_trace():
    """The quaternion branch for a trace <= 0 (angles near pi) agrees with scipy too."""
    from scipy.spatial.transform import Rotation
    for R in (_rz(170.0), _rz(-179.0) @ _rx(5.0), _rx(175.0) @ _rz(20.0), _rz(91.0) @ _rx(120.0)):
        want = Rotation.from_matrix(R).as_rotvec()[2]
        assert abs(_P().rotation_about_axis_z(R) - want) <= 1e-12
    assert _P().rotation_about_axis_z(np.eye(3)) == 0.0


def test_invert_affine_composes_to_the_identity():
    P = _P()
    Ra = _rz(31.0) @ _rx(-50.0)
    poses = np.stack([_pose(Ra), _pose(Ra @ _rz(-75.0))])
    roi = np.array([[200, 420, 150, 330], [180, 400, 120, 260]])
    tf_a, tf_b, _ = P.pair_transforms(roi, poses, [(0, 1), (1, 0)], 480, 640)
    for tf in list(tf_a) + list(tf_b):
        inv = P.invert_affine(tf)
        assert inv.shape == (2, 3)
        full = np.vstack([inv, [0.0, 0.0, 1.0]])
        np.testing.assert_allclose(full @ tf, np.eye(3), rtol=0, atol=1e-12)
    assert P.invert_affine(np.stack([tf_a, tf_b], 1)).shape == (2, 2, 2, 3)
    with pytest.raises(ValueError, match="singular"):
        P.invert_affine(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="not finite"):
        P.invert_affine(np.array([[1.0, np.nan, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="affine"):
        P.invert_affine(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1e-3, 0.0, 1.0]]))


# ---- refusals --------------------------------------------------------------------------------------------

def test_an_empty_mask_makes_its_pairs_invalid():
    P = _P()
    masks = np.zeros((3, 48, 64), np.uint8)
    masks[0, 10:30, 12:40] = 1
    masks[1, 5:25, 20:50] = 1
    roi, count = O.mask_roi(masks)
    poses = np.stack([_pose(np.eye(3)), _pose(_rz(50.0)), _pose(_rz(10.0))])
    for r in (np.concatenate([roi, count[:, None]], 1), roi):            # with the count column and without
        tf_a, tf_b, valid = P.pair_transforms(r, poses, [(0, 1), (1, 2), (2, 0)], 48, 64, out_size=64)
        assert valid.tolist() == [True, False, False]
        for p in (1, 2):
            np.testing.assert_array_equal(tf_a[p], np.eye(3))
            np.testing.assert_array_equal(tf_b[p], np.eye(3))
        assert not np.array_equal(tf_a[0], np.eye(3))


def test_refusals_name_the_argument():
    P = _P()
    roi = np.array([[5, 20, 5, 20], [5, 20, 5, 20]])
    poses = np.stack([np.eye(4)] * 2)
    with pytest.raises(ValueError, match="margin"):
        P.pair_transforms(roi, poses, [(0, 1)], 48, 64, margin=0)
    with pytest.raises(ValueError, match="margin"):                 # before anything else: the other arguments are junk
        P.pair_transforms("junk", None, None, 48, 64, margin=0)
    with pytest.raises(ValueError, match="margin"):
        P.pair_crops("junk", None, None, None, margin=0)
    bad = poses.copy()
    bad[1, 0, 0] = np.inf
    with pytest.raises(ValueError, match="poses"):
        P.pair_transforms(roi, bad, [(0, 1)], 48, 64)
    for size in (60, 0, 4104):
        with pytest.raises(ValueError, match="out_size"):
            P.pair_transforms(roi, poses, [(0, 1)], 48, 64, out_size=size)
    with pytest.raises(ValueError, match="out_size"):
        P.warp_images(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 2, 3)), [0], 60)
    with pytest.raises(ValueError, match="out_size"):
        P.pair_crops("junk", None, None, None, out_size=60)
    with pytest.raises(ValueError, match="pairs"):
        P.pair_transforms(roi, poses, [(0, 2)], 48, 64)


# ---- warp oracle -----------------------------------------------------------------------------------------

def test_warp_oracle_on_the_exact_scale_2_case():
    """A 48 x 64 uint8 source through a scale-2 transform onto integer offsets (crop (x, y) reads source
    (x / 2 - 3, y / 2 - 2)): even-even pixels are source / 255 rounded once, odd pixels the float64 mean of
    their two or four neighbours rounded once, and pixels that map outside the image are 0."""
    src = O.sources()[0][O.GREY_U8][:1]
    H, W = src.shape[1:]
    S = 64
    inv = O.scale2_inverse(-3, -2)[None]
    out, cells = O.warp(src, inv, [0], S)
    assert out.dtype == np.float32 and out.shape == (1, S, S) and cells.shape == (1, 8, 8)
    v = np.zeros((H + 2, W + 2))                                     # the source in float64 with a border of zeros
    v[1:-1, 1:-1] = src[0].astype(np.float64) / 255.0

    def at(u, r):                                                    # value at source (u, r), 0 outside
        return v[r + 1, u + 1] if -1 <= u <= W and -1 <= r <= H else 0.0

    checked = {"even": 0, "odd": 0, "outside": 0}
    for y in range(S):
        for x in range(S):
            u, r = x // 2 - 3, y // 2 - 2                            # floor of the source coordinate
            if x % 2 == 0 and y % 2 == 0:
                want, kind = at(u, r), "even"
            elif y % 2 == 0:
                want, kind = (at(u, r) + at(u + 1, r)) / 2, "odd"
            elif x % 2 == 0:
                want, kind = (at(u, r) + at(u, r + 1)) / 2, "odd"
            else:
                want, kind = ((at(u, r) + at(u + 1, r)) / 2 + (at(u, r + 1) + at(u + 1, r + 1)) / 2) / 2, "odd"
            if x / 2 - 3 <= -1 or y / 2 - 2 <= -1:
                want, kind = 0.0, "outside"
            assert out[0, y, x] == np.float32(want), (x, y, kind)
            checked[kind] += 1
    assert min(checked.values()) > 100
    # cells: a cell is seen iff one of its pixels' nearest source pixel is inside the image
    assert cells[0, 0, 0] == 1 and cells.all()                      # every 8 x 8 cell reaches x / 2 - 3 + 0.5 >= 0
    far, far_cells = O.warp(src, np.array([[[1.0, 0.0, 500.0], [0.0, 1.0, -900.0]]]), [0], S)
    assert not far.any() and not far_cells.any()


def test_warp_oracle_mask_and_missing_frame():
    srcs, masks = O.sources()
    ident = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]] * 2)
    out, cells = O.warp(srcs[O.GREY_F32], ident, [0, 7], 32, masks)
    np.testing.assert_array_equal(out[0], np.where(masks[0, :32, :32] != 0, srcs[O.GREY_F32][0, :32, :32], 0))
    np.testing.assert_array_equal(cells[0], (masks[0, :32, :32] != 0).reshape(4, 8, 4, 8).any(axis=(1, 3)))
    assert not out[1].any() and not cells[1].any()
    rgb, _ = O.warp(srcs[O.RGB_U8], ident[:1], [1], 32)
    a = srcs[O.RGB_U8][1, :32, :32].astype(np.float64)
    want = (((0.2989 * a[..., 0] + 0.587 * a[..., 1]) + 0.114 * a[..., 2]) / 255.0).astype(np.float32)
    np.testing.assert_array_equal(rgb[0], want)
