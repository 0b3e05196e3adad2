"""GPU: nof_mask_roi and nof_warp_images against tests/pair_crop_oracle.py, exactly (integers for the ROI, every
bit of the float32 crops and the uint8 cells for the warp), pair_crops against pair_transforms plus the oracle
warp, and find_corres against its composition written out by hand.

The crops are compared bit for bit: csrc/pair_crop.hip is compiled without contraction and states the order
of every float64 operation, and numpy evaluates the oracle's operations one by one in that order."""
import numpy as np
import pytest
import torch

from tests import pair_crop_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(cuda_device):
    from bundlesdf_amd import pairs
    return pairs


@pytest.fixture(scope="module")
def data():
    """(form -> images, masks), computed once and left unchanged."""
    return O.sources()


# ---- mask_roi --------------------------------------------------------------------------------------------

def test_mask_roi_equals_the_oracle(P, cuda_device):
    named = O.roi_masks()                      # corner_br is the frame whose only pixel is (52, 36): the last
    masks = np.stack(list(named.values()))     # column of a partial block and the last row of the second block
    assert masks.shape[1:] == (37, 53) and named["corner_br"][36, 52] and named["corner_br"].sum() == 1
    want_roi, want_n = O.mask_roi(masks)
    roi, count = P.mask_roi(masks, device=cuda_device)
    assert roi.dtype == torch.int32 and count.dtype == torch.int32 and roi.is_cuda and count.is_cuda
    np.testing.assert_array_equal(roi.cpu().numpy(), want_roi)
    np.testing.assert_array_equal(count.cpu().numpy(), want_n)
    again = P.mask_roi(masks, device=cuda_device)
    assert torch.equal(again[0], roi) and torch.equal(again[1], count)
    # input forms: bool and int64 tensors on the device, one [H,W] mask
    for m in (torch.from_numpy(masks != 0).to(cuda_device), torch.from_numpy(masks.astype(np.int64) * -3).to(cuda_device)):
        r, c = P.mask_roi(m)
        assert torch.equal(r, roi) and torch.equal(c, count)
    r1, c1 = P.mask_roi(named["blobs"], device=cuda_device)
    assert r1.tolist() == [5, 46, 3, 30] and int(c1) == 6 * 6 + 11 * 14


def test_mask_roi_of_several_blocks_and_of_no_frame(P, data, cuda_device):
    masks = np.concatenate([data[1], np.ones((1, 48, 64), np.uint8)])          # 48 rows: two blocks of 32 rows
    roi, count = P.mask_roi(masks, device=cuda_device)
    want_roi, want_n = O.mask_roi(masks)
    np.testing.assert_array_equal(roi.cpu().numpy(), want_roi)
    np.testing.assert_array_equal(count.cpu().numpy(), want_n)
    assert want_roi[2].tolist() == [64, -1, 48, -1] and want_n[2] == 0
    roi0, count0 = P.mask_roi(np.zeros((0, 37, 53), np.uint8), device=cuda_device)
    assert tuple(roi0.shape) == (0, 4) and tuple(count0.shape) == (0,)
    with pytest.raises(ValueError, match="masks"):
        P.mask_roi(np.zeros((2, 37, 53), np.float32), device=cuda_device)


# ---- warp_images -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("form", [O.GREY_U8, O.GREY_F32, O.RGB_U8])
@pytest.mark.parametrize("S", [32, 40, 64])                 # 40: a last tile of 8 columns, an odd count of cells
def test_warp_images_equals_the_oracle_bit_for_bit(P, data, cuda_device, S, form, masked):
    srcs, masks = data
    inv, frames = O.warp_cases(S)
    m = masks if masked else None
    want, want_cells = O.warp(srcs[form], inv, frames, S, m)
    got, cells = P.warp_images(torch.from_numpy(srcs[form]).to(cuda_device), inv, frames, S, masks=m)
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, S, S)
    assert cells.dtype == torch.uint8 and tuple(cells.shape) == (6, S // 8, S // 8)
    g = got.cpu().numpy()
    for q in range(6):
        assert np.array_equal(g[q].view(np.uint32), want[q].view(np.uint32)), \
            (q, float(np.abs(g[q].astype(np.float64) - want[q]).max()))
    np.testing.assert_array_equal(cells.cpu().numpy(), want_cells)
    # the cases are what they claim to be
    assert not want[3].any() and not want_cells[3].any()            # wholly outside the image
    assert not want[5].any() and not want_cells[5].any()            # frames[5] = 7 does not exist
    if not masked:
        assert want[0].any() and want[1].any() and want[2].any() and want[4].any()
        assert want_cells[0].all() == (S <= 48)                     # the identity crop of 64 rows leaves the 48-row image
        assert not want_cells[4].all() and want_cells[4].any()      # the down-scaled image ends inside the crop


def test_warp_images_input_forms_and_refusals(P, data, cuda_device):
    srcs, masks = data
    inv, frames = O.warp_cases(32)
    base, base_cells = P.warp_images(torch.from_numpy(srcs[O.GREY_U8]).to(cuda_device), inv, frames, 32, masks=masks)
    same, none = P.warp_images(srcs[O.GREY_U8], torch.from_numpy(inv), torch.from_numpy(frames), 32,
                               masks=torch.from_numpy(masks != 0).to(cuda_device), cell_masks=False)
    assert none is None and torch.equal(same, base)
    empty, empty_cells = P.warp_images(srcs[O.GREY_U8], inv[:0], frames[:0], 32)
    assert tuple(empty.shape) == (0, 32, 32) and tuple(empty_cells.shape) == (0, 4, 4)
    with pytest.raises(ValueError, match="images"):
        P.warp_images(srcs[O.GREY_U8].astype(np.float64), inv, frames, 32)
    with pytest.raises(ValueError, match="inv"):
        P.warp_images(srcs[O.GREY_U8], inv[:, :, :2], frames, 32)
    with pytest.raises(ValueError, match="masks"):
        P.warp_images(srcs[O.GREY_U8], inv, frames, 32, masks=masks[:2])
    with pytest.raises(ValueError, match="out_size"):
        P.warp_images(srcs[O.GREY_U8], inv, frames, 36)


# ---- pair_crops ------------------------------------------------------------------------------------------

def _rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _poses(angles):
    tilt = np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    T = np.tile(np.eye(4), (len(angles), 1, 1))
    for f, a in enumerate(angles):
        T[f, :3, :3] = tilt @ _rz(a)
        T[f, :3, 3] = (0.01 * f, -0.02 * f, 0.5)
    return T


@pytest.mark.parametrize("form", [O.GREY_F32, O.RGB_U8])
def test_pair_crops_equals_the_transforms_and_the_oracle_warp(P, data, cuda_device, form):
    """Three pairs over three frames: (0, 1) turned by 50 degrees, (1, 0) with frame 1 in a second pair, and
    (1, 2) whose frame 2 has an empty mask."""
    srcs, masks = data
    assert not masks[2].any()
    poses = _poses([0.0, 50.0, 20.0])
    pairs = np.array([(0, 1), (1, 0), (1, 2)])
    S, margin = 64, 10
    pc = P.pair_crops(torch.from_numpy(srcs[form]).to(cuda_device), masks, poses, pairs, out_size=S, margin=margin)

    roi, count = O.mask_roi(masks)
    np.testing.assert_array_equal(pc.roi.cpu().numpy(), roi)
    np.testing.assert_array_equal(pc.count.cpu().numpy(), count)
    tf_a, tf_b, valid = P.pair_transforms(np.concatenate([roi, count[:, None]], 1), poses, pairs, 48, 64, S, margin)
    assert valid.tolist() == [True, True, False] and pc.valid.tolist() == valid.tolist()
    np.testing.assert_array_equal(pc.tf_a, tf_a)
    np.testing.assert_array_equal(pc.tf_b, tf_b)
    assert abs(np.degrees(np.arctan2(tf_b[0][1, 0], tf_b[0][0, 0])) - 50.0) < 1e-9
    np.testing.assert_array_equal(pc.match_pairs, [(0, 1), (2, 3), (4, 5)])
    inv = P.invert_affine(np.stack([tf_a, tf_b], 1).reshape(6, 3, 3))
    frames = np.array([0, 1, 1, 0, -1, -1])
    want, want_cells = O.warp(srcs[form], inv, frames, S, masks)
    got = pc.images.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (6, S, S)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(pc.cells.cpu().numpy(), want_cells)
    assert want[:4].reshape(4, -1).any(1).all() and want_cells[:4].reshape(4, -1).any(1).all()
    assert not got[4:].any() and not pc.cells[4:].any()              # the invalid pair
    assert P.pair_crops(srcs[form], masks, poses, pairs, out_size=S, cell_masks=False).cells is None


# ---- find_corres -----------------------------------------------------------------------------------------

def test_find_corres_equals_its_composition(P, data, cuda_device):
    from bundlesdf_amd.frames import lift_matches, prepare_frames
    from bundlesdf_amd.loftr import Loftr
    from bundlesdf_amd.ransac import ransac_pairs
    from tests.test_gpu_backbone import _matcher_weights
    dev = cuda_device
    srcs, _ = data
    grey = torch.from_numpy(srcs[O.GREY_F32]).to(dev)
    masks = np.zeros((3, 48, 64), np.uint8)
    masks[0, 6:44, 8:58] = 1
    masks[1, 4:40, 10:60] = 1
    masks[2, 8:46, 4:52] = 1
    v, u = np.meshgrid(np.arange(48.0), np.arange(64.0), indexing="ij")
    depth = np.stack([0.5 + 0.0003 * u + 0.0002 * v + 0.002 * f for f in range(3)]).astype(np.float32)
    K = np.array([[60.0, 0.0, 31.5], [0.0, 60.0, 23.5], [0.0, 0.0, 1.0]])
    maps = prepare_frames(depth, K, masks, device=dev)
    assert int(maps.n_valid.min()) > 500
    poses = _poses([0.0, 15.0, -10.0])
    pairs = np.array([(0, 1), (1, 2), (2, 0)])
    matcher = Loftr.from_state_dict(_matcher_weights(), device=dev)
    rk = dict(inlier_dist=0.05, normal_angle_deg=30.0, n_trials=64, min_inliers=3, seed=3)
    S = 64

    got = P.find_corres(matcher, grey, masks, maps, poses, pairs, out_size=S, thr=0.0, border_rm=0, ransac=rk)

    pc = P.pair_crops(grey, masks, poses, pairs, S, 10, True)
    assert pc.valid.all() and pc.cells.reshape(6, -1).any(1).all()       # at least one cell per side
    fm = matcher.match(pc.images, pc.match_pairs, pc.cells, thr=0.0, border_rm=0, temperature=0.1)
    uv_a, uv_b, pair_start, conf = fm.to_pixels(scale=8, tf_a=pc.tf_a, tf_b=pc.tf_b)
    lifted = lift_matches(maps, pairs, uv_a, uv_b, pair_start, poses=poses, max_dist=None, max_normal_deg=None).compact()
    res = ransac_pairs(lifted.pts_a, lifted.pts_b, lifted.pair_start, lifted.normals_a, lifted.normals_b,
                       conf=conf[lifted.rows].double(), **rk)

    n_raw = got.n_raw.cpu().numpy()
    print("find_corres: n_raw", n_raw.tolist(), "lifted", np.diff(got.lifted.pair_start.cpu().numpy()).tolist(),
          "inliers", got.ransac.n_inliers.tolist())
    assert (n_raw >= 1).all()                                            # an empty result cannot pass for agreement
    np.testing.assert_array_equal(n_raw, np.diff(pair_start.cpu().numpy()))
    assert torch.equal(got.crops.images, pc.images) and torch.equal(got.crops.cells, pc.cells)
    assert got.uv_a.dtype == torch.float64 and torch.equal(got.uv_a, uv_a) and torch.equal(got.uv_b, uv_b)
    assert torch.equal(got.pair_start, pair_start) and torch.equal(got.conf, conf)
    for name in ("rows", "pair_start", "pts_a", "pts_b", "normals_a", "normals_b", "valid", "pair_frames"):
        assert torch.equal(getattr(got.lifted, name), getattr(lifted, name)), name
    for name in ("inlier", "n_inliers", "best_trial", "pose", "score"):
        assert torch.equal(getattr(got.ransac, name), getattr(res, name)), name
    # without a dict there is no RANSAC, and cell_masks=False runs the matcher without a mask
    bare = P.find_corres(matcher, grey, masks, maps, poses, pairs, out_size=S, thr=0.0, border_rm=0, cell_masks=False)
    assert bare.ransac is None and bare.crops.cells is None and torch.equal(bare.crops.images, pc.images)
    plain = matcher.match(pc.images, pc.match_pairs, None, thr=0.0, border_rm=0)
    assert torch.equal(bare.fine.expec, plain.expec) and torch.equal(bare.fine.j, plain.j)
