"""CPU: tests/match_oracle.py (the float64 restatement of csrc/match.hip's definition) against a torch
float64 route that materialises the confidence matrix as the reference's matching head does and against
the recorded output of that head (tests/golden/coarse_match.npz); its tie and empty-row rules;
CoarseMatches.to_pixels; and the argument validation of match_descriptors and nof_match_descriptors,
which all happens before the first device call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bundlesdf_amd import _lib
from bundlesdf_amd import matching as M
from tests import match_oracle as O


def _materialised(a, b, hw_a, hw_b, va=None, vb=None, temperature=0.1, thr=0.2, border_rm=2):
    """The reference's route in torch float64: scaled features, einsum, two softmaxes, product, threshold,
    border, the == mutual test, max over dim 2 (coarse_matching.py:109-119, 175-196). -> b_ids, i_ids, j_ids, mconf."""
    f0, f1 = torch.from_numpy(a.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
    C = f0.shape[-1]
    f0, f1 = f0 / C ** .5, f1 / C ** .5
    sim = torch.einsum("nlc,nsc->nls", f0, f1) / float(np.float32(temperature))
    if va is not None:
        ok = torch.from_numpy(va != 0)[..., None] & torch.from_numpy(vb != 0)[:, None]
        sim = sim.masked_fill(~ok, -1e9)
    conf = torch.softmax(sim, 1) * torch.softmax(sim, 2)
    P, (h0, w0), (h1, w1) = conf.shape[0], hw_a, hw_b
    mask = (conf > float(np.float32(thr))).reshape(P, h0, w0, h1, w1).clone()
    if border_rm > 0:
        bd = border_rm
        mask[:, :bd] = False
        mask[:, :, :bd] = False
        mask[:, :, :, :bd] = False
        mask[:, :, :, :, :bd] = False
        mask[:, -bd:] = False
        mask[:, :, -bd:] = False
        mask[:, :, :, -bd:] = False
        mask[:, :, :, :, -bd:] = False
    mask = mask.reshape(conf.shape)
    mask = mask & (conf == conf.max(dim=2, keepdim=True)[0]) & (conf == conf.max(dim=1, keepdim=True)[0])
    mask_v, all_j = mask.max(dim=2)
    b_ids, i_ids = torch.where(mask_v)
    j_ids = all_j[b_ids, i_ids]
    return b_ids.numpy(), i_ids.numpy(), j_ids.numpy(), conf[b_ids, i_ids, j_ids].numpy()


def _triples(res):
    p, i = np.nonzero(res["j_of_i"] >= 0)
    return p, i, res["j_of_i"][p, i], res["conf"][p, i]


@pytest.mark.parametrize("shape", [(7, 9, 6, 8, 24), (11, 13, 11, 13, 8), (9, 9, 10, 7, 256)])
@pytest.mark.parametrize("masks", [False, True])
def test_oracle_equals_the_materialised_route(shape, masks):
    h0, w0, h1, w1, C = shape
    a, b, va, vb, _ = O.planted(3, (h0, w0), (h1, w1), C, seed=C + masks, masks=masks)
    res = O.match(a, b, (h0, w0), (h1, w1), va, vb)
    # the route's -1e9 in place of -inf: a masked entry's softmax is exactly 0 along any line that has a valid
    # entry and 1/n along a fully masked one, so its conf is 0 or 1/(L S), never above thr
    want = _materialised(a, b, (h0, w0), (h1, w1), va, vb)
    got = _triples(res)
    assert len(got[0]) > 0
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert np.abs(got[3] - want[3]).max() < 1e-12
    assert np.array_equal(res["n_matches"], np.bincount(got[0], minlength=3))


def test_oracle_equals_the_recorded_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "coarse_match.npz"))
    assert g["desc_a"].dtype == np.float16
    res = O.match(g["desc_a"], g["desc_b"], tuple(g["hw_a"]), tuple(g["hw_b"]), temperature=float(g["temperature"]),
                  thr=float(g["thr"]), border_rm=int(g["border_rm"]))
    p, i, j, c = _triples(res)
    assert len(g["b_ids"]) > 10
    assert np.array_equal(p, g["b_ids"]) and np.array_equal(i, g["i_ids"]) and np.array_equal(j, g["j_ids"])
    # the recording ran with temperature 0.1 in float64, the ABI carries float32(0.1): 1.5e-8 relative on sim
    assert np.abs(c - g["mconf"]).max() < 1e-5


def test_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(5)
    hw = (5, 5)
    a = rng.normal(0, 1.4, (1, 25, 16)).astype(np.float16)
    b = rng.normal(0, 1.4, (1, 25, 16)).astype(np.float16)
    a[0, 13] = a[0, 7]               # rows 7 and 13 of A are equal: column 12 of B sees a tie
    b[0, 12] = a[0, 7]
    b[0, 17] = b[0, 11] = a[0, 8]    # rows 11 and 17 of B are equal: row 8 of A sees a tie
    res = O.match(a, b, hw, hw, thr=0.05, border_rm=0)
    conf = res["conf_matrix"][0]
    assert conf[7, 12] == conf[13, 12] == conf[:, 12].max()
    assert conf[8, 11] == conf[8, 17] == conf[8].max()
    assert res["j_of_i"][0, 7] == 12 and res["j_of_i"][0, 13] == -1
    assert res["j_of_i"][0, 8] == 11 and 17 not in res["j_of_i"][0]


def test_all_invalid_rows_and_columns_have_no_nan():
    a, b, va, vb, _ = O.planted(2, (5, 6), (4, 7), 16, seed=3, masks=True)
    va[0] = 0                        # pair 0: nothing of A is valid
    vb[1, :] = 0
    vb[1, 9] = 1                     # pair 1: one valid cell of B
    va[1, 4] = 0
    res = O.match(a, b, (5, 6), (4, 7), va, vb, border_rm=0)
    for k in ("conf_matrix", "row_sum", "col_sum", "conf"):
        assert np.isfinite(res[k]).all(), k
    assert (res["row_max"][0] == -np.inf).all() and (res["row_sum"][0] == 0).all() and res["n_matches"][0] == 0
    assert (res["conf_matrix"][0] == 0).all()
    assert res["row_max"][1, 4] == -np.inf and (res["conf_matrix"][1, 4] == 0).all()
    # one valid column: its column softmax picks one row, every row's softmax over j is 1 there
    hits = np.flatnonzero(res["j_of_i"][1] >= 0)
    assert len(hits) <= 1 and (res["j_of_i"][1, hits] == 9).all()


def _matches(j_of_i, conf, hw_a, hw_b):
    j = torch.tensor(j_of_i, dtype=torch.int32)
    return M.CoarseMatches(j_of_i=j, conf=torch.tensor(conf, dtype=torch.float32), n_matches=(j >= 0).sum(1).int(), hw_a=hw_a,
                           hw_b=hw_b)


def test_to_pixels_layout_and_transforms():
    hw_a, hw_b = (3, 4), (2, 5)
    j_of_i = np.full((3, 12), -1)
    conf = np.zeros((3, 12), np.float32)
    j_of_i[0, [1, 7]] = [9, 0]
    j_of_i[2, [11, 2, 5]] = [4, 3, 8]
    conf[j_of_i >= 0] = [0.5, 0.25, 0.75, 0.3, 0.9]
    cm = _matches(j_of_i, conf, hw_a, hw_b)
    uv_a, uv_b, ps, c = cm.to_pixels()
    assert uv_a.dtype == torch.float64 and ps.dtype == torch.int32 and c.dtype == torch.float32
    assert ps.tolist() == [0, 2, 2, 5]
    assert uv_a.tolist() == [[8, 0], [24, 8], [16, 0], [8, 8], [24, 16]]         # rows by (pair, i): i = 1, 7 | 2, 5, 11
    assert uv_b.tolist() == [[32, 8], [0, 0], [24, 0], [24, 8], [32, 0]]
    assert c.tolist() == [0.5, 0.25, 0.75, 0.30000001192092896, 0.8999999761581421]
    want = O.to_pixels(j_of_i, conf, hw_a, hw_b)
    for g, w in zip((uv_a, uv_b, ps, c), want):
        assert np.array_equal(g.numpy(), w)
    # per-pair image transforms (crop and resize: x' = s x + t): the pixel goes back through the inverse
    tf_a = np.tile(np.eye(3), (3, 1, 1))
    tf_a[:, 0, 0] = tf_a[:, 1, 1] = [2.0, 1.0, 0.5]
    tf_a[:, 0, 2], tf_a[:, 1, 2] = [-3.0, 0.0, 4.0], [5.0, 0.0, -2.0]
    tf_b = np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    uv_a2, uv_b2, ps2, _ = cm.to_pixels(scale=4, tf_a=tf_a, tf_b=torch.from_numpy(tf_b))
    assert ps2.tolist() == ps.tolist()
    # pair 0: (4 x + 3) / 2, (4 y - 5) / 2 -> cell 1 = (4, 0): (3.5, -2.5) -> (4, -3): halves away from zero
    assert uv_a2[0].tolist() == [4.0, -3.0]
    assert uv_a2[1].tolist() == [8.0, -1.0]                   # cell 7 = (12, 4): (7.5, -0.5) -> (8, -1)
    assert uv_a2[2].tolist() == [8.0, 4.0]                    # pair 2, cell 2 = (8, 0): (8 - 4) / 0.5, (0 + 2) / 0.5
    assert uv_b2[0].tolist() == [4.0, -1.0]                   # cell 9 = (16, 4): (14 / 4, -2 / 4) = (3.5, -0.5) -> (4, -1)
    want = O.to_pixels(j_of_i, conf, hw_a, hw_b, scale=4, tf_a=tf_a, tf_b=tf_b)
    assert np.array_equal(uv_a2.numpy(), want[0]) and np.array_equal(uv_b2.numpy(), want[1])
    with pytest.raises(ValueError, match="tf_a"):
        cm.to_pixels(tf_a=np.eye(4))
    empty = _matches(np.full((2, 12), -1), np.zeros((2, 12)), hw_a, hw_b).to_pixels()
    assert empty[0].shape == (0, 2) and empty[2].tolist() == [0, 0, 0] and empty[3].shape == (0,)


def test_argument_validation_happens_before_any_device_call():
    a = np.zeros((2, 12, 16), np.float32)
    b = np.zeros((2, 10, 16), np.float32)
    ok = dict(hw_a=(3, 4), hw_b=(2, 5))
    with pytest.raises(ValueError, match="hw_a=4x4"):
        M.match_descriptors(a, b, (4, 4), (2, 5))
    with pytest.raises(ValueError, match="hw_b"):
        M.match_descriptors(a, b, (3, 4), (5, 5))
    with pytest.raises(ValueError, match="C=12"):
        M.match_descriptors(a[:, :, :12], b[:, :, :12], **ok)
    with pytest.raises(ValueError, match="C=520"):
        M.match_descriptors(np.zeros((1, 12, 520), np.float16), np.zeros((1, 10, 520), np.float16), **ok)
    with pytest.raises(ValueError, match="P and C must agree"):
        M.match_descriptors(a, b[:, :, :8], **ok)
    for thr in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="thr"):
            M.match_descriptors(a, b, thr=thr, **ok)
    with pytest.raises(ValueError, match="temperature"):
        M.match_descriptors(a, b, temperature=0.0, **ok)
    with pytest.raises(ValueError, match="border_rm"):
        M.match_descriptors(a, b, border_rm=-1, **ok)
    with pytest.raises(ValueError, match="both sides"):
        M.match_descriptors(a, b, valid_a=np.ones((2, 12)), **ok)
    with pytest.raises(ValueError, match="valid_b"):
        M.match_descriptors(a, b, valid_a=np.ones((2, 12)), valid_b=np.ones((2, 12)), **ok)
    with pytest.raises(ValueError, match="floating-point"):
        M.match_descriptors(a.astype(np.int32), b, **ok)
    with pytest.raises(ValueError, match="desc_a is on"):      # a device mismatch
        M.match_descriptors(torch.zeros(2, 12, 16), torch.zeros(2, 10, 16, device="meta"), **ok)
    with pytest.raises(ValueError, match="P axis"):
        M.match_descriptors(a[0], b, **ok)


def test_entry_point_names_the_bad_field():
    from bundlesdf_amd import build
    build.build()
    L = _lib.lib()

    def good():
        D = _lib.MatchDesc()
        D.P, D.L, D.S, D.C, D.h0, D.w0, D.h1, D.w1 = 2, 12, 10, 16, 3, 4, 2, 5
        D.border_rm, D.temperature, D.thr = 2, 0.1, 0.2
        return D

    for field, value, text in (("P", 0, b"P=0"), ("C", 12, b"C=12"), ("C", 520, b"C=520"), ("L", 13, b"L=13"),
                               ("S", 9, b"S=9"), ("thr", 1.0, b"thr=1"), ("thr", -0.5, b"thr=-0.5"),
                               ("temperature", 0.0, b"temperature=0"), ("border_rm", -1, b"border_rm=-1"),
                               ("valid_a", 64, b"valid_b is NULL")):
        D = good()
        setattr(D, field, value)
        assert L.nof_match_descriptors(ctypes.byref(D), None) == 1, field
        assert text in L.nof_last_error(), (field, L.nof_last_error())
    assert L.nof_match_descriptors(ctypes.byref(good()), None) == 1 and b"desc_a is NULL" in L.nof_last_error()
    assert L.nof_match_descriptors(None, None) == 1


def test_workspace_does_not_grow_with_L_times_S():
    from bundlesdf_amd import build
    build.build()
    L = _lib.lib()
    n = L.nof_match_workspace_bytes(45, 2500, 2500)
    assert 0 < n <= 45 * (4 * 2500 + 3 * 2500) * 4 + 7 * 256
    assert n < 45 * 2500 * 2500 * 4 // 100
    assert L.nof_match_workspace_bytes(0, 5, 5) == 0
