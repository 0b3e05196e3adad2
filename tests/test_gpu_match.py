"""GPU: bundlesdf_amd.matching (csrc/match.hip, include/nof.h group 11) against tests/match_oracle.py on
the same float16 inputs.

The bound (eps = 2^-24, half a float32 ulp; everything first order, widened by 1 %):

  sim.   The kernel's sim differs from the oracle's by at most
           E_ij = C eps sum_k |a_ik b_jk| / (C T)  +  4 eps |sim_ij|:
         float32 accumulation of C exact fp16 products in any order, then the scale (its own two
         roundings, 1 / (C T) from a product and a division) and one product with it.
  max.   A maximum of perturbed values moves by at most the largest perturbation of its line:
           Er_i = max_j E_ij (row), Ec_j = max_i E_ij (column).
  exp.   The argument x = sim - max carries E_ij + Er_i and one rounding, eps |x|; expf is taken as good to
         2 float32 ulp = 4 eps. In the statistics kernel a term is also rescaled when the running maximum
         of its line rises, at most once per tile: a product (eps) with an exp (4 eps) whose argument
         carries one rounding; the arguments of one term's rescales add up to at most |x|, so all of them
         add n_tiles 5 eps + eps |x|. Relative error of one term of a line's sum:
           d_ij = 1.01 (E_ij + E_line + 2 eps |x_ij|) + 4 eps + 5 n_tiles eps.
  sum.   Non-negative terms added one after the other: the weighted mean of the terms' errors plus one
         rounding per addition, n additions of the keys and 2 per tile for the rescaled carry and the
         meeting of the lane halves:
           dsum_i = sum_j e_ij d_ij / sum_j e_ij + (n + 2 n_tiles + 2) eps.
  conf.  (exp (1/rowsum)) (exp (1/colsum)): both exp terms, both sums, two reciprocals (2 eps each with
         their rounding) and three products (eps each):
           B_ij = 1.01 conf_ij (d_ij(row) + dsum_i + d_ij(col) + dsum_j + 8 eps) + 1e-37.

Fragile rows. Row i with the oracle's best partner j1 is fragile if the oracle's top-two margin of row i
or of column j1 is below twice the largest B of that line, or |conf(i,j1) - thr| is below B; a row whose
best conf lies below thr by more than B cannot match on either side and is not fragile whatever its
margins. Fragile rows may differ; they may be at most 1 % of the oracle's matches and the planted cases
must have none.
"""
import numpy as np
import pytest
import torch

from bundlesdf_amd import matching as M
from tests import match_oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_CACHE = {}


def _np(t):
    return t.cpu().numpy()


def _line_bounds(sim, abs_dot, C, temperature, axis, tile=M.TILE[1]):
    """(E_line, d [P,L,S], dsum) for the statistics along `axis` (2: rows, 1: columns)."""
    T = float(np.float32(temperature))
    finite = np.isfinite(sim)
    E = np.where(finite, C * EPS * abs_dot / (C * T) + 4 * EPS * np.abs(np.where(finite, sim, 0.0)), 0.0)
    E_line = E.max(axis)
    m = sim.max(axis)
    x = np.where(finite, sim - np.expand_dims(np.where(np.isfinite(m), m, 0.0), axis), -np.inf)
    n = sim.shape[axis]
    n_tiles = -(-n // tile)
    d = 1.01 * (E + np.expand_dims(E_line, axis) + 2 * EPS * np.abs(np.where(finite, x, 0.0))) + 4 * EPS + 5 * n_tiles * EPS
    e = np.exp(x)
    s = e.sum(axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        dsum = np.where(s > 0, (e * d).sum(axis) / s, 0.0) + (n + 2 * n_tiles + 2) * EPS
    return E_line, d, dsum


def _bounds(res, C, temperature):
    Er, d_row, dsum_row = _line_bounds(res["sim"], res["abs_dot"], C, temperature, 2)
    Ec, d_col, dsum_col = _line_bounds(res["sim"], res["abs_dot"], C, temperature, 1)
    B = 1.01 * res["conf_matrix"] * (d_row + dsum_row[:, :, None] + d_col + dsum_col[:, None, :] + 8 * EPS) + 1e-37
    return dict(Er=Er, Ec=Ec, dsum_row=dsum_row, dsum_col=dsum_col, B=B)


def _top_two_margin(conf, axis):
    s = np.sort(conf, axis)
    top = np.take(s, -1, axis)
    second = np.take(s, -2, axis) if conf.shape[axis] > 1 else np.zeros_like(top)
    return top - second


def _fragile(res, bd, thr):
    conf, B = res["conf_matrix"], bd["B"]
    P, L, S = conf.shape
    pi, ii = np.arange(P)[:, None], np.arange(L)[None, :]
    j1 = res["row_best"]
    c1, B1 = conf[pi, ii, j1], B[pi, ii, j1]
    row_close = _top_two_margin(conf, 2) < 2 * B.max(2)
    col_close = (_top_two_margin(conf, 1) < 2 * B.max(1))[pi, j1]
    thr32 = float(np.float32(thr))
    hopeless = (conf + B).max(2) <= thr32          # no entry of the row can pass the threshold on either side
    return (row_close | col_close | (np.abs(c1 - thr32) < B1)) & ~hopeless


def _check(dev, a, b, hw_a, hw_b, va=None, vb=None, planted=False, **kw):
    """match_descriptors against the oracle; returns (got, want)."""
    C = a.shape[-1]
    temperature, thr = kw.get("temperature", 0.1), kw.get("thr", 0.2)
    got = M.match_descriptors(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), hw_a, hw_b,
                              None if va is None else torch.from_numpy(va).to(dev),
                              None if vb is None else torch.from_numpy(vb).to(dev), return_stats=True, **kw)
    torch.cuda.synchronize()
    want = O.match(a, b, hw_a, hw_b, va, vb, **kw)
    bd = _bounds(want, C, temperature)
    P, L, S = want["sim"].shape
    assert got.j_of_i.shape == (P, L) and got.j_of_i.dtype == torch.int32 and got.conf.dtype == torch.float32
    assert got.n_matches.shape == (P,) and got.n_matches.dtype == torch.int32

    # statistics
    for name, E, dsum in (("row", bd["Er"], bd["dsum_row"]), ("col", bd["Ec"], bd["dsum_col"])):
        gm, gs = _np(getattr(got, name + "_max")).astype(np.float64), _np(getattr(got, name + "_sum")).astype(np.float64)
        wm, ws = want[name + "_max"], want[name + "_sum"]
        empty = ~np.isfinite(wm)
        assert np.array_equal(np.isneginf(gm), empty) and (gs[empty] == 0).all(), name
        err_m = np.abs(gm[~empty] - wm[~empty])
        # each side's sum is relative to its own maximum: d_ij carries the maximum's error E_line already
        rel_s = (np.abs(gs - ws) / np.where(empty, 1.0, ws))[~empty]
        if err_m.size:
            print(f"{name}: max err {err_m.max():.3e} (bound {E[~empty].max():.3e}), sum rel err {rel_s.max():.3e} "
                  f"(bound {dsum[~empty].max():.3e})")
        assert (err_m <= E[~empty] + 1e-30).all(), name
        assert (rel_s <= dsum[~empty]).all(), name

    # matches
    fragile = _fragile(want, bd, thr)
    n_want = int((want["j_of_i"] >= 0).sum())
    print(f"matches {n_want}, fragile rows {int(fragile.sum())}")
    assert fragile.sum() <= 0.01 * n_want
    if planted:
        assert fragile.sum() == 0 and n_want > 0
    gj, gc = _np(got.j_of_i), _np(got.conf).astype(np.float64)
    solid = ~fragile
    assert np.array_equal(gj[solid], want["j_of_i"][solid])
    hit = solid & (want["j_of_i"] >= 0)
    pi, ii = np.nonzero(hit)
    err = np.abs(gc[hit] - want["conf"][hit])
    if err.size:
        print(f"conf: max err {err.max():.3e}, smallest slack {(bd['B'][pi, ii, want['j_of_i'][hit]] - err).min():.3e}")
    assert (err <= bd["B"][pi, ii, want["j_of_i"][hit]]).all()
    assert (gc[gj < 0] == 0).all() and (gc[gj >= 0] > np.float32(thr)).all()
    assert np.array_equal(_np(got.n_matches), (gj >= 0).sum(1))
    return got, want


SHAPES = [(7, 9, 6, 8, 24), (11, 13, 11, 13, 8), (9, 9, 10, 7, 256)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
def test_planted_descriptors(cuda_device, shape, masks):
    h0, w0, h1, w1, C = shape
    a, b, va, vb, _ = O.planted(3, (h0, w0), (h1, w1), C, seed=C + masks, masks=masks)
    # L and S straddle the 32-key tile and (L = 143) the 128-query block; C = 24 and 8 end inside a 16-wide k-step
    assert (h0 * w0) % M.TILE[1] or (h1 * w1) % M.TILE[1]
    got, want = _check(cuda_device, a, b, (h0, w0), (h1, w1), va, vb, planted=True)
    if not masks:
        again = _check(cuda_device, a, b, (h0, w0), (h1, w1), planted=True, border_rm=0, thr=0.05)[0]
        assert int(again.n_matches.sum()) > int(got.n_matches.sum())


@pytest.mark.parametrize("C", [8, 512])
def test_one_cell_against_one(cuda_device, C):
    a, b, _, _, _ = O.planted(3, (1, 1), (1, 1), C, seed=1)
    got, _ = _check(cuda_device, a, b, (1, 1), (1, 1), border_rm=0)
    assert _np(got.conf).tolist() == [[1.0]] * 3 and _np(got.j_of_i).tolist() == [[0]] * 3      # softmax of one entry
    none, _ = _check(cuda_device, a, b, (1, 1), (1, 1))                                         # the border takes it
    assert _np(none.j_of_i).tolist() == [[-1]] * 3 and _np(none.n_matches).tolist() == [0, 0, 0]


def test_one_row_against_33(cuda_device):
    a, b, _, _, truth = O.planted(3, (1, 1), (3, 11), 8, seed=4)
    got, want = _check(cuda_device, a, b, (1, 1), (3, 11), border_rm=0, planted=True)
    assert (_np(got.j_of_i)[:, 0] == truth[:, 0]).all()
    # and the other way round: 33 rows, one column, so every row's softmax is 1 and the column's picks one row
    got, want = _check(cuda_device, b, a, (3, 11), (1, 1), border_rm=0, thr=0.05)
    assert (_np(got.n_matches) <= 1).all()


def test_single_pair_float32_and_numpy_inputs(cuda_device):
    a, b, va, vb, _ = O.planted(1, (7, 9), (6, 8), 24, seed=11, masks=True)
    got = M.match_descriptors(a[0].astype(np.float32), b[0].astype(np.float32), (7, 9), (6, 8), va[0], vb[0])
    ref = M.match_descriptors(torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device), (7, 9), (6, 8),
                              va, vb)
    assert got.j_of_i.shape == (1, 63) and got.row_max is None
    assert _np(got.j_of_i).tobytes() == _np(ref.j_of_i).tobytes() and _np(got.conf).tobytes() == _np(ref.conf).tobytes()


def test_ties_go_to_the_lowest_index(cuda_device):
    rng = np.random.default_rng(5)
    hw = (6, 7)                      # 42 cells: the tied rows 7 and 40 lie in different 32-key tiles
    a = rng.normal(0, 1.4, (3, 42, 16)).astype(np.float16)
    b = rng.normal(0, 1.4, (3, 42, 16)).astype(np.float16)
    a[:, 40] = a[:, 7]               # rows 7 and 40 of A are equal: column 12 of B sees a tie
    b[:, 12] = a[:, 7]
    b[:, 11] = a[:, 8]               # rows 11, 17 and 39 of B are equal: row 8 of A sees a tie
    b[:, 17] = a[:, 8]
    b[:, 39] = a[:, 8]
    want = O.match(a, b, hw, hw, thr=0.05, border_rm=0)
    got = M.match_descriptors(torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device), hw, hw, thr=0.05,
                              border_rm=0)
    gj = _np(got.j_of_i)
    for p in range(3):
        assert want["j_of_i"][p, 7] == 12 and want["j_of_i"][p, 40] == -1 and want["j_of_i"][p, 8] == 11
        assert gj[p, 7] == 12 and gj[p, 40] == -1, gj[p]
        assert gj[p, 8] == 11 and 17 not in gj[p] and 39 not in gj[p], gj[p]
    # the tied entries carry one confidence: the kernel's columns saw equal bits
    assert abs(float(got.conf[0, 7]) - want["conf"][0, 7]) < 1e-4


def test_same_bytes_on_every_run_and_stream(cuda_device):
    a, b, va, vb, _ = O.planted(3, (11, 13), (11, 13), 40, seed=9, masks=True)
    args = [torch.from_numpy(x).to(cuda_device) for x in (a, b)]
    masks = [torch.from_numpy(x).to(cuda_device) for x in (va, vb)]
    runs = [M.match_descriptors(*args, (11, 13), (11, 13), *masks, return_stats=True) for _ in range(2)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        runs.append(M.match_descriptors(*args, (11, 13), (11, 13), *masks, return_stats=True))
    s.synchronize()
    for k in ("j_of_i", "conf", "n_matches", "row_max", "row_sum", "col_max", "col_sum"):
        first = _np(getattr(runs[0], k)).tobytes()
        assert all(_np(getattr(r, k)).tobytes() == first for r in runs[1:]), k
    assert int(runs[0].n_matches.sum()) > 0


def test_workspace_does_not_grow_with_L_times_S(cuda_device):
    from bundlesdf_amd import _lib
    L = _lib.lib()
    small, big = L.nof_match_workspace_bytes(3, 100, 100), L.nof_match_workspace_bytes(3, 1000, 1000)
    assert small > 0 and big <= 10 * small + 7 * 256         # linear in L + S
    assert L.nof_match_workspace_bytes(45, 2500, 2500) < 45 * 2500 * 2500 * 4 // 100


def _scene(dev):
    """The 3-frame 128x96 scene the frame-map hand-over renders, with descriptors made from where each
    1/8-grid cell's pixel lies on the object: random Fourier features of the object-space point, so that
    a cell's best partner in another frame is the cell that sees the nearest surface point."""
    if "scene" not in _CACHE:
        from bundlesdf_amd import frames as F
        from scripts.frame_maps import bumpy_mesh, object_poses, render_depth
        H, W, C = 96, 128, 128
        K = np.array([[260.0, 0.0, W / 2 - 0.5], [0.0, 260.0, H / 2 - 0.5], [0.0, 0.0, 1.0]])
        ob_in_cam = object_poses(3)
        depth = render_depth(bumpy_mesh(3), ob_in_cam, K, H, W, dev)
        maps = F.prepare_frames(depth, K)
        pts = _np(maps.points).astype(np.float64)[:, ::8, ::8]                  # [3,12,16,3] camera space
        valid = (_np(maps.depth)[:, ::8, ::8] > 0).reshape(3, -1).astype(np.uint8)
        cam_in_ob = np.linalg.inv(ob_in_cam)
        obj = np.einsum("nij,nhwj->nhwi", cam_in_ob[:, :3, :3], pts) + cam_in_ob[:, None, None, :3, 3]
        rng = np.random.default_rng(0)
        w, phase = rng.normal(0.0, 100.0, (C, 3)), rng.uniform(0, 2 * np.pi, C)   # a 1 cm wide kernel
        desc = (2.8 * np.cos(obj.reshape(3, -1, 3) @ w.T + phase)).astype(np.float16)
        _CACHE["scene"] = dict(maps=maps, desc=desc, valid=valid, ob_in_cam=ob_in_cam, hw=(H // 8, W // 8),
                               model=bumpy_mesh(3).vertices)
    return _CACHE["scene"]


def test_chain_descriptors_to_ransac(cuda_device):
    """match_descriptors -> to_pixels -> lift_matches -> ransac_pairs with no host array in between but
    the counts. Cells are 8 pixels apart, about 15 mm on the object at 0.5 m with f = 260: a correct
    match joins two pixels that see surface points up to about a cell's half diagonal (11 mm) apart, so
    inlier_dist is 20 mm; the refit over all inliers averages that out and must put every model point
    within inlier_dist of where the true motion puts it."""
    from bundlesdf_amd import frames as F
    from bundlesdf_amd.ransac import ransac_pairs
    sc = _scene(cuda_device)
    pairs = np.array([(0, 1), (1, 2), (0, 2)])
    d = torch.from_numpy(sc["desc"]).to(cuda_device)
    v = torch.from_numpy(sc["valid"]).to(cuda_device)
    fa, fb = pairs[:, 0].tolist(), pairs[:, 1].tolist()
    cm = M.match_descriptors(d[fa], d[fb], sc["hw"], sc["hw"], v[fa], v[fb], border_rm=0)
    uv_a, uv_b, pair_start, conf = cm.to_pixels(scale=8)
    lifted = F.lift_matches(sc["maps"], pairs, uv_a, uv_b, pair_start).compact()
    min_inliers, inlier_dist = 8, 0.02
    res = ransac_pairs(lifted.pts_a, lifted.pts_b, lifted.pair_start, lifted.normals_a, lifted.normals_b,
                       conf=conf[lifted.rows].double(), inlier_dist=inlier_dist, normal_angle_deg=45.0, n_trials=512,
                       min_inliers=min_inliers)
    torch.cuda.synchronize()
    n_in = _np(res.n_inliers)
    print("matches", _np(cm.n_matches).tolist(), "lifted", np.diff(_np(lifted.pair_start)).tolist(), "inliers", n_in.tolist())
    assert (n_in >= min_inliers).all()
    model = np.asarray(sc["model"], np.float64)
    for p, (fa, fb) in enumerate(pairs):
        true = sc["ob_in_cam"][fb] @ np.linalg.inv(sc["ob_in_cam"][fa])          # camera a onto camera b
        at_a = model @ sc["ob_in_cam"][fa][:3, :3].T + sc["ob_in_cam"][fa][:3, 3]
        want = at_a @ true[:3, :3].T + true[:3, 3]
        got = at_a @ res.refit_pose[p][:3, :3].T + res.refit_pose[p][:3, 3]
        worst = np.linalg.norm(got - want, axis=1).max()
        print(f"pair {p}: refit off by at most {1e3 * worst:.2f} mm at the model's points")
        assert worst < inlier_dist
