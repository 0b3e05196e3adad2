"""CPU: the RANSAC oracle (tests/ransac_oracle.py) is a fair yardstick on the shared cases, and the
new entry points are declared, laid out and validated as include/nof.h (group 8) says, on a machine
with no GPU. The device results are held to the oracle in tests/test_gpu_ransac.py."""
import ctypes
import os

import numpy as np
import pytest

from bundlesdf_amd import _lib
from bundlesdf_amd import ransac as R
from tests import ransac_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the oracle
def test_hash_and_draws():
    assert int(O.hash32(0)) == 0
    x = 1                                    # the header's five steps on Python integers
    x ^= x >> 16
    x = x * 0x7feb352d & 0xFFFFFFFF
    x ^= x >> 15
    x = x * 0x846ca68b & 0xFFFFFFFF
    x ^= x >> 16
    assert int(O.hash32(1)) == x
    idx, ok = O.draws(3, 1000, [0, 2, 50], seed=5)
    assert (idx[0] == 0).all() and not ok[:2].any()
    assert idx[2].min() == 0 and idx[2].max() == 49
    assert 0.9 < ok[2].mean() < 1.0          # 1 - P(two of three equal) = 0.9408
    assert not np.array_equal(idx[2], O.draws(3, 1000, [0, 2, 50], seed=6)[0][2])
    # the counter wraps in uint32: pair 40000 of 65536 trials starts over
    big = O.draws(40001, 4, [7] * 40001, seed=5)[0]
    p, T, t, j = 40000, 4, 3, 2
    u = O.hash32(np.uint32(((p * T + t) * 3 + j) & 0xFFFFFFFF) ^ O.hash32(5))
    assert big[p, t, j] == (int(u) * 7) >> 32


def test_two_routes_agree_and_fit_exact_data():
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, (200, 3, 3))
    Rm = np.stack([O.rotation(v) for v in rng.normal(size=(200, 3))])
    t = rng.normal(size=(200, 3))
    b = np.einsum("trc,tic->tir", Rm, a) + t[:, None]
    for fit in (O.fit_svd, O.fit_horn):
        R_, t_ = fit(a, b)
        keep = O.sigma_ratio(a, b) >= 1e-3
        assert keep.sum() > 150
        assert np.abs(R_[keep] - Rm[keep]).max() < 1e-9 and np.abs(t_[keep] - t[keep]).max() < 1e-9
        assert (np.linalg.det(R_) > 0).all()


@pytest.mark.parametrize("name", O.CASES)
def test_case_is_fair(name):
    """No value the exact comparisons depend on lies within 1e-9 (relative for the distances and the
    translation gate, absolute for the cosines and the trace) of its threshold, over every trial the
    oracle fits (live or gated out) and every row: a pose that differs from the oracle's in its last bits then scores
    the same."""
    c, h = O.case(name), O.expected(name)
    max_trans_sq, min_trace, dist_sq, cos_normal = O.settings(c)
    for p, s in enumerate(O.pair_slices(c)):
        ok = h["ok"][p]
        t2, tr = O.gate_values(h["poses"][p][ok])
        if np.isfinite(max_trans_sq[p]):
            assert (np.abs(t2 - max_trans_sq[p]) > O.FAIR_REL * max_trans_sq[p]).all()
        if np.isfinite(min_trace[p]):
            assert (np.abs(tr - min_trace[p]) > O.FAIR_REL).all()
        if s.stop == s.start or not ok.any():
            continue
        na, nb = O._normals(c, s)
        d2, dot = O.inlier_values(h["poses"][p][ok], c["pts_a"][s], c["pts_b"][s], na, nb)
        assert (np.abs(d2 - dist_sq) > O.FAIR_REL * dist_sq).all()
        if dot is not None:
            assert (np.abs(dot - cos_normal) > O.FAIR_REL).all()


def test_planted_case_meets_its_conditions():
    c, h = O.case("planted"), O.expected("planted")
    share = O.well_conditioned("planted").sum() / h["live"].sum()
    print("well-conditioned share of the live trials", share, "e0", O.route_gap("planted"), "bound", O.pose_bound("planted"))
    assert share >= 0.9
    assert np.array_equal(h["inlier"], c["planted"])
    sl = O.pair_slices(c)
    assert [s.stop - s.start for s in sl] == [200, 317, 64] and c["n_trials"] == 512
    for p, s in enumerate(sl):
        assert c["planted"][s].sum() == round(0.6 * (s.stop - s.start))
        T = c["planted_pose"][p]
        res = np.linalg.norm(c["pts_b"][s] - (c["pts_a"][s] @ T[:3, :3].T + T[:3, 3]), axis=1)
        assert (res[~c["planted"][s]] >= 10 * c["inlier_dist"] * (1 - 1e-12)).all()
        assert (res[c["planted"][s]] < c["inlier_dist"]).all()
        assert np.allclose(np.linalg.norm(c["normals_a"][s], axis=1), 1) and np.allclose(
            np.linalg.norm(c["normals_b"][s], axis=1), 1)


def test_other_cases_show_what_they_are_for():
    h = O.expected("gated")
    assert h["ok"][0].sum() > 200 and not h["live"][0].any() and h["best_trial"][0] == -1
    assert h["live"][1].any() and (h["ok"][1] & ~h["live"][1]).any() and h["n_inliers"][1] > 0
    h = O.expected("tiny")
    assert not h["live"][:3].any() and (h["best_trial"][:3] == -1).all()
    assert np.array_equal(h["live"][3], h["ok"][3]) and 0 < h["ok"][3].mean() < 0.35      # 6 / 27 = 0.22
    assert h["score"][4] == 4 * 65536 and h["n_inliers"][4] == 0                          # cleared by min_inliers = 5
    assert O.finish(O.case("tiny"), h["poses"], h["live"], h["scores"], min_inliers=3)["n_inliers"].tolist() == [0, 0, 0, 3, 4]
    h = O.expected("duplicated_best")
    assert (np.where(h["live"][0], h["scores"][0], 0) == h["score"][0]).sum() >= 2
    c = O.case("weights")
    assert np.array_equal(c["conf"] * 256, np.rint(c["conf"] * 256)) and c["conf"].max() > 1 and (c["conf"] == 0).any()
    assert O.case("no_normals")["normals_a"] is None
    c = O.case("degenerate")
    assert (c["pts_a"][:50] == c["pts_a"][0]).all() and np.linalg.matrix_rank(c["pts_a"][50:] - c["pts_a"][50]) == 1
    assert np.diff(O.case("uneven")["pair_start"]).tolist() == [5, 600]
    assert [np.diff(O.case(f"tails_T{t}")["pair_start"]).tolist() for t in O.TAIL_TRIALS] == [[63, 64, 65, R.ROW_TILE + 1]] * 3


# ----------------------------------------------------------------------------- header and binding
def test_symbols_and_tile_constant():
    header = open(os.path.join(ROOT, "include", "nof.h")).read()
    for sym in ("nof_ransac_workspace_bytes", "nof_ransac_pairs"):
        assert sym + "(" in header and sym in _lib.declared_symbols()
        assert hasattr(_lib.lib(), sym)
    src = open(os.path.join(ROOT, "bundlesdf_amd", "csrc", "ransac.hip")).read()
    assert f"constexpr int RANSAC_TILE = {R.ROW_TILE};" in src


def _valid_desc(P=2, M=10, T=8, normals=True):
    """A descriptor that passes validation; its pointers are host addresses that no test lets the
    library reach (each test breaks one field, and validation comes before the first HIP call)."""
    keep = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(keep)
    D = _lib.RansacDesc()
    for name, kind in _lib.RansacDesc._fields_:
        if kind is _lib._p:
            setattr(D, name, addr)
    if not normals:
        D.normals_a = D.normals_b = None
    D.M, D.P, D.n_trials, D.seed, D.min_inliers = M, P, T, 0, 5
    D.inlier_dist_sq, D.cos_normal = 1e-4, 0.5
    D.workspace_bytes = _lib.lib().nof_ransac_workspace_bytes(P, M, T)
    D._keep = keep
    return D


BAD = [("P", dict(P=0), b"P=0"), ("P", dict(P=65536), b"P=65536"), ("n_trials", dict(n_trials=0), b"n_trials=0"),
       ("n_trials", dict(n_trials=65537), b"n_trials=65537"), ("M", dict(M=-1), b"M=-1"),
       ("M", dict(M=2 ** 31), b"M=2147483648"), ("normals", dict(normals_a=None), b"normals_a"),
       ("normals", dict(normals_b=None), b"normals_b"), ("inlier_dist_sq", dict(inlier_dist_sq=-1.0), b"inlier_dist_sq"),
       ("inlier_dist_sq", dict(inlier_dist_sq=float("nan")), b"inlier_dist_sq"),
       ("workspace", dict(workspace_bytes=None), b"workspace_bytes"), ("workspace", dict(workspace=None), b"workspace is NULL")]
BAD += [(name, {name: None}, name.encode() + b" is NULL") for name in
        ("best_trial", "score", "pose", "n_inliers", "inlier", "sums", "pts_a", "pts_b", "pair_start", "max_trans_sq",
         "min_trace")]


@pytest.mark.parametrize("what,change,needle", BAD, ids=[f"{b[0]}-{i}" for i, b in enumerate(BAD)])
def test_bad_descriptor_is_refused_before_device_work(what, change, needle):
    L = _lib.lib()
    D = _valid_desc()
    for k, v in change.items():
        if k == "workspace_bytes":
            v = D.workspace_bytes - 1
        setattr(D, k, v)
    assert L.nof_ransac_pairs(ctypes.byref(D), None) == 1          # NOF_EINVAL
    msg = L.nof_last_error()
    assert needle in msg and b"ransac_pairs" in msg, msg
    assert L.nof_ransac_pairs(None, None) == 1 and b"desc is NULL" in L.nof_last_error()


def test_empty_call_and_workspace_size():
    L = _lib.lib()
    D = _valid_desc(M=0)
    D.pts_a = D.pts_b = D.inlier = D.workspace = None               # what empty tensors give
    D.workspace_bytes = 0
    assert L.nof_ransac_pairs(ctypes.byref(D), None) == 0
    # poses, scores and live flags per trial, nothing per row: far below a [T x n] flag array
    assert L.nof_ransac_workspace_bytes(20, 40000, 2000) == -(-20 * 2000 * (96 + 8 + 1) // 256) * 256
    assert L.nof_ransac_workspace_bytes(20, 40000, 2000) == L.nof_ransac_workspace_bytes(20, 4, 2000)
    assert L.nof_ransac_workspace_bytes(0, 10, 10) == 0


# ----------------------------------------------------------------------------- the Python layer
def test_python_layer_refuses_bad_input_on_the_host():
    c = O.case("planted")
    kw = dict(inlier_dist=0.01, device="cpu")           # never reached: the checks come before any device use
    bad = c["pair_start"].copy()
    bad[1], bad[2] = bad[2], bad[1]
    with pytest.raises(ValueError, match="pair_start"):
        R.ransac_pairs(c["pts_a"], c["pts_b"], bad, **kw)
    with pytest.raises(ValueError, match="pair_start"):
        R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"][:-1], **kw)      # does not end at M
    with pytest.raises(ValueError, match="normals"):
        R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"], normals_a=c["normals_a"], **kw)
    with pytest.raises(ValueError, match="normals"):
        R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"], normals_b=c["normals_b"], **kw)
    for v in (-0.5, 32768.0, float("nan")):
        conf = np.ones(len(c["pts_a"]))
        conf[17] = v
        with pytest.raises(ValueError, match="conf"):
            R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"], conf=conf, **kw)
    with pytest.raises(ValueError, match="n_trials"):
        R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"], n_trials=65537, **kw)
