"""GPU: bundlesdf_amd.ransac against tests/ransac_oracle.py on the seeded cases whose fairness
tests/test_ransac_cpu.py checks. The draws, the scores, the winner, the flags and the counts are
compared exactly; the three-point fits are held to the oracle's SVD route within 16 times the gap
between the oracle's own two routes, and the refit sums to math.fsum within the bound
tests/test_gpu_evaluate.py derives for the correspondence sums."""
import functools

import numpy as np
import pytest
import torch

from bundlesdf_amd import ransac as R
from bundlesdf_amd.evaluate import _kabsch
from tests import ransac_oracle as O

pytestmark = pytest.mark.gpu

ARGS = ("inlier_dist", "normal_angle_deg", "n_trials", "max_trans", "max_rot_deg", "min_inliers", "seed")
OUTPUTS = ("inlier", "n_inliers", "score", "best_trial", "pose", "sums", "trial_idx", "trial_pose", "trial_live",
           "trial_score")


def _call(c, **over):
    kw = {k: c[k] for k in ARGS}
    kw.update(over)
    return R.ransac_pairs(c["pts_a"], c["pts_b"], c["pair_start"], c["normals_a"], c["normals_b"], c["conf"],
                          return_trials=True, device=torch.device("cuda", 0), **kw)


def _numpy(res):
    out = {k: getattr(res, k).cpu().numpy() for k in OUTPUTS}
    out["refit_pose"] = res.refit_pose
    out["trial_live"] = out["trial_live"].astype(bool)
    return out


@functools.lru_cache(maxsize=None)
def _run(name):
    """One device run of a case, shared by the tests and left unchanged."""
    return _numpy(_call(O.case(name)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check_outcome(c, got, min_inliers=None):
    """Winner, score, pose, flags and counts equal the oracle's rule applied to the kernel's own trials."""
    want = O.finish(c, got["trial_pose"], got["trial_live"], got["trial_score"], min_inliers)
    assert np.array_equal(got["best_trial"], want["best_trial"])
    assert np.array_equal(np.rint(got["score"] * 65536).astype(np.int64), want["score"])
    assert got["pose"].shape == want["pose"].shape and np.array_equal(_bits(got["pose"]), _bits(want["pose"]))
    assert np.array_equal(got["inlier"], want["inlier"])
    assert np.array_equal(got["n_inliers"], want["n_inliers"])
    return want


@pytest.mark.parametrize("name", O.CASES)
def test_draws_are_the_oracles(cuda_device, name):
    c, h, got = O.case(name), O.expected(name), _run(name)
    assert got["trial_idx"].dtype == np.int32 and np.array_equal(got["trial_idx"], h["idx"])
    assert not got["trial_live"][~h["ok"]].any()                  # dead by a repeated row or by n < 3
    assert (got["trial_pose"][~h["ok"]] == 0).all()
    # the gates of the header on the kernel's own poses decide the rest, and (the case being fair) agree
    # with the oracle's own trials wherever the sample is well conditioned
    max_trans_sq, min_trace, _, _ = O.settings(c)
    for p in range(len(h["ok"])):
        assert np.array_equal(got["trial_live"][p], h["ok"][p] & O.gate(got["trial_pose"][p], max_trans_sq[p], min_trace[p]))
    keep = h["ok"] & (h["ratio"] >= 1e-3)
    assert np.array_equal(got["trial_live"][keep], h["live"][keep])


def test_hypotheses_on_planted(cuda_device):
    got, h = _run("planted"), O.expected("planted")
    keep = O.well_conditioned("planted")
    e0, bound = O.route_gap("planted"), O.pose_bound("planted")
    err = float(np.abs(got["trial_pose"][keep] - h["poses"][keep]).max())
    print(f"planted: {int(keep.sum())} well-conditioned trials, e0 {e0:.3e}, bound {bound:.3e}, kernel max {err:.3e}")
    assert got["trial_live"][keep].all()
    assert err <= bound


@pytest.mark.parametrize("name", O.CASES)
def test_live_poses_are_proper_rotations(cuda_device, name):
    got = _run(name)
    Rm = got["trial_pose"][got["trial_live"]].reshape(-1, 3, 4)[:, :, :3]
    if len(Rm) == 0:
        return
    orth = float(np.abs(Rm.transpose(0, 2, 1) @ Rm - np.eye(3)).max())
    print(name, "max |R^T R - I|", orth, "bound", O.pose_bound("planted"))
    assert orth <= O.pose_bound("planted")
    assert (np.linalg.det(Rm) > 0).all()


@pytest.mark.parametrize("name", O.CASES)
def test_scores_are_exact(cuda_device, name):
    got = _run(name)
    want = O.trial_scores(O.case(name), got["trial_pose"], got["trial_live"])
    assert got["trial_score"].dtype == np.int64 and np.array_equal(got["trial_score"], want)
    assert (got["trial_score"][~got["trial_live"]] == 0).all()


@pytest.mark.parametrize("name", O.CASES)
def test_winner_and_flags(cuda_device, name):
    c, got = O.case(name), _run(name)
    _check_outcome(c, got)
    if name == "gated":
        assert got["best_trial"][0] == -1 and got["best_trial"][1] >= 0 and got["n_inliers"][1] > 0
    if name == "tiny":
        assert (got["best_trial"][:3] == -1).all() and got["best_trial"][4] >= 0
        assert got["score"][4] == 4.0 and got["n_inliers"][4] == 0          # four inliers, cleared by min_inliers = 5
    for p in np.flatnonzero(got["best_trial"] < 0):
        s = O.pair_slices(c)[p]
        assert np.array_equal(got["pose"][p], np.eye(4)) and got["score"][p] == 0 and not got["inlier"][s].any()
        assert got["n_inliers"][p] == 0 and (got["sums"][p] == 0).all()
    if name == "duplicated_best":
        top = np.flatnonzero(got["trial_live"][0] & (got["trial_score"][0] == got["trial_score"][0].max()))
        assert len(top) >= 2 and got["best_trial"][0] == top[0]
    if name == "planted":
        assert np.array_equal(got["inlier"], c["planted"])
        assert [a.tolist() for a in R.inliers_per_pair(_call(c))] == [
            np.flatnonzero(c["planted"][s]).tolist() for s in O.pair_slices(c)]


def test_min_inliers_keeps_or_clears(cuda_device):
    c = O.case("tiny")
    got = _numpy(_call(c, min_inliers=3))
    _check_outcome(c, got, min_inliers=3)
    assert got["n_inliers"].tolist() == [0, 0, 0, 3, 4]
    cleared = _run("tiny")
    for k in ("best_trial", "score", "pose"):                                  # these stay as they were
        assert np.array_equal(got[k], cleared[k])
    assert cleared["n_inliers"].tolist() == [0] * 5 and not cleared["inlier"].any() and (cleared["sums"] == 0).all()
    assert np.array_equal(cleared["refit_pose"], np.tile(np.eye(4), (5, 1, 1)))


@pytest.mark.parametrize("name", O.CASES)
def test_sums_and_refit(cuda_device, name):
    """Each sum is within n * 2^-52 * sum |term| of math.fsum (any order of n additions stays inside
    it), n the pair's inlier count."""
    c, got = O.case(name), _run(name)
    want = _check_outcome(c, got)
    n = want["n_inliers"][:, None]
    bound = n * 2.0 ** -52 * want["sums_mag"]
    print(name, "worst err / bound", (np.abs(got["sums"] - want["sums"]) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(got["sums"] - want["sums"]) <= bound).all()
    assert np.array_equal(got["sums"][:, 0], want["n_inliers"].astype(np.float64))
    for p in range(len(n)):
        if want["n_inliers"][p] < c["min_inliers"]:
            assert np.array_equal(got["refit_pose"][p], np.eye(4))
        elif name == "planted":
            err = float(np.abs(got["refit_pose"][p] - _kabsch(want["sums"][p])).max())
            print("pair", p, "refit vs _kabsch of the oracle's sums", err, "bound", O.pose_bound("planted"))
            assert err <= O.pose_bound("planted")
            # 38 rows or more with noise of a tenth of inlier_dist: the fit is far inside inlier_dist
            assert np.abs(got["refit_pose"][p] - c["planted_pose"][p]).max() < c["inlier_dist"]


def test_runs_repeat_and_seeds_differ(cuda_device):
    c = O.case("weights")
    a, b = _numpy(_call(c)), _numpy(_call(c))
    for k in OUTPUTS + ("refit_pose",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["trial_idx"].tobytes() == _run("weights")["trial_idx"].tobytes()
    other = _numpy(_call(c, seed=c["seed"] + 1))
    assert not np.array_equal(other["trial_idx"], a["trial_idx"])
    assert np.array_equal(other["trial_idx"], O.draws(2, c["n_trials"], np.diff(c["pair_start"]), c["seed"] + 1)[0])


def test_split_calls(cuda_device):
    """A pair's result depends on its rows and its own index alone: pair 0 of `uneven` alone gives the
    joint call's bytes; pair 1 alone is pair 0 of its call, drawn as the oracle draws for p = 0."""
    c, joint = O.case("uneven"), _run("uneven")
    s0, s1 = O.pair_slices(c)
    T = c["n_trials"]

    def one(s):
        sub = dict(c, pts_a=c["pts_a"][s], pts_b=c["pts_b"][s], normals_a=c["normals_a"][s], normals_b=c["normals_b"][s],
                   pair_start=np.array([0, s.stop - s.start]))
        return sub, _numpy(_call(sub))

    _, first = one(s0)
    for k in OUTPUTS:
        want = joint[k][s0] if k == "inlier" else joint[k][:1]
        assert first[k].tobytes() == want.tobytes(), k
    sub, second = one(s1)
    assert np.array_equal(second["trial_idx"], O.draws(1, T, [600], c["seed"])[0])
    assert not np.array_equal(second["trial_idx"][0], joint["trial_idx"][1])
    assert np.array_equal(second["trial_score"], O.trial_scores(sub, second["trial_pose"], second["trial_live"]))
    _check_outcome(sub, second)
    assert np.array_equal(second["inlier"], c["planted"][s1])
    # lists of per-pair arrays in place of pair_start give the joint call
    res = R.ransac_pairs([c["pts_a"][s0], c["pts_a"][s1]], [c["pts_b"][s0], c["pts_b"][s1]], None,
                         [c["normals_a"][s0], c["normals_a"][s1]], [c["normals_b"][s0], c["normals_b"][s1]],
                         return_trials=True, device=cuda_device, **{k: c[k] for k in ARGS})
    listed = _numpy(res)
    for k in OUTPUTS:
        assert listed[k].tobytes() == joint[k].tobytes(), k


def test_degenerate_is_finite(cuda_device):
    got = _run("degenerate")
    for k in ("pose", "sums", "score", "trial_pose", "refit_pose"):
        assert np.isfinite(got[k]).all(), k
    assert np.isfinite(got["trial_pose"][got["trial_live"]]).all() and got["trial_live"].any()
    assert got["n_inliers"].tolist() == [50, 50]             # every row fits every live trial: the lowest wins
    assert [int(np.flatnonzero(got["trial_live"][p])[0]) for p in range(2)] == got["best_trial"].tolist()


def test_empty_call(cuda_device):
    res = R.ransac_pairs(np.zeros((0, 3)), np.zeros((0, 3)), np.array([0, 0, 0]), inlier_dist=0.01, device=cuda_device)
    assert res.best_trial.tolist() == [-1, -1] and res.n_inliers.tolist() == [0, 0] and len(res.inlier) == 0
    assert np.array_equal(res.pose.cpu().numpy(), np.tile(np.eye(4), (2, 1, 1))) and np.array_equal(res.refit_pose, res.pose.cpu().numpy())
