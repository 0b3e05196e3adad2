"""CPU: the pose-graph oracle (tests/pose_graph_oracle.py) against finite differences and planted
poses, the tie guard of the dense cases, and what the library and optimize_poses refuse before any
device work. No GPU is needed."""
import ctypes

import numpy as np
import pytest

from bundlesdf_amd import _lib
from bundlesdf_amd import pose_graph as PG
from tests import pose_graph_oracle as O

# weight 1e4 on two cases: at weight 1 the absolute 1e-6 guards of the PCG end the steps after the second
DENSE_CASES = {
    "r5": dict(seed=0, N=4, radius=5, w_dense=1e4),
    "r1": dict(seed=1, N=2, radius=1, rot=0.004, trans=0.0005),
    "far": dict(seed=2, N=4, radius=5, far_frame=True),
    "tie": dict(seed=3, N=4, radius=5, tie=True),
    "both": dict(seed=4, N=6, radius=5, with_sparse=True, w_dense=1e4, w_sparse=1e4),
}


def test_sparse_jacobians_match_central_differences():
    """r(d_i, d_j) = Exp(d_i) T_i pa - Exp(d_j) T_j pb: J_i = [-[a]x | I], J_j = -[-[b]x | I]. Step 1e-6:
    truncation ~ h^2 |a| / 6 ~ 1e-13, rounding ~ 2^-53 |a| / h ~ 1e-10; the bound is 1e-8."""
    rng = np.random.default_rng(0)
    Ti, Tj = O.rigid(rng.normal(0, 0.5, 3), rng.normal(0, 0.3, 3)), O.rigid(rng.normal(0, 0.5, 3), rng.normal(0, 0.3, 3))
    pa, pb = rng.normal(0, 0.3, (5, 3)), rng.normal(0, 0.3, (5, 3))
    Ja, Jb = O.jac(O.xform(Ti, pa)), O.jac(O.xform(Tj, pb))
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        di = (O.xform(O.apply_update(Ti, e), pa) - O.xform(O.apply_update(Ti, -e), pa)) / (2 * h)
        dj = -(O.xform(O.apply_update(Tj, e), pb) - O.xform(O.apply_update(Tj, -e), pb)) / (2 * h)
        assert np.abs(di - Ja[:, :, k]).max() < 1e-8
        assert np.abs(dj + Jb[:, :, k]).max() < 1e-8


def test_dense_jacobians_match_central_differences():
    """d = n_t . (p_t - (Exp(d_i) T_i)^-1 Exp(d_j) T_j p_s) at a held correspondence: J_i = +u, J_j = -u
    with u = [a x m, m]. Same step and bound as the sparse rows."""
    case = O.dense_case(**DENSE_CASES["r5"])
    poses = case["poses"]
    (i, j) = O.dense_pairs(case, poses)[0]
    idx = O.dense_search(case, poses, i, j)
    rows = O.dense_rows(case, poses, i, j, idx)
    assert len(rows["d"]) > 50
    keep = np.full_like(idx, -1)
    some = np.flatnonzero(idx >= 0)[::7]
    keep[some] = idx[some]
    u = O.dense_rows(case, poses, i, j, keep)["u"]

    def resid(Ti, Tj):
        p = [x.copy() for x in poses]
        p[i], p[j] = Ti, Tj
        return O.dense_rows(case, np.stack(p), i, j, keep)["d"]

    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        di = (resid(O.apply_update(poses[i], e), poses[j]) - resid(O.apply_update(poses[i], -e), poses[j])) / (2 * h)
        dj = (resid(poses[i], O.apply_update(poses[j], e)) - resid(poses[i], O.apply_update(poses[j], -e))) / (2 * h)
        assert np.abs(di - u[:, k]).max() < 1e-8
        assert np.abs(dj + u[:, k]).max() < 1e-8


def test_linearise_is_the_gradient_of_the_energy():
    """g = -sum w J^T r is minus half the gradient of the energy (rho' is the weight): central
    differences of the sparse energy along every variable of a free frame."""
    case = O.sparse_case(seed=3, N=3, counts=(40, 50))
    poses = np.asarray(case["poses"])
    L = O.linearise(case, poses)
    h = 1e-6
    for k in (1, 2):
        for c in range(6):
            e = np.zeros(6)
            e[c] = h
            Ep = O.linearise(case, [O.apply_update(T, e) if f == k else T for f, T in enumerate(poses)])["history"][0]
            Em = O.linearise(case, [O.apply_update(T, -e) if f == k else T for f, T in enumerate(poses)])["history"][0]
            assert abs(-(Ep - Em) / (2 * h) / 2 - L["g"][6 * k + c]) < 1e-7 * max(1.0, np.abs(L["g"]).max())


def test_planted_poses_are_recovered_sparse_only():
    """Exact matches of planted poses: the energy never rises from one linearisation to the next, ends
    below a thousandth of its start, and the final poses are ten times closer to the truth than the
    start: 7 x 5 Jacobi-preconditioned CG steps on 18 unknowns solve no step exactly, so the descent is
    linear, and one decimal order in the poses is the least that shows it. w_sparse is 1e4 because the
    reference's guards stop the PCG once p.Ap <= 1e-6, an absolute figure: at weight 1 and these few
    hundred millimetre-scale rows the steps end early (the energy stays at 1.6e-5 from the third on)."""
    case = O.sparse_case(seed=0, w_sparse=1e4)
    res = O.optimise(case)
    e = res["history"][:, 0]
    print("sparse energies", e)
    assert (np.diff(e) <= 0).all()
    start, end = O.pose_error(case["poses"], case["truth"]), O.pose_error(res["poses"], case["truth"])
    print("pose error", start, "->", end)
    assert end < 0.1 * start and e[-1] < 1e-3 * e[0]
    assert res["history"][0, 2] == (np.asarray(case["weight"]) != 0).sum()


@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_tie_guard_is_small_on_every_dense_case(name):
    """At most 2 % of the valid source pixels of a dense case are within the guard band of another
    choice, at the initial poses and along the oracle's own iterations."""
    case = O.dense_case(**DENSE_CASES[name])
    res = O.optimise(dict(case, n_outer=3))
    for poses in res["iter_poses"]:
        share, total = O.guarded_share(case, poses)
        assert total > 200
        assert share <= 0.02, (name, share)


def test_dense_cases_cover_their_shapes():
    """What the GPU dense tests rely on: a pair beyond max_rot_deg, equal valid counts, invalid normals
    with a valid depth, source pixels that project outside the image and windows across every border."""
    far = O.dense_case(**DENSE_CASES["far"])
    assert len(O.dense_pairs(far, far["poses"])) == 3              # the far frame pairs with nobody
    tie = O.dense_case(**DENSE_CASES["tie"])
    cnt = O.valid_mask(tie).sum(1)
    assert cnt[0] == cnt[1] and (0, 1) in O.dense_pairs(tie, tie["poses"])      # the higher index is the source
    case = O.dense_case(**DENSE_CASES["r5"])
    P = case["points"].reshape(4, -1, 3)
    assert ((P[1][:, 2] > 0.1) & ~O.valid_mask(case)[1]).any()
    H, W = case["points"].shape[1:3]
    K = case["K"]
    outside = lo_w = hi_w = lo_h = hi_h = False
    for (i, j) in O.dense_pairs(case, case["poses"]):
        R, t = O.relative(case["poses"][i], case["poses"][j])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        val = O.valid_mask(case)[j]
        q = O.xform(T, P[j].astype(np.float64))[val]
        u, v = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2], K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
        w0, h0 = np.rint(u), np.rint(v)
        outside |= bool(((w0 < 0) | (w0 >= W) | (h0 < 0) | (h0 >= H)).any())
        lo_w |= bool((w0 - 5 < 0).any())
        hi_w |= bool((w0 + 5 >= W).any())
        lo_h |= bool((h0 - 5 < 0).any())
        hi_h |= bool((h0 + 5 >= H).any())
    assert outside and lo_w and hi_w and lo_h and hi_h


def test_pcg_routes_agree_and_solve():
    rng = np.random.default_rng(5)
    B = rng.normal(size=(30, 12))
    A = B.T @ B + np.eye(12)
    g = rng.normal(size=12)
    A, g = 1e6 * A, 1e6 * g                 # far above the absolute 1e-6 guards
    x = O.pcg(A, g, 12)
    assert np.abs(A @ x - g).max() < 1e-8 * np.abs(g).max()
    assert O.pcg_gap(A, g, 5) < 1e-12


# ----------------------------------------------------------------------------- refused before device work
def _good_kwargs():
    case = O.dense_case(seed=0, N=3, with_sparse=True)
    return dict(poses=case["poses"], pair_frames=case["pair_frames"], pts_a=case["pts_a"], pts_b=case["pts_b"],
                pair_start=case["pair_start"], points=case["points"], normals=case["normals"], K=case["K"])


def test_optimize_poses_refuses_bad_inputs_before_device_work():
    kw = _good_kwargs()
    with pytest.raises(ValueError, match="fixed"):
        PG.optimize_poses(**dict(kw, fixed=np.zeros(3, bool)))
    with pytest.raises(ValueError, match="neither"):
        PG.optimize_poses(kw["poses"])
    with pytest.raises(ValueError, match="N=129"):
        PG.optimize_poses(np.tile(np.eye(4), (129, 1, 1)), points=np.zeros((129, 2, 2, 3), np.float32),
                          normals=np.zeros((129, 2, 2, 3), np.float32), K=np.eye(3))
    bad = kw["pair_start"].copy()
    bad[1] = bad[2] + 1
    with pytest.raises(ValueError, match="pair_start"):
        PG.optimize_poses(**dict(kw, pair_start=bad))
    bad = kw["pair_frames"].copy()
    bad[0, 1] = 3
    with pytest.raises(ValueError, match="frame index"):
        PG.optimize_poses(**dict(kw, pair_frames=bad))
    with pytest.raises(ValueError, match="normals"):
        PG.optimize_poses(**dict(kw, normals=kw["normals"][:, :-1]))
    with pytest.raises(ValueError, match="points"):
        PG.optimize_poses(**dict(kw, points=kw["points"][:2]))


def test_library_refuses_bad_descriptors_before_device_work():
    """nof_pose_graph_optimize validates the whole descriptor before its first HIP call: NOF_EINVAL with
    nof_last_error naming the field, on a machine with no GPU."""
    L = _lib.lib()

    def desc(**kw):
        D = _lib.PoseGraphDesc()
        one = ctypes.c_void_p(256)                  # never dereferenced: validation fails first
        D.poses = D.fixed = D.poses_out = D.history = D.workspace = one
        D.pair_frames = D.pts_a = D.pts_b = D.pair_start = one
        D.N, D.n_outer, D.n_inner, D.P, D.M = 4, 7, 5, 2, 10
        D.robust_delta, D.w_sparse, D.w_dense, D.dist_thresh = 0.005, 1.0, 1.0, 0.01
        for k, v in kw.items():
            setattr(D, k, v)
        return D

    def refused(D, word):
        assert L.nof_pose_graph_optimize(ctypes.byref(D), None) != 0
        assert word in L.nof_last_error(), L.nof_last_error()

    refused(desc(N=129), b"N=129")
    refused(desc(N=0), b"N=0")
    refused(desc(P=0, pair_frames=None), b"neither")
    refused(desc(n_outer=0), b"n_outer=0")
    refused(desc(robust_delta=0.0), b"robust_delta")
    refused(desc(pair_start=None), b"pair_start is NULL")
    refused(desc(points=ctypes.c_void_p(256)), b"normals is NULL")
    refused(desc(points=ctypes.c_void_p(256), normals=ctypes.c_void_p(256), H=0, W=4), b"H=0")
    refused(desc(points=ctypes.c_void_p(256), normals=ctypes.c_void_p(256), H=4, W=4, radius=33), b"radius=33")
    refused(desc(history=None), b"history is NULL")
    refused(desc(workspace_bytes=16), b"workspace_bytes=16")
    assert L.nof_pose_graph_workspace_bytes(129, 0, 0, 0, 0) == 0
    assert L.nof_pose_graph_workspace_bytes(4, 2, 10, 24, 32) >= 4 * 128 + 24 * 24 * 8
