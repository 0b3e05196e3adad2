"""GPU: nof_pose_graph_optimize (csrc/pose_graph.hip) against tests/pose_graph_oracle.py, iteration by
iteration on the kernel's own poses: the dense correspondences exactly (outside the tie guard), A and
g against math.fsum over the kernel's own correspondences within the first-order summation bound, the
PCG step within 16 times the gap between the oracle's float64 and long-double routes, then the whole
optimisation against the oracle and against the planted truth, determinism and stream use.

The summation bound. A term of a sum (w dot(J_r, J_c), (w u_r) u_c, (w u_r) d, w0 rho) is computed by
the oracle with the kernel's float64 operations in the kernel's order, from the same poses, float32
maps (exact in float64) and correspondences: where +, -, x, / and sqrt are correctly rounded on both
sides the terms are the same bits. Only the Huber weight goes through a sqrt and a division (w =
delta / sqrt(e), rho = 2 sqrt(e) delta - delta^2); allowing each to be one ulp off on the device moves
a term by at most 4 x 2^-53 of its size. The kernel adds the n terms of an entry in a tree of n - 1
additions (lane, butterfly, waves, chunks, pairs; adding the zero of an empty lane or chunk is exact),
each rounding by at most 2^-53 of a partial sum that is at most sum |term|. So |kernel - fsum| <=
(n - 1 + 4) 2^-53 sum |term| to first order, and the tests use (n + c) 2^-53 sum |term| with c = 4."""
import numpy as np
import pytest
import torch

from bundlesdf_amd import pose_graph as PG
from tests import pose_graph_oracle as O
from tests.test_pose_graph_cpu import DENSE_CASES

pytestmark = pytest.mark.gpu

C_TERM = 4
U = 2.0 ** -53

SPARSE_CASES = {
    "planted": dict(seed=0, N=4, w_sparse=1e4),                              # pairs of 0, 1, 65, 600, 40, 130 rows, zero weights
    "two": dict(seed=1, N=2, counts=(65, 1, 0), zero_weights=False),
    "lonely": dict(seed=2, N=5, lonely=3),                                   # free frame 3 is touched by nothing
    "one_free": dict(seed=3, N=4, fixed=(True, True, False, True)),
    "six": dict(seed=4, N=6, counts=(300, 7, 0, 65, 257, 12, 90, 33), w_sparse=1e4),
}
GPU_DENSE = dict(DENSE_CASES, both=dict(DENSE_CASES["both"], n_outer=3))    # N = 6: fewer steps keep the test short

_RUNS = {}


def _case(name):
    if name in SPARSE_CASES:
        return O.sparse_case(**SPARSE_CASES[name])
    return O.dense_case(**GPU_DENSE[name])


def _call(case, dev, **kw):
    keys = ("pair_frames", "pts_a", "pts_b", "pair_start", "weight", "points", "normals", "K", "fixed") + tuple(O.DEFAULTS)
    args = {k: case[k] for k in keys if case.get(k) is not None}
    args.update(kw)
    return PG.optimize_poses(case["poses"], device=dev, **args)


def _run(name, dev):
    """One debug run per case, shared by the tests (read-only)."""
    if name not in _RUNS:
        case = _case(name)
        poses, history, dbg = _call(case, dev, return_debug=True)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in dbg.items()}
        out.update(poses=poses.cpu().numpy(), history=history.cpu().numpy())
        _RUNS[name] = (case, out)
    return _RUNS[name]


def _check_iterations(name, case, out):
    n_outer, n_inner = int(O._param(case, "n_outer")), int(O._param(case, "n_inner"))
    dense = case.get("points") is not None
    assert out["iter_poses"].shape[0] == n_outer + 1
    assert np.array_equal(out["iter_poses"][0], case["poses"]) and np.array_equal(out["iter_poses"][-1], out["poses"])
    val = O.valid_mask(case) if dense else None
    for k in range(n_outer):
        poses = out["iter_poses"][k]
        if dense:
            got = out["dense_index"][k]
            active = O.dense_pairs(case, poses)
            for i in range(len(poses)):
                for j in range(len(poses)):
                    if (i, j) not in active:
                        assert (got[i, j] == -1).all(), (name, k, i, j)
            guarded = total = 0
            for (i, j) in active:
                want, guard = O.dense_search(case, poses, i, j, want_guard=True)
                assert np.array_equal(got[i, j][~guard], want[~guard]), (name, k, i, j)
                guarded += int((guard & val[j]).sum())
                total += int(val[j].sum())
            assert guarded <= 0.02 * total, (name, k, guarded, total)
        L = O.linearise(case, poses, dense_index=out["dense_index"][k] if dense else None, how="fsum", bounds=True)
        errA, errg = np.abs(out["A"][k] - L["A"]), np.abs(out["g"][k] - L["g"])
        bA, bg = (L["A_n"] + C_TERM) * U * L["A_abs"], (L["g_n"] + C_TERM) * U * L["g_abs"]
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"{name} k={k}: A worst err/bound {np.nanmax(np.where(bA > 0, errA / bA, 0)):.3f}, "
                  f"g {np.nanmax(np.where(bg > 0, errg / bg, 0)):.3f}, terms up to {L['A_n'].max()}")
        assert (errA <= bA).all(), (name, k)
        assert (errg <= bg).all(), (name, k)
        assert np.array_equal(out["A"][k], out["A"][k].T)
        # energies: sums of non-negative terms, the same bound with sum |term| = the sum itself
        h, hw = out["history"][k], L["history"]
        assert h[2] == hw[2] and h[3] == hw[3], (name, k, h, hw)
        assert abs(h[0] - hw[0]) <= (hw[2] + C_TERM) * U * hw[0] and abs(h[1] - hw[1]) <= (hw[3] + C_TERM) * U * hw[1]
        x = O.pcg(out["A"][k], out["g"][k], n_inner)
        gap = O.pcg_gap(out["A"][k], out["g"][k], n_inner)
        far = float(np.abs(out["delta"][k] - x).max())
        floor = float(np.spacing(np.abs(x).max()))
        print(f"{name} k={k}: pcg route gap {gap:.3e}, kernel away {far:.3e}, floor {floor:.3e}")
        assert far <= 16 * gap + floor, (name, k, far, gap)
        fixed = np.repeat(np.asarray(case["fixed"], bool), 6)
        assert (out["delta"][k][fixed] == 0).all()


@pytest.mark.parametrize("name", sorted(SPARSE_CASES))
def test_sparse_iterations_match_the_oracle(cuda_device, name):
    case, out = _run(name, cuda_device)
    _check_iterations(name, case, out)


@pytest.mark.parametrize("name", sorted(SPARSE_CASES))
def test_sparse_end_to_end(cuda_device, name):
    """No discrete choice on the sparse term: the final poses are within 16 route gaps (plus one ulp of
    the largest entry) of the oracle's."""
    case, out = _run(name, cuda_device)
    want = O.optimise(case)
    gap = O.route_gap(case)
    far = float(np.abs(out["poses"] - want["poses"]).max())
    floor = float(np.spacing(np.abs(want["poses"]).max()))
    print(f"{name}: route gap {gap:.3e}, kernel away {far:.3e}, floor {floor:.3e}")
    assert far <= 16 * gap + floor
    fixed = np.asarray(case["fixed"], bool)
    assert np.array_equal(out["poses"][fixed], np.asarray(case["poses"])[fixed])
    assert np.allclose(out["history"], want["history"], rtol=1e-6, atol=0)
    start, end = O.pose_error(case["poses"], case["truth"]), O.pose_error(out["poses"], case["truth"])
    print(f"{name}: pose error {start:.3e} -> {end:.3e}")
    assert end < start


def test_untouched_free_frame_comes_back_bit_identical(cuda_device):
    case, out = _run("lonely", cuda_device)
    assert not case["fixed"][3] and 3 not in case["pair_frames"]
    assert out["poses"][3].tobytes() == np.asarray(case["poses"][3], np.float64).tobytes()
    assert (out["delta"][:, 18:24] == 0).all()
    far_case, far = _run("far", cuda_device)
    assert far["poses"][-1].tobytes() == np.asarray(far_case["poses"][-1], np.float64).tobytes()
    assert (far["dense_index"][:, -1] == -1).all() and (far["dense_index"][:, :, -1] == -1).all()


@pytest.mark.parametrize("name", sorted(GPU_DENSE))
def test_dense_iterations_and_recovery(cuda_device, name):
    """The per-iteration checks at every k, and the poses end strictly closer to the planted truth than
    they started (pose_error: the frames' worst entries, averaged)."""
    case, out = _run(name, cuda_device)
    _check_iterations(name, case, out)
    start, end = O.pose_error(case["poses"], case["truth"]), O.pose_error(out["poses"], case["truth"])
    print(f"{name}: pose error {start:.3e} -> {end:.3e}, history {out['history'][[0, -1]]}")
    assert end < start
    assert out["history"][0, 3] > 200


@pytest.mark.parametrize("name", ["six", "both"])
def test_two_calls_give_the_same_bytes(cuda_device, name):
    case, out = _run(name, cuda_device)
    poses, history, dbg = _call(case, cuda_device, return_debug=True)
    torch.cuda.synchronize()
    assert poses.cpu().numpy().tobytes() == out["poses"].tobytes()
    assert history.cpu().numpy().tobytes() == out["history"].tobytes()
    for k, v in dbg.items():
        assert v.cpu().numpy().tobytes() == out[k].tobytes(), k


def test_call_on_another_stream(cuda_device):
    case, out = _run("both", cuda_device)
    s = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(s):
        poses, history = _call(case, cuda_device)
    s.synchronize()
    assert poses.cpu().numpy().tobytes() == out["poses"].tobytes()
    assert history.cpu().numpy().tobytes() == out["history"].tobytes()


def test_ransac_output_feeds_in(cuda_device):
    """weight=result.inlier (bool) composes without compaction: gross outliers that RANSAC flags do not
    move the result away from the run on the clean rows alone."""
    from bundlesdf_amd.ransac import ransac_pairs
    case = O.sparse_case(seed=6, N=3, counts=(80, 90), zero_weights=False)
    rng = np.random.default_rng(6)
    bad = rng.uniform(size=170) < 0.2
    b = case["pts_b"].copy()
    b[bad] += rng.uniform(0.05, 0.1, (int(bad.sum()), 3))
    res = ransac_pairs(case["pts_a"], b, case["pair_start"], inlier_dist=0.003, n_trials=500, device=cuda_device)
    assert np.array_equal(res.inlier.cpu().numpy(), ~bad)
    poses, _ = PG.optimize_poses(case["poses"], pair_frames=case["pair_frames"], pts_a=case["pts_a"], pts_b=b,
                                 pair_start=res.pair_start, weight=res.inlier, device=cuda_device)
    clean, _ = PG.optimize_poses(case["poses"], pair_frames=case["pair_frames"], pts_a=case["pts_a"], pts_b=case["pts_b"],
                                 pair_start=case["pair_start"], weight=(~bad).astype(np.float32), device=cuda_device)
    assert poses.cpu().numpy().tobytes() == clean.cpu().numpy().tobytes()
