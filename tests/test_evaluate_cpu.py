"""CPU: the host side of bundlesdf_amd.evaluate (compute_auc, the first-frame alignment, the rigid-pose
check), the argument checks of the two new entry points, and the fairness of every seeded cloud pair
the GPU tests compare exactly (tests/nearest_oracle.py): no query with two equally near points, and
the brute force agrees with scipy's cKDTree."""
import ctypes
import os
import re

import numpy as np
import pytest

from bundlesdf_amd import evaluate as E
from tests import nearest_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1   # NOF_EINVAL, include/nof.h


def _auc_loop(errs, max_val):
    """The curve by hand: sorted errors below max_val, a step of height (rank / n) ending at each, and
    the last height held up to max_val."""
    e = sorted(float(x) for x in errs)
    n = len(e)
    area, prev_x, height = 0.0, 0.0, 0.0
    for rank, x in enumerate(e, 1):
        if not x < max_val:
            break
        height = rank / n
        area += (x - prev_x) * height
        prev_x = x
    if height == 0.0:
        return 0.0
    area += (max_val - prev_x) * height
    return area / max_val


def test_compute_auc_values():
    assert abs(E.compute_auc([0.02, 0.05, 0.2]) - 0.6) <= 1e-12
    assert E.compute_auc([]) == 0
    assert E.compute_auc([0.3]) == 0.0
    assert E.compute_auc(np.zeros(4)) == 1.0
    # repeated errors: a zero-width step; (0.05 * 1/2 + 0.05 * 1) / 0.1
    assert abs(E.compute_auc([0.05, 0.05]) - 0.75) <= 1e-12


@pytest.mark.parametrize("max_val", [0.1, 0.05])
def test_compute_auc_against_float_loop(max_val):
    errs = np.random.default_rng(0).uniform(0, 0.15, 50)
    assert (errs < max_val).any() and (errs >= max_val).any()
    assert abs(E.compute_auc(errs, max_val) - _auc_loop(errs, max_val)) <= 1e-12
    assert abs(E.compute_auc(list(errs[::-1]), max_val) - _auc_loop(errs, max_val)) <= 1e-12


def test_first_frame_alignment():
    rng = np.random.default_rng(1)
    pred = np.stack([O.rigid(rng.normal(0, 1, 3), rng.normal(0, 0.3, 3)) for _ in range(6)])
    gt = np.stack([O.rigid(rng.normal(0, 1, 3), rng.normal(0, 0.3, 3)) for _ in range(6)])
    al = E.align_first_frame(pred, gt)
    assert al.shape == (6, 4, 4)
    np.testing.assert_allclose(al[0], gt[0], rtol=0, atol=1e-14)
    for f in range(6):   # the relative motion from frame 0 is the predicted one
        want = pred[f] @ np.linalg.inv(pred[0]) @ gt[0]
        np.testing.assert_allclose(al[f], want, rtol=0, atol=1e-14)
    # a track that is the ground truth seen from another object frame aligns onto the ground truth
    off = O.rigid([0.3, -0.2, 0.5], [0.1, 0.2, -0.3])
    np.testing.assert_allclose(E.align_first_frame(gt @ off, gt), gt, rtol=0, atol=1e-13)
    assert E.align_first_frame(np.zeros((0, 4, 4)), np.zeros((0, 4, 4))).shape == (0, 4, 4)


def test_non_rigid_pose_raises_before_device_work():
    """The check is on the host and comes first: this passes on a machine with no GPU."""
    model = np.random.default_rng(2).uniform(-0.1, 0.1, (50, 3))
    good = O.rigid([0.1, 0.2, 0.3], [0.0, 0.1, 0.2])
    sheared = good.copy()
    sheared[0, 1] += 1e-3
    scaled = good.copy()
    scaled[:3, :3] *= 1.0 + 1e-5
    for fn in (E.adi_err, E.add_err):
        for bad in (sheared, scaled):
            with pytest.raises(ValueError, match="not rigid"):
                fn(bad, good, model)
            with pytest.raises(ValueError, match="not rigid"):
                fn(np.stack([good, good]), np.stack([good, bad]), model)
    with pytest.raises(ValueError, match="2 predicted poses, 1 ground-truth"):
        E.adi_err(np.stack([good, good]), good[None], model)


@pytest.mark.parametrize("name", O.CASES)
def test_gpu_cloud_pairs_are_fair(name):
    from scipy.spatial import cKDTree
    c = O.case(name)
    cloud, queries = c["cloud"], c["queries"]
    for T in (c["T"] if c["T"] is not None else [None]):
        q = queries if T is None else O.transform(T, queries)
        dist, idx = O.nearest(queries, cloud, T)
        kd_dist, kd_idx = cKDTree(cloud).query(q)
        if c["ties"]:
            assert (O.top2_gap(queries, cloud, T) == 0).sum() >= 100     # the case does exercise the rule
            same = np.all(cloud[idx] == cloud[kd_idx], axis=1)           # cKDTree may name another copy
            assert same.all()
            d2 = O.d2_matrix(q, cloud)
            assert np.array_equal(idx, np.array([np.flatnonzero(r == r.min())[0] for r in d2]))
        else:
            if len(cloud) > 1:
                assert (O.top2_gap(queries, cloud, T) > 0).all()
            assert np.array_equal(idx, kd_idx)
        np.testing.assert_allclose(dist, kd_dist, rtol=1e-14, atol=0)
    if c["max_dist"] is not None:
        miss = (O.expected(name)[1] < 0).mean()
        assert 0.4 < miss < 0.6


def test_new_symbols_declared_in_header_and_binding():
    from bundlesdf_amd import _lib
    src = open(os.path.join(ROOT, "include", "nof.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("nof_nearest_points", "nof_correspondence_moments", "nof_nearest_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.declared_symbols(), name


def test_entry_points_validate_before_device_work():
    """Bad arguments are NOF_EINVAL with null device pointers and no GPU; empty work returns 0 at once."""
    from bundlesdf_amd import build, _lib
    build.build()
    L = _lib.lib()
    org = (ctypes.c_double * 3)(0, 0, 0)
    one = ctypes.c_void_p(8)      # a non-null pointer that is never dereferenced on these paths

    def nn(Q=4, B=1, xf=None, start=one, cpts=one, ids=one, n=5, origin=org, dims=(2, 2, 2), cell=0.5, md=0.0,
           queries=one, index=one, dist=one):
        dm = (ctypes.c_int32 * 3)(*dims) if dims is not None else None
        return L.nof_nearest_points(queries, Q, xf, B, start, cpts, ids, n, origin, dm, cell, md, index, dist, None)

    for kw in (dict(Q=-1), dict(B=-1, xf=one), dict(n=-1), dict(B=2), dict(B=70000, xf=one), dict(origin=None),
               dict(dims=None), dict(cell=0.0), dict(cell=float("nan")), dict(md=float("nan")), dict(start=None),
               dict(dims=(0, 2, 2)), dict(dims=(2, -1, 2)), dict(dims=(1 << 9, 1 << 9, (1 << 8) + 1)),
               dict(n=0), dict(queries=None), dict(cpts=None), dict(ids=None), dict(index=None), dict(dist=None)):
        assert nn(**kw) == EINVAL, kw
        assert "nearest_points" in L.nof_last_error().decode()
    assert nn(n=0) == EINVAL and "empty cloud" in L.nof_last_error().decode()
    assert nn(Q=0, n=0, queries=None, index=None, dist=None) == 0
    assert nn(B=0, xf=one) == 0

    def mom(src=one, n=4, tgt=one, m=4, index=one, dist=one, sums=one, ws=one):
        return L.nof_correspondence_moments(src, n, None, tgt, m, index, dist, sums, ws, None)

    for kw in (dict(n=-1), dict(m=-1), dict(src=None), dict(tgt=None), dict(index=None), dict(dist=None),
               dict(sums=None), dict(ws=None)):
        assert mom(**kw) == EINVAL, kw
        assert "correspondence_moments" in L.nof_last_error().decode()
    assert L.nof_nearest_workspace_bytes(1) == 17 * 8
    assert L.nof_nearest_workspace_bytes(257) == 2 * 17 * 8
    assert L.nof_nearest_workspace_bytes(1 << 30) == 1024 * 17 * 8
