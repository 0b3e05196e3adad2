"""numpy float64 restatement of what bundlesdf_amd.ransac must compute (include/nof.h group 8), written
for the tests: the hash and the draws, the three-point rigid fit by two routes (Kabsch through
np.linalg.svd, Horn's quaternion through np.linalg.eigh), the gates, the inlier test and the
fixed-point score in the header's operation order, the winner rule, the refit sums with math.fsum,
and the seeded cases the CPU and GPU tests share."""
import functools
import math

import numpy as np

from bundlesdf_amd.ransac import ROW_TILE

FAIR_REL = 1e-9      # no tested value lies this close to its threshold (tests/test_ransac_cpu.py)


# ----------------------------------------------------------------------------- sampling
def hash32(x):
    x = np.array(x, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def draws(P, T, counts, seed):
    """(idx [P,T,3] i32 local rows, ok [P,T]: n_p >= 3 and three different rows)."""
    p = np.arange(P, dtype=np.uint64)[:, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None]
    j = np.arange(3, dtype=np.uint64)[None, None, :]
    counter = (((p * np.uint64(T) + t) * np.uint64(3) + j) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    u = hash32(counter ^ hash32(np.uint32(int(seed) & 0xFFFFFFFF)))
    n = np.asarray(counts, np.uint64)[:, None, None]
    idx = ((u.astype(np.uint64) * n) >> np.uint64(32)).astype(np.int32)
    ok = (idx[..., 0] != idx[..., 1]) & (idx[..., 0] != idx[..., 2]) & (idx[..., 1] != idx[..., 2])
    return idx, ok & (np.asarray(counts)[:, None] >= 3)


# ----------------------------------------------------------------------------- hypotheses
def _centred(a, b):
    am, bm = a.mean(1), b.mean(1)
    return am, bm, a - am[:, None], b - bm[:, None]


def fit_svd(a, b):
    """Kabsch with the reflection fix. a, b [T,3,3] (trial, point, coordinate) -> (R [T,3,3], t [T,3])."""
    am, bm, ac, bc = _centred(a, b)
    H = np.einsum("tir,tic->trc", ac, bc)
    U, _, Vt = np.linalg.svd(H)
    V, Ut = Vt.transpose(0, 2, 1), U.transpose(0, 2, 1)
    d = np.sign(np.linalg.det(V @ Ut))
    d[d == 0] = 1.0
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ Ut
    return R, bm - np.einsum("trc,tc->tr", R, am)


def fit_horn(a, b):
    """Horn 1987: the quaternion is the eigenvector of the largest eigenvalue of N(S)."""
    am, bm, ac, bc = _centred(a, b)
    S = np.einsum("tir,tic->trc", ac, bc)
    N = np.empty((len(S), 4, 4))
    N[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    N[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    N[:, 2, 2] = -S[:, 0, 0] + S[:, 1, 1] - S[:, 2, 2]
    N[:, 3, 3] = -S[:, 0, 0] - S[:, 1, 1] + S[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    _, vec = np.linalg.eigh(N)
    q = vec[:, :, 3]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    return R, bm - np.einsum("trc,tc->tr", R, am)


def sigma_ratio(a, b):
    """sigma_2 / sigma_1 of the sample's cross-covariance (0 where sigma_1 is 0)."""
    _, _, ac, bc = _centred(a, b)
    s = np.linalg.svd(np.einsum("tir,tic->trc", ac, bc), compute_uv=False)
    return np.where(s[:, 0] > 0, s[:, 1] / np.where(s[:, 0] > 0, s[:, 0], 1.0), 0.0)


def pose12(R, t):
    return np.concatenate([R, t[:, :, None]], 2).reshape(len(R), 12)


# ----------------------------------------------------------------------------- gates, inliers, scores
def gate_values(poses):
    """(|t|^2, trace) of poses [..., 12] in the header's order."""
    tx, ty, tz = poses[..., 3], poses[..., 7], poses[..., 11]
    return (tx * tx + ty * ty) + tz * tz, (poses[..., 0] + poses[..., 5]) + poses[..., 10]


def gate(poses, max_trans_sq, min_trace):
    t2, tr = gate_values(poses)
    with np.errstate(invalid="ignore"):
        return np.isfinite(poses).all(-1) & (t2 <= max_trans_sq) & (tr >= min_trace)


def inlier_values(poses, a, b, na=None, nb=None):
    """poses [T,12], rows [n,3] -> (d2 [T,n], dot [T,n] or None), every product and sum rounded once."""
    T = poses[:, None, :]
    ax, ay, az = a[None, :, 0], a[None, :, 1], a[None, :, 2]
    d = [b[None, :, k] - (((T[..., 4 * k] * ax + T[..., 4 * k + 1] * ay) + T[..., 4 * k + 2] * az) + T[..., 4 * k + 3])
         for k in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if na is None:
        return d2, None
    nx, ny, nz = na[None, :, 0], na[None, :, 1], na[None, :, 2]
    r = [(T[..., 4 * k] * nx + T[..., 4 * k + 1] * ny) + T[..., 4 * k + 2] * nz for k in range(3)]
    return d2, (r[0] * nb[None, :, 0] + r[1] * nb[None, :, 1]) + r[2] * nb[None, :, 2]


def inlier_test(poses, a, b, na, nb, dist_sq, cos_normal):
    d2, dot = inlier_values(poses, a, b, na, nb)
    return (d2 <= dist_sq) if dot is None else (d2 <= dist_sq) & (dot >= cos_normal)


def weights(conf, n):
    return np.full(n, 65536, np.int64) if conf is None else np.rint(np.asarray(conf, np.float64) * 65536.0).astype(np.int64)


def winner(score, live):
    """(best_trial, score): the live trial of the highest score above 0, the lowest among equals; else (-1, 0)."""
    s = np.where(live, score, 0)
    if len(s) == 0 or s.max() <= 0:
        return -1, 0
    return int(np.argmax(s)), int(s.max())          # argmax returns the first maximum


def refit_sums(a, b):
    """(sums [17], magnitudes [17]) over rows a, b with the identity transform, by math.fsum."""
    d = b - a
    cols = [np.ones(len(a))] + [a[:, k] for k in range(3)] + [b[:, k] for k in range(3)]
    cols += [a[:, r] * b[:, c] for r in range(3) for c in range(3)]
    cols += [(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]]
    return np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols])


# ----------------------------------------------------------------------------- the whole call
def settings(c):
    """Per-pair gate bounds and the scalar thresholds, as ransac_pairs derives them."""
    P = len(c["pair_start"]) - 1
    mt = np.full(P, np.inf) if c["max_trans"] is None else np.broadcast_to(np.asarray(c["max_trans"], np.float64), (P,))
    mr = np.full(P, np.inf) if c["max_rot_deg"] is None else np.broadcast_to(np.asarray(c["max_rot_deg"], np.float64), (P,))
    min_trace = np.where(np.isinf(mr), -np.inf, 1.0 + 2.0 * np.cos(np.deg2rad(np.minimum(mr, 180.0))))
    cos_normal = -math.inf if c["normal_angle_deg"] is None else math.cos(math.radians(float(c["normal_angle_deg"])))
    return mt * mt, min_trace, float(c["inlier_dist"]) * float(c["inlier_dist"]), cos_normal


def pair_slices(c):
    ps = np.asarray(c["pair_start"])
    return [slice(int(ps[p]), int(ps[p + 1])) for p in range(len(ps) - 1)]


def hypotheses(c, route="svd"):
    """The oracle's own trials -> dict(idx [P,T,3], ok, poses [P,T,12], live [P,T], ratio [P,T])."""
    sl = pair_slices(c)
    P, T = len(sl), c["n_trials"]
    counts = [s.stop - s.start for s in sl]
    idx, ok = draws(P, T, counts, c["seed"])
    max_trans_sq, min_trace, _, _ = settings(c)
    poses, ratio = np.zeros((P, T, 12)), np.zeros((P, T))
    live = np.zeros((P, T), bool)
    fit = fit_svd if route == "svd" else fit_horn
    for p, s in enumerate(sl):
        k = np.flatnonzero(ok[p])
        if len(k) == 0:
            continue
        a, b = c["pts_a"][s][idx[p, k]], c["pts_b"][s][idx[p, k]]
        poses[p, k] = pose12(*fit(a, b))
        ratio[p, k] = sigma_ratio(a, b)
        live[p, k] = gate(poses[p, k], max_trans_sq[p], min_trace[p])
    return dict(idx=idx, ok=ok, poses=poses, live=live, ratio=ratio)


def _normals(c, s):
    return (None, None) if c["normals_a"] is None else (c["normals_a"][s], c["normals_b"][s])


def trial_scores(c, poses, live):
    """int64 [P,T]: the fixed-point score of every live trial of the given poses; dead trials 0."""
    _, _, dist_sq, cos_normal = settings(c)
    out = np.zeros(poses.shape[:2], np.int64)
    for p, s in enumerate(pair_slices(c)):
        n = s.stop - s.start
        if n == 0:
            continue
        na, nb = _normals(c, s)
        w = weights(None if c["conf"] is None else c["conf"][s], n)
        inl = inlier_test(poses[p], c["pts_a"][s], c["pts_b"][s], na, nb, dist_sq, cos_normal)
        out[p] = np.where(live[p], (inl * w[None, :]).sum(1), 0)
    return out


def finish(c, poses, live, scores, min_inliers=None):
    """The winner rule, the flags, min_inliers and the refit sums applied to given trial arrays."""
    _, _, dist_sq, cos_normal = settings(c)
    min_inliers = c["min_inliers"] if min_inliers is None else min_inliers
    sl = pair_slices(c)
    P, M = len(sl), len(c["pts_a"])
    out = dict(best_trial=np.zeros(P, np.int32), score=np.zeros(P, np.int64), pose=np.tile(np.eye(4), (P, 1, 1)),
               inlier=np.zeros(M, bool), n_inliers=np.zeros(P, np.int32), sums=np.zeros((P, 17)),
               sums_mag=np.zeros((P, 17)))
    for p, s in enumerate(sl):
        bt, sc = winner(scores[p], live[p])
        out["best_trial"][p], out["score"][p] = bt, sc
        if bt < 0:
            continue
        out["pose"][p, :3, :] = poses[p, bt].reshape(3, 4)
        na, nb = _normals(c, s)
        inl = inlier_test(poses[p, bt][None], c["pts_a"][s], c["pts_b"][s], na, nb, dist_sq, cos_normal)[0]
        if inl.sum() < min_inliers:
            continue
        out["inlier"][s] = inl
        out["n_inliers"][p] = inl.sum()
        out["sums"][p], out["sums_mag"][p] = refit_sums(c["pts_a"][s][inl], c["pts_b"][s][inl])
    return out


# ----------------------------------------------------------------------------- cases
def rotation(rotvec):
    r = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pair(rng, n, inlier_dist, share=0.6, rot_deg=20.0, trans=0.2):
    """One pair: n rows, round(share n) of them moved by a planted pose with noise sigma = inlier_dist / 10
    (clipped at 3 sigma per axis), the others displaced by 10 .. 30 inlier_dist; unit normals, those of
    the planted rows rotated and tilted by at most 5 degrees."""
    R = rotation(_unit(rng.normal(size=3)) * math.radians(rot_deg))
    t = _unit(rng.normal(size=3)) * trans
    a = rng.uniform(-0.3, 0.3, (n, 3))
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:int(round(share * n))]] = True
    noise = np.clip(rng.normal(0, inlier_dist / 10, (n, 3)), -0.3 * inlier_dist, 0.3 * inlier_dist)
    away = _unit(rng.normal(size=(n, 3))) * rng.uniform(10, 30, (n, 1)) * inlier_dist
    b = a @ R.T + t + np.where(planted[:, None], noise, away)
    na = _unit(rng.normal(size=(n, 3)))
    tilt = np.stack([rotation(_unit(v) * math.radians(d)) for v, d in zip(rng.normal(size=(n, 3)), rng.uniform(0, 5, n))]) \
        if n else np.zeros((0, 3, 3))
    nb = np.where(planted[:, None], np.einsum("nrc,nc->nr", tilt, na @ R.T), _unit(rng.normal(size=(n, 3))))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(a=a, b=b, na=na, nb=nb, planted=planted, pose=T)


def _join(pairs, **kw):
    c = dict(pts_a=np.concatenate([q["a"] for q in pairs]), pts_b=np.concatenate([q["b"] for q in pairs]),
             normals_a=np.concatenate([q["na"] for q in pairs]), normals_b=np.concatenate([q["nb"] for q in pairs]),
             pair_start=np.concatenate([[0], np.cumsum([len(q["a"]) for q in pairs])]).astype(np.int64),
             planted=np.concatenate([q["planted"] for q in pairs]), planted_pose=np.stack([q["pose"] for q in pairs]),
             conf=None, inlier_dist=0.01, normal_angle_deg=20.0, n_trials=256, max_trans=None, max_rot_deg=None,
             min_inliers=5, seed=0)
    c.update(kw)
    if c["normal_angle_deg"] is None:
        c["normals_a"] = c["normals_b"] = None
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


TAIL_TRIALS = (1, 255, 257)
CASES = ("planted", "weights", "gated", "no_normals", "tiny", "degenerate", "uneven", "duplicated_best") + tuple(
    f"tails_T{t}" for t in TAIL_TRIALS)


@functools.lru_cache(maxsize=None)
def case(name):
    """A named, seeded case -> the arguments of ransac_pairs plus `planted` [M] (the rows moved by the
    planted pose) and `planted_pose` [P,4,4]. Shared by the CPU and GPU tests; the arrays are read-only."""
    d = 0.01
    if name == "planted":
        rng = np.random.default_rng(101)
        return _join([_pair(rng, n, d) for n in (200, 317, 64)], n_trials=512, seed=7)
    if name == "weights":
        rng = np.random.default_rng(102)
        c = [_pair(rng, n, d) for n in (150, 90)]
        conf = rng.integers(1, 1025, 240) / 256.0
        conf[::40] = 0.0           # a row of no weight may be an inlier and adds nothing to a score
        return _join(c, conf=conf, seed=11)
    if name == "gated":
        rng = np.random.default_rng(103)
        # pair 0: no fit of three of its rows has a translation below a micrometre; pair 1 passes, though
        # the trials of its outliers fail one gate or the other
        return _join([_pair(rng, 120, d, trans=0.5), _pair(rng, 120, d)], max_trans=np.array([1e-6, 0.5]),
                     max_rot_deg=np.array([np.inf, 60.0]), seed=3)
    if name == "no_normals":
        rng = np.random.default_rng(104)
        return _join([_pair(rng, n, d) for n in (130, 77)], normal_angle_deg=None, seed=5)
    if name == "tiny":
        rng = np.random.default_rng(105)
        return _join([_pair(rng, n, d, share=1.0) for n in (0, 1, 2, 3, 4)], seed=9)
    if name == "degenerate":
        rng = np.random.default_rng(106)
        same = _pair(rng, 50, d, share=1.0)
        same["a"] = np.tile(same["a"][:1], (50, 1))
        same["b"] = np.tile(same["b"][:1], (50, 1))
        line = _pair(rng, 50, d, share=1.0)
        line["a"] = line["a"][:1] + np.linspace(-1, 1, 50)[:, None] * _unit(rng.normal(size=3)) * 0.3
        line["b"] = line["a"] @ line["pose"][:3, :3].T + line["pose"][:3, 3]
        return _join([same, line], normal_angle_deg=None, seed=13)
    if name == "uneven":
        rng = np.random.default_rng(107)
        return _join([_pair(rng, 5, d, share=1.0), _pair(rng, 600, d)], seed=17)
    if name == "duplicated_best":
        rng = np.random.default_rng(108)
        q = _pair(rng, 100, d)
        twice = {k: (np.concatenate([v, v]) if k != "pose" else v) for k, v in q.items()}
        return _join([twice], seed=19)
    if name.startswith("tails_T"):
        rng = np.random.default_rng(109)
        return _join([_pair(rng, n, d) for n in (63, 64, 65, ROW_TILE + 1)], n_trials=int(name[7:]), seed=23)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, route="svd"):
    """The oracle's own run of a case (its hypotheses, their scores, the outcome); computed once."""
    c = case(name)
    h = hypotheses(c, route)
    h["scores"] = trial_scores(c, h["poses"], h["live"])
    h.update(finish(c, h["poses"], h["live"], h["scores"]))
    return h


def well_conditioned(name):
    """[P,T] bool: the oracle's live trials whose sample has sigma_2 / sigma_1 >= 1e-3."""
    h = expected(name)
    return h["live"] & (h["ratio"] >= 1e-3)


def route_gap(name):
    """e0: the largest element-wise difference between the SVD and the quaternion route over the
    well-conditioned trials of a case."""
    keep = well_conditioned(name)
    return float(np.abs(expected(name)["poses"][keep] - expected(name, "horn")["poses"][keep]).max())


def pose_bound(name):
    """The hypothesis tolerance: 16 e0, at least 16 ulp of the case's largest coordinate."""
    c = case(name)
    big = max(np.abs(c["pts_a"]).max(), np.abs(c["pts_b"]).max())
    return max(16 * route_gap(name), 16 * np.spacing(big))
