"""numpy restatement of what bundlesdf_amd.evaluate must compute, written for the tests: a brute-force
nearest neighbour in the operation order include/nof.h fixes, plain ADD / ADD-S / chamfer the
reference's way (both clouds transformed, nearest neighbour of one in the other), the 17
correspondence sums with math.fsum, and the seeded clouds the CPU and GPU tests share."""
import functools
import math

import numpy as np


def transform(T, pts):
    """((T0 x + T1 y) + T2 z) + T3 per row, every product and sum rounded once (numpy never contracts)."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


def d2_matrix(queries, cloud):
    """[Q,N] f64: (dx dx + dy dy) + dz dz with dx = c_x - q_x."""
    dx = cloud[None, :, 0] - queries[:, None, 0]
    dy = cloud[None, :, 1] - queries[:, None, 1]
    dz = cloud[None, :, 2] - queries[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(queries, cloud, T=None, max_dist=None):
    """(dist [Q] f64, index [Q] i32): argmin takes the lowest index among equal d2."""
    q = np.asarray(queries, np.float64) if T is None else transform(np.asarray(T, np.float64), np.asarray(queries, np.float64))
    d2 = d2_matrix(q, np.asarray(cloud, np.float64))
    idx = np.argmin(d2, 1).astype(np.int32)
    dist = np.sqrt(d2[np.arange(len(q)), idx])
    if max_dist is not None:
        miss = dist > max_dist
        idx[miss] = -1
        dist[miss] = np.inf
    return dist, idx


def top2_gap(queries, cloud, T=None):
    """Per query, second smallest d2 minus smallest: 0 where two cloud points tie for nearest."""
    q = np.asarray(queries, np.float64) if T is None else transform(np.asarray(T, np.float64), np.asarray(queries, np.float64))
    d2 = np.partition(d2_matrix(q, np.asarray(cloud, np.float64)), 1, axis=1)
    return d2[:, 1] - d2[:, 0]


def _homo(T, pts):
    return (T @ np.concatenate([pts, np.ones((len(pts), 1))], 1).T).T[:, :3]


def add(pred, gt, model):
    return float(np.linalg.norm(_homo(pred, model) - _homo(gt, model), axis=1).mean())


def adds(pred, gt, model):
    """Nearest neighbour of every ground-truth-posed point among the predicted-posed points, mean distance."""
    p, g = _homo(pred, model), _homo(gt, model)
    return float(np.sqrt(d2_matrix(g, p).min(1)).mean())


def chamfer(a, b):
    d2 = d2_matrix(np.asarray(a, np.float64), np.asarray(b, np.float64))   # [len(a), len(b)]
    return 0.5 * (float(np.sqrt(d2.min(0)).mean()) + float(np.sqrt(d2.min(1)).mean()))


def moments(source, T, target, index, dist):
    """(sums [17], abs_sums [17]): math.fsum of the terms of the pairs with index >= 0, and of their
    magnitudes (the error bound's scale). Terms are formed as the kernel forms them: p' by `transform`,
    one rounded product per p'_a q_c, dist * dist."""
    p = transform(np.asarray(T, np.float64), source) if T is not None else np.asarray(source, np.float64)
    keep = index >= 0
    p, q, d = p[keep], target[index[keep]], dist[keep]
    cols = [np.ones(len(p))] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)]
    cols += [p[:, a] * q[:, c] for a in range(3) for c in range(3)] + [d * d]
    return (np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols]))


def rigid(rotvec, t):
    """4x4 from an axis-angle vector (Rodrigues) and a translation."""
    r = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(r)
    K = np.zeros((3, 3))
    if th > 0:
        k = r / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def _uniform(seed, n, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def _outside_queries(cloud, seed, n):
    """Queries up to 10 box diagonals outside the cloud's box, on every side."""
    lo, hi = cloud.min(0), cloud.max(0)
    diag = np.linalg.norm(hi - lo)
    c = 0.5 * (lo + hi)
    q = c + np.random.default_rng(seed).uniform(-1, 1, (n, 3)) * (0.5 * (hi - lo) + 10 * diag)
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    corners = c + signs * (0.5 * (hi - lo) + 10 * diag)      # the eight far corners themselves
    faces = np.concatenate([c + np.eye(3)[a] * s * (0.5 * (hi - lo)[a] + 10 * diag) for a in range(3) for s in (-1, 1)]
                           ).reshape(6, 3)
    return np.concatenate([q, corners, faces])


@functools.lru_cache(maxsize=None)
def case(name):
    """A named, seeded search case -> dict(cloud, queries, T ([B,4,4] or None), max_dist, cell, ties).
    Shared by the CPU fairness test and the GPU tests; never modified. `cell` is the PointGrid cell
    (None = default); `ties` marks the one case whose queries have several equally near points."""
    c = dict(T=None, max_dist=None, cell=None, ties=False)
    if name == "one":
        c.update(cloud=_uniform(1, 1), queries=_uniform(2, 1))
    elif name == "n257":
        c.update(cloud=_uniform(3, 257), queries=_uniform(4, 300))
    elif name in ("n3000", "n3000_tiny_cell", "n3000_huge_cell"):
        c.update(cloud=_uniform(0, 3000), queries=_uniform(5, 2500),
                 cell={"n3000": None, "n3000_tiny_cell": 0.02, "n3000_huge_cell": 100.0}[name])
    elif name == "planar":
        cloud = _uniform(6, 1000)
        cloud[:, 1] = 0.375
        c.update(cloud=cloud, queries=_uniform(7, 700))
    elif name == "outside":
        cloud = _uniform(8, 800, -0.3, 0.5)
        c.update(cloud=cloud, queries=_outside_queries(cloud, 9, 600))
    elif name == "duplicates":
        cloud = _uniform(10, 500)
        cloud[np.random.default_rng(11).permutation(500)[:64]] = cloud[17]     # 64 copies of one point (+ itself)
        q = _uniform(12, 300)
        q[:100] = cloud[17] + np.random.default_rng(13).normal(0, 1e-3, (100, 3))   # nearest = the duplicated point
        c.update(cloud=cloud, queries=q, ties=True)
    elif name == "batched":
        rng = np.random.default_rng(14)
        T = np.stack([rigid(rng.normal(0, 0.5, 3), rng.normal(0, 0.2, 3)) for _ in range(5)])
        c.update(cloud=_uniform(15, 1200), queries=_uniform(16, 300), T=T)
    elif name == "max_dist":
        cloud, q = _uniform(17, 1500), _uniform(18, 1000, -1.3, 1.3)
        d, _ = nearest(q, cloud)
        c.update(cloud=cloud, queries=q, max_dist=float(np.median(d)) * (1 + 1e-9))   # about half miss
    else:
        raise KeyError(name)
    return c


CASES = ("one", "n257", "n3000", "n3000_tiny_cell", "n3000_huge_cell", "planar", "outside", "duplicates", "batched",
         "max_dist")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(dist [B,Q] or [Q], index) of a case from the brute force; computed once."""
    c = case(name)
    if c["T"] is None:
        return nearest(c["queries"], c["cloud"], None, c["max_dist"])
    out = [nearest(c["queries"], c["cloud"], T, c["max_dist"]) for T in c["T"]]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
