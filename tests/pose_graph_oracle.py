"""numpy float64 restatement of the pose-graph definition in bundlesdf_amd/csrc/pose_graph.hip's header
comment (include/nof.h group 9), written against that definition: every term of every sum is computed
with the same float64 operations in the same order as the kernels, so a term here and a term there
are the same bits wherever +, -, x, / and sqrt are correctly rounded; only the order in which terms
are added differs. Two routes for the sums and the PCG: float64 (the PCG in the kernel's own order of
additions) and np.longdouble. The seeded cases of the pose-graph tests live here too."""
import math

import numpy as np

EPS = 1e-6                  # FLOAT_EPSILON of the PCG guards
GUARD_BAND = 1e-9           # a choice closer than this to flipping is "guarded" (metres, cosines, pixels, scores)

DEFAULTS = dict(n_outer=7, n_inner=5, robust_delta=0.005, w_sparse=1.0, w_dense=1.0, dist_thresh=0.01,
                normal_thresh=math.cos(math.radians(20.0)), depth_min=0.1, depth_max=9999.0, radius=5,
                max_rot_deg=60.0)


# ----------------------------------------------------------------------------- Lie algebra, transforms
def exp_se3(x):
    """Exp of delta = [omega, v] -> 4x4, in the order of exp_se3 in csrc/pose_graph.hip."""
    wx, wy, wz, vx, vy, vz = (float(v) for v in x)
    th2 = (wx * wx + wy * wy) + wz * wz
    cr = (wy * vz - wz * vy, wz * vx - wx * vz, wx * vy - wy * vx)
    if th2 < 1e-8:
        A, B = 1.0 - th2 / 6.0, 0.5
        t = (vx + 0.5 * cr[0], vy + 0.5 * cr[1], vz + 0.5 * cr[2])
    else:
        if th2 < 1e-6:
            C = (1.0 - th2 / 20.0) / 6.0
            A = 1.0 - th2 * C
            B = 0.5 - th2 / 24.0
        else:
            th = math.sqrt(th2)
            A = math.sin(th) / th
            B = (1.0 - math.cos(th)) / th2
            C = (1.0 - A) / th2
        wc = (wy * cr[2] - wz * cr[1], wz * cr[0] - wx * cr[2], wx * cr[1] - wy * cr[0])
        t = ((vx + B * cr[0]) + C * wc[0], (vy + B * cr[1]) + C * wc[1], (vz + B * cr[2]) + C * wc[2])
    E = np.eye(4)
    E[0] = [1.0 - B * (wy * wy + wz * wz), B * (wx * wy) - A * wz, B * (wx * wz) + A * wy, t[0]]
    E[1] = [B * (wx * wy) + A * wz, 1.0 - B * (wx * wx + wz * wz), B * (wy * wz) - A * wx, t[1]]
    E[2] = [B * (wx * wz) - A * wy, B * (wy * wz) + A * wx, 1.0 - B * (wx * wx + wy * wy), t[2]]
    return E


def apply_update(T, x):
    """Exp(x) T with the kernel's order of additions; the bottom row of T stays."""
    E = exp_se3(x)
    out = T.copy()
    for r in range(3):
        for c in range(4):
            v = (E[r, 0] * T[0, c] + E[r, 1] * T[1, c]) + E[r, 2] * T[2, c]
            out[r, c] = v + E[r, 3] if c == 3 else v
    return out


def xform(T, p):
    """T p for p [n,3] -> [n,3]."""
    return np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], 1)


def rotate(R, v):
    return np.stack([(R[k, 0] * v[:, 0] + R[k, 1] * v[:, 1]) + R[k, 2] * v[:, 2] for k in range(3)], 1)


def huber(e, delta):
    """rho, rho' of the squared residual e."""
    e = np.asarray(e, np.float64)
    out = e > delta * delta
    s = np.sqrt(np.where(out, e, 1.0))
    return np.where(out, (2.0 * s) * delta - delta * delta, e), np.where(out, delta / s, 1.0)


def jac(a):
    """[-[a]x | I] for a [n,3] -> [n,3,6]."""
    n = len(a)
    J = np.zeros((n, 3, 6))
    J[:, 0, 1], J[:, 0, 2] = a[:, 2], -a[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -a[:, 2], a[:, 0]
    J[:, 2, 0], J[:, 2, 1] = a[:, 1], -a[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return J


def _jtj(Ja, Jb):
    """[n,6,6]: dot over the three rows of column r of Ja and column c of Jb, (x0 y0 + x1 y1) + x2 y2."""
    return (Ja[:, 0, :, None] * Jb[:, 0, None, :] + Ja[:, 1, :, None] * Jb[:, 1, None, :]) + Ja[:, 2, :, None] * Jb[:, 2, None, :]


def _jtr(J, r):
    return (J[:, 0, :] * r[:, 0, None] + J[:, 1, :] * r[:, 1, None]) + J[:, 2, :] * r[:, 2, None]


def _param(case, name):
    return case.get(name, DEFAULTS[name])


def min_trace(case):
    m = float(_param(case, "max_rot_deg"))
    return 1.0 + 2.0 * math.cos(math.radians(max(m, 0.0))) if m < 180.0 else -math.inf


# ----------------------------------------------------------------------------- sparse rows
def sparse_rows(case, poses, p):
    """The live rows of sparse pair p at `poses`: dict of i, j, a, b, r, e, w0 (= w_sparse weight), rho, w."""
    i, j = (int(v) for v in case["pair_frames"][p])
    s, t = int(case["pair_start"][p]), int(case["pair_start"][p + 1])
    wt = np.ones(t - s) if case.get("weight") is None else np.asarray(case["weight"][s:t], np.float64)
    live = wt != 0
    a = xform(poses[i], np.asarray(case["pts_a"][s:t], np.float64)[live])
    b = xform(poses[j], np.asarray(case["pts_b"][s:t], np.float64)[live])
    r = a - b
    e = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    rho, drho = huber(e, _param(case, "robust_delta"))
    w0 = _param(case, "w_sparse") * wt[live]
    return dict(i=i, j=j, a=a, b=b, r=r, e=e, w0=w0, rho=rho, w=w0 * drho)


# ----------------------------------------------------------------------------- dense pairs
def valid_mask(case):
    """[N,HW] bool: depth_min < z < depth_max and the normal not all zero."""
    P = np.asarray(case["points"], np.float32).reshape(len(case["points"]), -1, 3)
    Nn = np.asarray(case["normals"], np.float32).reshape(P.shape)
    z = P[..., 2].astype(np.float64)
    return (z > _param(case, "depth_min")) & (z < _param(case, "depth_max")) & ~(Nn == 0).all(-1)


def relative(Ti, Tj):
    """Rij = R_i^T R_j [3,3] and tij = R_i^T (t_j - t_i) [3], in the kernel's order."""
    R = np.empty((3, 3))
    t = np.empty(3)
    d = [Tj[k, 3] - Ti[k, 3] for k in range(3)]
    for r in range(3):
        for c in range(3):
            R[r, c] = (Ti[0, r] * Tj[0, c] + Ti[1, r] * Tj[1, c]) + Ti[2, r] * Tj[2, c]
        t[r] = (Ti[0, r] * d[0] + Ti[1, r] * d[1]) + Ti[2, r] * d[2]
    return R, t


def dense_pairs(case, poses):
    """The active ordered pairs (target i, source j), one per unordered pair, in the order (hi, lo)
    irrelevant to any sum: the source has fewer valid points, the higher index on a tie."""
    cnt = valid_mask(case).sum(1)
    N = len(poses)
    out = []
    for lo in range(N):
        for hi in range(lo + 1, N):
            i = lo if cnt[hi] <= cnt[lo] else hi
            j = hi if i == lo else lo
            R, _ = relative(poses[i], poses[j])
            if (R[0, 0] + R[1, 1]) + R[2, 2] > min_trace(case):
                out.append((i, j))
    return out


def _round_half_away(u):
    t = np.trunc(u)
    return t + np.where(np.abs(u - t) >= 0.5, np.sign(u), 0.0)


def dense_search(case, poses, i, j, want_guard=False):
    """The chosen target pixel of every source pixel of ordered pair (target i, source j): [HW] int32, -1 =
    none; with want_guard also [HW] bool: the choice is within GUARD_BAND of changing."""
    H, W = np.asarray(case["points"]).shape[1:3]
    HW = H * W
    P = np.asarray(case["points"], np.float32).reshape(-1, HW, 3).astype(np.float64)
    Nn = np.asarray(case["normals"], np.float32).reshape(-1, HW, 3).astype(np.float64)
    val = valid_mask(case)
    dmin, dmax, rad = _param(case, "depth_min"), _param(case, "depth_max"), int(_param(case, "radius"))
    dth, nth = _param(case, "dist_thresh"), _param(case, "normal_thresh")
    K = np.asarray(case["K"], np.float64)
    R, t = relative(poses[i], poses[j])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    q, nq = xform(T, P[j]), rotate(R, Nn[j])
    front = q[:, 2] > 0
    qz = np.where(front, q[:, 2], 1.0)
    u, v = (K[0, 0] * q[:, 0]) / qz + K[0, 2], (K[1, 1] * q[:, 1]) / qz + K[1, 2]
    ok = val[j] & front & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    w0, h0 = _round_half_away(u).astype(np.int64), _round_half_away(v).astype(np.int64)
    dh, dw = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")     # row-major scan
    hh, ww = h0[:, None] + dh.reshape(-1)[None], w0[:, None] + dw.reshape(-1)[None]
    inside = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W) & ok[:, None]
    tt = np.where(inside, hh * W + ww, 0)
    pt, nt = P[i][tt], Nn[i][tt]                                   # [HW,win,3]
    dx, dy, dz = pt[..., 0] - q[:, None, 0], pt[..., 1] - q[:, None, 1], pt[..., 2] - q[:, None, 2]
    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
    dn = (nq[:, None, 0] * nt[..., 0] + nq[:, None, 1] * nt[..., 1]) + nq[:, None, 2] * nt[..., 2]
    cand = inside & val[i][tt]
    qual = cand & (dist <= dth) & (dn >= nth)
    score = np.where(qual, (1.0 - dn) + dist / dth, np.inf)
    best = score.argmin(1)                                         # the first of equals
    found = qual.any(1)
    index = np.where(found, tt[np.arange(HW), best], -1).astype(np.int32)
    if not want_guard:
        return index
    g = GUARD_BAND
    zs = P[j][:, 2]
    guard = (np.abs(zs - dmin) < g) | (np.abs(zs - dmax) < g)
    guard |= val[j] & (np.abs(q[:, 2]) < g)
    fu, fv = np.abs(u - np.trunc(u)), np.abs(v - np.trunc(v))
    guard |= ok & ((np.abs(fu - 0.5) < g) | (np.abs(fv - 0.5) < g))
    zt = pt[..., 2]
    guard |= (inside & ((np.abs(zt - dmin) < g) | (np.abs(zt - dmax) < g))).any(1)
    guard |= (cand & ((np.abs(dist - dth) < g) | (np.abs(dn - nth) < g))).any(1)
    srt = np.sort(score, 1)
    if srt.shape[1] > 1:
        with np.errstate(invalid="ignore"):
            guard |= found & (srt[:, 1] - srt[:, 0] < g)
    return index, guard


def dense_rows(case, poses, i, j, index):
    """The rows of ordered pair (i, j) for the correspondences `index` [HW]: dict of u [n,6], d, rho, w."""
    HW = index.shape[0]
    P = np.asarray(case["points"], np.float32).reshape(-1, HW, 3).astype(np.float64)
    Nn = np.asarray(case["normals"], np.float32).reshape(-1, HW, 3).astype(np.float64)
    s = np.flatnonzero(index >= 0)
    t = index[s]
    R, tr = relative(poses[i], poses[j])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, tr
    q = xform(T, P[j][s])
    pt, nt = P[i][t], Nn[i][t]
    dx, dy, dz = pt[:, 0] - q[:, 0], pt[:, 1] - q[:, 1], pt[:, 2] - q[:, 2]
    d = (nt[:, 0] * dx + nt[:, 1] * dy) + nt[:, 2] * dz
    rho, drho = huber(d * d, _param(case, "robust_delta"))
    w = _param(case, "w_dense") * drho
    a, m = xform(poses[j], P[j][s]), rotate(poses[i][:3, :3], nt)
    u = np.stack([a[:, 1] * m[:, 2] - a[:, 2] * m[:, 1], a[:, 2] * m[:, 0] - a[:, 0] * m[:, 2],
                  a[:, 0] * m[:, 1] - a[:, 1] * m[:, 0], m[:, 0], m[:, 1], m[:, 2]], 1)
    return dict(u=u, d=d, rho=_param(case, "w_dense") * rho, w=w)


# ----------------------------------------------------------------------------- the linear system
def _reduce(terms, how):
    """Sum term arrays [n, ...] over n: 'f64' plain numpy, 'ld' np.longdouble, 'fsum' math.fsum."""
    if not terms:
        return None
    t = np.concatenate(terms, 0)
    if how == "fsum":
        flat = t.reshape(len(t), -1)
        return np.array([math.fsum(flat[:, k]) for k in range(flat.shape[1])]).reshape(t.shape[1:])
    if how == "ld":
        return t.astype(np.longdouble).sum(0)
    return t.sum(0)


def linearise(case, poses, dense_index=None, how="f64", bounds=False):
    """A [6N,6N], g [6N] and the history row at `poses` -> dict(A, g, history, dense_index). dense_index
    [N,N,HW] (target, source, pixel; -1 = none) replaces the oracle's own correspondence search, so the
    sums can be taken over the kernel's correspondences. how: the route of the sums. bounds=True adds
    A_abs / g_abs (sum of |term| per entry) and A_n / g_n (terms per entry)."""
    poses = np.asarray(poses, np.float64)
    N = len(poses)
    n = 6 * N
    At = {}         # (bi, bj) -> list of [m,6,6] term arrays
    gt = {}         # bi -> list of [m,6]
    e_sparse = e_dense = []
    e_sparse, e_dense, rows, corr = [], [], 0, 0
    if case.get("pair_frames") is not None:
        for p in range(len(case["pair_frames"])):
            S = sparse_rows(case, poses, p)
            if not len(S["w"]):
                continue
            i, j, w = S["i"], S["j"], S["w"]
            Ja, Jb = jac(S["a"]), jac(S["b"])
            X = w[:, None, None] * _jtj(Ja, Jb)
            At.setdefault((i, i), []).append(w[:, None, None] * _jtj(Ja, Ja))
            At.setdefault((j, j), []).append(w[:, None, None] * _jtj(Jb, Jb))
            At.setdefault((i, j), []).append(-X)
            At.setdefault((j, i), []).append(-X.transpose(0, 2, 1))
            gt.setdefault(i, []).append(-(w[:, None] * _jtr(Ja, S["r"])))
            gt.setdefault(j, []).append(w[:, None] * _jtr(Jb, S["r"]))
            e_sparse.append(S["w0"] * S["rho"])
            rows += len(w)
    out_index = None
    if case.get("points") is not None:
        HW = int(np.prod(np.asarray(case["points"]).shape[1:3]))
        out_index = np.full((N, N, HW), -1, np.int32)
        pairs = dense_pairs(case, poses)
        for (i, j) in pairs:
            idx = dense_search(case, poses, i, j) if dense_index is None else np.asarray(dense_index[i, j])
            out_index[i, j] = idx
            D = dense_rows(case, poses, i, j, idx)
            if not len(D["w"]):
                continue
            wu = D["w"][:, None] * D["u"]
            S = wu[:, :, None] * D["u"][:, None, :]
            S = np.where(np.triu(np.ones((6, 6), bool))[None], S, S.transpose(0, 2, 1))     # (w u_r) u_c, r <= c, mirrored
            h = wu * D["d"][:, None]
            At.setdefault((i, i), []).append(S)
            At.setdefault((j, j), []).append(S)
            At.setdefault((i, j), []).append(-S)
            At.setdefault((j, i), []).append(-S)
            gt.setdefault(i, []).append(-h)
            gt.setdefault(j, []).append(h)
            e_dense.append(D["rho"])
            corr += len(D["w"])
    dt = np.longdouble if how == "ld" else np.float64
    A, g = np.zeros((n, n), dt), np.zeros(n, dt)
    out = dict(dense_index=out_index)
    if bounds:
        out.update(A_abs=np.zeros((n, n)), g_abs=np.zeros(n), A_n=np.zeros((n, n), np.int64), g_n=np.zeros(n, np.int64))
    fixed = np.asarray(case["fixed"], bool)
    for (bi, bj), terms in At.items():
        if fixed[bi] or fixed[bj]:
            continue
        A[6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6] = _reduce(terms, how)
        if bounds:
            out["A_abs"][6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6] = _reduce([np.abs(t) for t in terms], "fsum")
            out["A_n"][6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6] = sum(len(t) for t in terms)
    for bi, terms in gt.items():
        if fixed[bi]:
            continue
        g[6 * bi:6 * bi + 6] = _reduce(terms, how)
        if bounds:
            out["g_abs"][6 * bi:6 * bi + 6] = _reduce([np.abs(t) for t in terms], "fsum")
            out["g_n"][6 * bi:6 * bi + 6] = sum(len(t) for t in terms)
    es = _reduce([e[:, None] for e in e_sparse], how)
    ed = _reduce([e[:, None] for e in e_dense], how)
    out.update(A=A, g=g, history=np.array([0.0 if es is None else float(es[0]), 0.0 if ed is None else float(ed[0]),
                                           float(rows), float(corr)]))
    return out


# ----------------------------------------------------------------------------- PCG
_LANE = np.arange(64)


def _dot(a, b):
    """The kernel's dot product in float64: thread t of 256 adds rows t, t + 256, ... in order, a
    butterfly adds the 64 lanes of a wave, the four waves are added in order."""
    prod = a * b
    k = -(-len(prod) // 256)
    pad = np.zeros(k * 256)
    pad[:len(prod)] = prod
    acc = np.zeros(256)
    for row in pad.reshape(k, 256):
        acc = acc + row
    acc = acc.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _LANE ^ o]
    return ((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0]


def pcg(A, g, n_inner, dtype=np.float64):
    """n_inner steps of Jacobi-preconditioned CG on A x = g from x = 0, with the guards of the
    definition. dtype float64: the kernel's own order of every addition; np.longdouble: the second route."""
    ld = dtype is np.longdouble
    A, g = np.asarray(A, dtype), np.asarray(g, dtype)
    n = len(g)
    dot = (lambda a, b: (a * b).sum()) if ld else _dot
    dg = np.diagonal(A)
    Mi = np.where(dg > EPS, 1.0 / np.where(dg > EPS, dg, 1.0), 1.0).astype(dtype)
    x, r = np.zeros(n, dtype), g.copy()
    z = Mi * r
    p = z.copy()
    rz = dot(r, z)
    for _ in range(n_inner):
        if ld:
            Ap = A.T @ p
        else:
            Ap = np.zeros(n)
            for c in range(n):
                Ap = Ap + A[c] * p[c]                   # row r: columns in ascending order, A read as its transpose
        pAp = dot(p, Ap)
        alpha = rz / pAp if pAp > EPS else dtype(0.0)
        x = x + alpha * p
        r = r - alpha * Ap
        z = Mi * r
        rz_new = dot(z, r)
        beta = rz_new / rz if rz > EPS else dtype(0.0)
        p = z + beta * p
        rz = rz_new
    return x


def pcg_gap(A, g, n_inner):
    """The oracle's own gap on one system: max |float64 route - long-double route| of the PCG result."""
    return float(np.abs(pcg(A, g, n_inner).astype(np.longdouble) - pcg(A, g, n_inner, np.longdouble)).max())


# ----------------------------------------------------------------------------- the whole optimisation
def optimise(case, how="f64"):
    """The definition end to end -> dict(poses, history [n_outer+1,4], iter_poses, delta)."""
    poses = np.array(case["poses"], np.float64)
    fixed = np.asarray(case["fixed"], bool)
    n_outer, n_inner = int(_param(case, "n_outer")), int(_param(case, "n_inner"))
    hist, iters, deltas = [], [poses.copy()], []
    for _ in range(n_outer):
        L = linearise(case, poses, how=how)
        hist.append(L["history"])
        x = pcg(L["A"], L["g"], n_inner, np.longdouble if how == "ld" else np.float64)
        x = np.asarray(x, np.float64)                   # the update itself is float64 on both routes
        deltas.append(x)
        poses = np.stack([poses[k] if fixed[k] else apply_update(poses[k], x[6 * k:6 * k + 6]) for k in range(len(poses))])
        iters.append(poses.copy())
    hist.append(linearise(case, poses, how=how)["history"])
    return dict(poses=poses, history=np.stack(hist), iter_poses=np.stack(iters), delta=np.stack(deltas))


def route_gap(case):
    """The oracle's own gap on a whole case: max |float64 route - long-double route| over the final poses."""
    return float(np.abs(optimise(case)["poses"] - optimise(case, "ld")["poses"]).max())


def pose_error(poses, truth):
    """Each frame's worst entry of poses against truth, averaged over the frames (a frame that nothing
    touches keeps its error, so the worst frame alone would hide what the others gain)."""
    return float(np.abs(np.asarray(poses) - np.asarray(truth)).max((1, 2)).mean())


# ----------------------------------------------------------------------------- seeded cases
def rigid(rotvec, trans):
    T = exp_se3([rotvec[0], rotvec[1], rotvec[2], 0.0, 0.0, 0.0])
    T[:3, 3] = trans
    return T


def inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def look_at(eye, target=(0.0, 0.0, 0.03), up=(0.0, 0.0, 1.0)):
    """Camera-in-world pose of a camera at `eye` looking at `target` (x right, y down, z forward)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


SPHERES = (((0.0, 0.0, 0.04), 0.05), ((0.075, 0.03, 0.025), 0.03))      # on the plane z = 0, a disc of radius 0.2
DISC = 0.2


def render_maps(T, K, H, W):
    """Exact camera-space point and normal maps [H,W,3] float32 of two spheres on a disc seen from pose T
    (camera-in-world); a pixel that sees nothing has a zero point and a zero normal."""
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1).reshape(-1, 3)
    o, dw = T[:3, 3], d @ T[:3, :3].T
    best = np.full(len(d), np.inf)
    nrm = np.zeros((len(d), 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = -o[2] / dw[:, 2]
    hit = o + tp[:, None] * dw
    okp = (tp > 0) & np.isfinite(tp) & (np.hypot(hit[:, 0], hit[:, 1]) < DISC)
    best[okp] = tp[okp]
    nrm[okp] = (0.0, 0.0, 1.0)
    for c, r in SPHERES:
        oc = o - np.asarray(c)
        a, b, cc = (dw * dw).sum(1), 2.0 * (dw @ oc), oc @ oc - r * r
        disc = b * b - 4.0 * a * cc
        with np.errstate(invalid="ignore"):
            ts = (-b - np.sqrt(disc)) / (2.0 * a)
        oks = (disc > 0) & (ts > 0) & (ts < best)
        best[oks] = ts[oks]
        nrm[oks] = ((o + ts[:, None] * dw - np.asarray(c)) / r)[oks]
    seen = np.isfinite(best)
    pts = np.where(seen[:, None], np.where(seen, best, 0.0)[:, None] * d, 0.0)
    ncam = np.where(seen[:, None], nrm @ T[:3, :3], 0.0)            # R^T n
    return pts.reshape(H, W, 3).astype(np.float32), ncam.reshape(H, W, 3).astype(np.float32)


def _ring_poses(N, rng, spread=0.35):
    """N cameras about 0.25 m from the scene, on an arc above it."""
    out = []
    for k in range(N):
        az = -0.5 * spread * (N - 1) + spread * k + rng.normal(0, 0.02)
        el = 0.9 + rng.normal(0, 0.03)
        rad = 0.25 + rng.normal(0, 0.005)
        out.append(look_at((rad * math.cos(el) * math.cos(az), rad * math.cos(el) * math.sin(az), rad * math.sin(el) + 0.03)))
    return np.stack(out)


def _perturb(truth, fixed, rng, rot, trans):
    out = truth.copy()
    for k in range(len(truth)):
        if not fixed[k]:
            out[k] = apply_update(truth[k], np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))
    return out


def sparse_case(seed=0, N=4, counts=(0, 1, 65, 600, 40, 130), zero_weights=True, fixed=None, lonely=None,
                rot=0.03, trans=0.003, **params):
    """Planted sparse-only case: world points seen from N true poses, pairs with `counts` rows each over
    a cycle of frame pairs, exact matches; the initial poses are the truth perturbed by rot rad / trans m
    (normal sigma) on the free frames. lonely: a free frame that no pair touches."""
    rng = np.random.default_rng(seed)
    truth = _ring_poses(N, rng)
    fx = np.zeros(N, bool)
    if fixed is None:
        fx[0] = True
    else:
        fx[:] = fixed
    frames = [k for k in range(N) if k != lonely]
    cand = [(frames[x], frames[y]) for x in range(len(frames)) for y in range(len(frames)) if x != y]
    pf, a, b, ps = [], [], [], [0]
    for p, cnt in enumerate(counts):
        i, j = cand[(p * 5 + 1) % len(cand)] if len(cand) > 2 else cand[p % len(cand)]
        X = rng.uniform(-0.08, 0.08, (cnt, 3)) + (0.0, 0.0, 0.04)
        pf.append((i, j))
        a.append(xform(inverse(truth[i]), X))
        b.append(xform(inverse(truth[j]), X))
        ps.append(ps[-1] + cnt)
    M = ps[-1]
    weight = None
    if zero_weights:
        weight = rng.uniform(0.5, 1.5, M)
        weight[rng.uniform(size=M) < 0.2] = 0.0
    case = dict(poses=_perturb(truth, fx, rng, rot, trans), truth=truth, fixed=fx,
                pair_frames=np.array(pf, np.int32), pts_a=np.concatenate(a), pts_b=np.concatenate(b),
                pair_start=np.array(ps, np.int32), weight=weight)
    case.update(params)
    return case


def dense_case(seed=0, N=4, H=24, W=32, radius=5, rot=0.012, trans=0.0015, with_sparse=False, far_frame=False,
               tie=False, **params):
    """Planted dense case: exact maps of the two-sphere scene from N true poses. A patch of normals of
    frame 1 is zeroed (invalid normals with a valid depth); far_frame turns the last camera to the far
    side of the scene, beyond max_rot_deg of every other; tie gives frames 0 and 1 the same number of
    valid points. with_sparse adds matches of scene points between neighbouring frames."""
    rng = np.random.default_rng(100 + seed)
    truth = _ring_poses(N, rng, spread=0.22)
    if far_frame:
        truth[-1] = look_at((-0.2, 0.02, 0.12))
    K = np.array([[40.0, 0.0, W / 2 - 0.3], [0.0, 40.0, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    maps = [render_maps(T, K, H, W) for T in truth]
    points, normals = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    normals[min(1, N - 1), 3:6, 4:9] = 0.0
    case = dict(truth=truth, K=K, radius=radius)
    case.update(params)
    if tie:
        c = dict(points=points, normals=normals, **{k: v for k, v in case.items() if k in DEFAULTS})
        cnt = valid_mask(c).sum(1)
        more, less = (0, 1) if cnt[0] > cnt[1] else (1, 0)
        ids = np.flatnonzero(valid_mask(c)[more])[:abs(int(cnt[0]) - int(cnt[1]))]
        normals[more].reshape(-1, 3)[ids] = 0.0
    fx = np.zeros(N, bool)
    fx[0] = True
    case.update(poses=_perturb(truth, fx, rng, rot, trans), fixed=fx, points=points, normals=normals)
    if with_sparse:
        pf, a, b, ps = [], [], [], [0]
        for i in range(N - 1):
            X = rng.uniform(-0.06, 0.06, (30, 3)) + (0.0, 0.0, 0.04)
            pf.append((i, i + 1))
            a.append(xform(inverse(truth[i]), X))
            b.append(xform(inverse(truth[i + 1]), X))
            ps.append(ps[-1] + 30)
        case.update(pair_frames=np.array(pf, np.int32), pts_a=np.concatenate(a), pts_b=np.concatenate(b),
                    pair_start=np.array(ps, np.int32), weight=None)
    return case


def guarded_share(case, poses=None):
    """Guarded source pixels over valid source pixels, across the active pairs at `poses`."""
    poses = np.asarray(case["poses"] if poses is None else poses, np.float64)
    val = valid_mask(case)
    guarded = total = 0
    for (i, j) in dense_pairs(case, poses):
        _, gd = dense_search(case, poses, i, j, want_guard=True)
        guarded += int((gd & val[j]).sum())
        total += int(val[j].sum())
    return guarded / max(total, 1), total
