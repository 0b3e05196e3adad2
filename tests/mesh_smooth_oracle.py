"""Plain numpy / Python-loop restatements of the mesh smoothing kernels (csrc/mesh_smooth.hip), in
exactly the operation order include/nof.h states, and the fixtures the smoothing tests share.

numpy float64 scalars follow IEEE arithmetic one operation at a time (no contraction), so a loop here
is the specification the device is compared with bit for bit. The volume is the exception: it is the
exactly rounded sum (math.fsum) of the per-face terms, the yardstick of any summation order."""
import functools
import math

import numpy as np


# ---------------------------------------------------------------- fixtures (built once, never modified)

def _frozen(v, f):
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(None)
def tetrahedron():
    """4 vertices, every degree 3, faces oriented outwards (volume 1/6 of a shifted unit corner)."""
    v = [[0.1, 0.2, 0.3], [1.1, 0.2, 0.3], [0.1, 1.2, 0.3], [0.1, 0.2, 1.3]]
    return _frozen(v, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


@functools.lru_cache(None)
def grid_patch():
    """An open 5 x 4 grid patch, each quad split in two: boundary vertices, degrees 2 to 6. It lies near
    z = -0.5 with its normals towards +z, that is towards the origin's side, so the cones from the origin
    to its faces all count negative: its signed volume is below zero, as an open mesh's may be."""
    nx, ny = 5, 4
    rng = np.random.default_rng(5)
    v = [[i * 0.25, j * 0.3, -0.5 + 0.05 * rng.standard_normal()] for j in range(ny) for i in range(nx)]
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            f += [[a, a + 1, a + nx + 1], [a, a + nx + 1, a + nx]]
    return _frozen(v, f)


@functools.lru_cache(None)
def tetrahedron_plus():
    """The tetrahedron, one isolated vertex (index 4) and the degenerate face (0, 0, 1)."""
    v, f = tetrahedron()
    return _frozen(np.concatenate([v, [[2.0, -1.0, 0.5]]]), np.concatenate([f, [[0, 0, 1]]]))


@functools.lru_cache(None)
def bumpy_sphere():
    """marching_cubes (torch backend) of r - 0.35 - 0.03 sin 9x sin 7y on a 24^3 grid over [-0.5, 0.5]^3,
    in those coordinates: closed, outward oriented, 1,240 vertices, 2,476 faces, degrees 4 to 9."""
    from bundlesdf_amd import mesh as M
    n = 24
    t = np.linspace(-0.5, 0.5, n)
    x, y, z = np.meshgrid(t, t, t, indexing="ij")
    sdf = np.sqrt(x * x + y * y + z * z) - 0.35 - 0.03 * np.sin(9 * x) * np.sin(7 * y)
    v, f = M.marching_cubes(sdf.astype(np.float32), 0.0, backend="torch")
    return _frozen(v / (n - 1) - 0.5, f)


FIXTURES = {"tetrahedron": tetrahedron, "grid_patch": grid_patch, "tetrahedron_plus": tetrahedron_plus,
            "bumpy_sphere": bumpy_sphere}


def bbox_diagonal(v):
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ---------------------------------------------------------------- the restatements

def vertex_adjacency(faces, n_vertices):
    """CSR (row_start [V+1] int32, cols int32): row v = the distinct vertices that share a face edge
    with v, ascending; self-edges dropped."""
    rows = [set() for _ in range(n_vertices)]
    for a, b, c in np.asarray(faces).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                rows[p].add(q)
                rows[q].add(p)
    return _csr([sorted(r) for r in rows])


def vertex_faces(faces, n_vertices):
    """CSR (row_start, face_ids): the faces of v, each once, in ascending face index."""
    rows = [[] for _ in range(n_vertices)]
    for fi, corners in enumerate(np.asarray(faces).tolist()):
        for p in sorted(set(corners)):
            rows[p].append(fi)
    return _csr(rows)


def _csr(rows):
    start = np.zeros(len(rows) + 1, np.int32)
    start[1:] = np.cumsum([len(r) for r in rows])
    return start, np.array([c for r in rows for c in r], np.int32)


def laplacian_step(v, row_start, cols, factor):
    """w = 1.0 / d, m = ((w v[j0] + w v[j1]) + ...) in stored order, out = v + factor (m - v); d == 0 copies."""
    v = np.asarray(v, np.float64)
    out = v.copy()
    factor = np.float64(factor)
    for i in range(len(v)):
        s, e = int(row_start[i]), int(row_start[i + 1])
        if e == s:
            continue
        w = np.float64(1.0) / np.float64(e - s)
        for a in range(3):
            m = w * v[cols[s], a]
            for k in range(s + 1, e):
                m = m + w * v[cols[k], a]
            out[i, a] = v[i, a] + factor * (m - v[i, a])
    return out


def volume_terms(v, faces):
    """Per face (x0 cx + y0 cy) + z0 cz with c = v1 x v2 in the header's component order."""
    t = np.asarray(v, np.float64)[np.asarray(faces, np.int64)]
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = (t[:, k].T for k in range(3))
    cx, cy, cz = y1 * z2 - z1 * y2, z1 * x2 - x1 * z2, x1 * y2 - y1 * x2
    return (x0 * cx + y0 * cy) + z0 * cz


def volume(v, faces):
    """The exactly rounded sum of the terms, over 6."""
    return math.fsum(volume_terms(v, faces).tolist()) / 6.0


def scale_to_volume(v, vol_target, vol_now):
    """(vertices, flag): v cbrt(target / now), or v itself and flag 1 when the ratio is not positive and finite."""
    with np.errstate(all="ignore"):
        r = np.float64(vol_target) / np.float64(vol_now)
    if not (r > 0 and r < np.inf):
        return np.asarray(v, np.float64).copy(), 1
    return np.asarray(v, np.float64) * np.cbrt(r), 0


def vertex_normal_sums(v, faces, face_row_start, face_ids):
    """Per vertex s = 0, then s = s + (v1 - v0) x (v2 - v0) over its faces in stored order."""
    v = np.asarray(v, np.float64)
    faces = np.asarray(faces, np.int64)
    out = np.zeros((len(v), 3))
    for i in range(len(v)):
        sx = sy = sz = np.float64(0.0)
        for k in range(int(face_row_start[i]), int(face_row_start[i + 1])):
            a, b, c = faces[face_ids[k]]
            ux, uy, uz = v[b] - v[a]
            wx, wy, wz = v[c] - v[a]
            sx = sx + (uy * wz - uz * wy)
            sy = sy + (uz * wx - ux * wz)
            sz = sz + (ux * wy - uy * wx)
        out[i] = sx, sy, sz
    return out


def vertex_normals(v, faces, face_row_start, face_ids):
    """sums / sqrt((sx sx + sy sy) + sz sz), one IEEE division per component; (0,0,0) for a zero sum."""
    s = vertex_normal_sums(v, faces, face_row_start, face_ids)
    n = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    ok = n > 0
    return np.where(ok[:, None], s / np.where(ok, n, 1.0)[:, None], 0.0)


def smooth(v, faces, factors, volume_constraint):
    """The filter loop: a step per factor, each followed by the rescale to the initial volume when asked."""
    v = np.asarray(v, np.float64)
    row_start, cols = vertex_adjacency(faces, len(v))
    vol0 = volume(v, faces) if volume_constraint else None
    for factor in factors:
        v = laplacian_step(v, row_start, cols, factor)
        if volume_constraint:
            v, flag = scale_to_volume(v, vol0, volume(v, faces))
            assert flag == 0
    return v


def filter_laplacian(v, faces, lamb=0.5, iterations=10, volume_constraint=True):
    return smooth(v, faces, [lamb] * iterations, volume_constraint)


def filter_taubin(v, faces, lamb=0.5, nu=0.5, iterations=10):
    return smooth(v, faces, [lamb if k % 2 == 0 else -nu for k in range(iterations)], False)
