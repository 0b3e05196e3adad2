"""ORACLE — test infrastructure only. Two numpy restatements of one frame of
NerfRunner.mesh_vertex_color_from_train_images (nerf_runner.py:1446-1458), the checkers of
nof_vertex_color_accumulate and bundlesdf_amd.texture.vertex_colors_from_images:

  brute_frame    every candidate against every vertex, in the kernel's operation order: the point is
                 nof_texture_hits' back-projection (depth2xyzmap in f64 rounded to f32, cam_in_ob in
                 f64), d2 = (dx*dx + dy*dy) + dz*dz in f64, the smallest d2 wins, ties to the lowest
                 pixel index, accepted where sqrt(d2) <= radius. No window: a kernel whose window
                 drops a candidate disagrees with it.
  kdtree_frame   the reference's own lines: cKDTree over the candidate points, one query per
                 vertex, dists <= radius, colour added, count + 1.

Both read the vertices as the C ABI does: float32, widened to float64 (the reference queries the
float64 vertices; the device mesh is float32 throughout, as in nof_raster_faces). The candidates come
from a z-buffer in nof_raster_faces' format: oracle.texture.raster's on the fixture.
"""
import functools

import numpy as np

EMPTY = np.iinfo(np.uint64).max


def candidates(zbuf, H, W, mask, min_depth, cam_in_ob, K):
    """-> (pixel indices ascending [M], points [M,3] f64 in the object frame)."""
    zbuf = np.asarray(zbuf).view(np.uint64).reshape(-1)
    z = (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        ok = (zbuf != EMPTY) & (np.asarray(mask).reshape(-1) != 0) & (z >= np.float32(min_depth))
    idx = np.nonzero(ok)[0]
    z = z[idx]
    py, px = np.divmod(idx, W)
    K = np.asarray(K, np.float64)
    zd = z.astype(np.float64)
    xc = ((px.astype(np.float64) - K[0, 2]) * zd / K[0, 0]).astype(np.float32).astype(np.float64)
    yc = ((py.astype(np.float64) - K[1, 2]) * zd / K[1, 1]).astype(np.float32).astype(np.float64)
    T = np.asarray(cam_in_ob, np.float64)
    pts = np.stack([((T[k, 0] * xc + T[k, 1] * yc) + T[k, 2] * zd) + T[k, 3] for k in range(3)], -1)
    return idx, pts.reshape(-1, 3)


def _vertices(V):
    return np.asarray(V, np.float32).astype(np.float64).reshape(-1, 3)


def brute_frame(V, idx, pts, colors, radius, color_sum, count, chunk=256):
    """In place on color_sum [Nv,3] f64 and count [Nv] i32. -> (nearest [Nv] i32, -1 = none;
    nearest_dist [Nv] f64, inf = none), as the kernel reports them."""
    v = _vertices(V)
    nearest = np.full(len(v), -1, np.int32)
    dist = np.full(len(v), np.inf)
    if len(idx) == 0 or len(v) == 0:
        return nearest, dist
    for a in range(0, len(v), chunk):
        d = pts[None, :, :] - v[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        k = np.argmin(d2, axis=1)                 # first occurrence = lowest pixel index (idx ascends)
        dd = np.sqrt(d2[np.arange(len(k)), k])
        ok = dd <= radius
        rows = a + np.nonzero(ok)[0]
        nearest[rows] = idx[k[ok]]
        dist[rows] = dd[ok]
        color_sum[rows] += np.asarray(colors, np.float32).reshape(-1, 3)[idx[k[ok]]].astype(np.float64)
        count[rows] += 1
    return nearest, dist


def two_nearest(V, pts):
    """-> distances [Nv,2] f64 of every vertex's two nearest candidates (the tie guard)."""
    v = _vertices(V)
    d = pts[None, :, :] - v[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(np.partition(d2, 1, axis=1)[:, :2])


def kdtree_frame(V, idx, pts, colors, radius, color_sum, count):
    """nerf_runner.py:1454-1458. In place; -> (pixel index of every vertex's nearest candidate
    [Nv] (whether accepted or not), its distance [Nv])."""
    from scipy.spatial import cKDTree
    v = _vertices(V)
    if len(idx) == 0 or len(v) == 0:
        return np.full(len(v), -1, np.int64), np.full(len(v), np.inf)
    dists, indices = cKDTree(pts).query(v)
    m = dists <= radius
    color_sum[m] += np.asarray(colors, np.float32).reshape(-1, 3)[idx][indices[m]]
    count[m] += 1
    return idx[indices], dists


def finish(color_sum, count):
    """nerf_runner.py:1460-1462 in f64 (sum / count * 255, clip, uint8 cast); count 0 -> (0, 0, 0), where
    the reference casts NaN to uint8 (undefined)."""
    out = np.zeros((len(count), 3), np.float64)
    seen = count > 0
    out[seen] = np.clip(color_sum[seen] / count[seen].astype(np.float64).reshape(-1, 1) * 255, 0, 255)
    return out.astype(np.uint8)


# ---------------------------------------------------------------- the shared fixture
H, W = 48, 64
K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
MIN_DEPTH, ZFAR = 0.1, 3.0
EYES = ([1.2, 0.3, 0.4], [-0.4, 1.1, -0.3], [0.5, 0.2, 0.45])   # the last one near: min vertex depth 0.35
RADII = (0.01, 0.02, 0.06)


def sphere_mesh():
    """tests/test_gpu_texture.py's _sphere_mesh: the 20^3 marching-cubes sphere, 840 vertices, 1,676 faces."""
    from bundlesdf_amd.mesh import Mesh, marching_cubes
    n = 20
    ax = np.linspace(-0.5, 0.5, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    v, f = marching_cubes(np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.35, 0.0)
    return Mesh(v / (n - 1) - 0.5, f)


@functools.lru_cache(maxsize=None)
def fixture():
    """The mesh, and per camera: cam_in_ob, ob_in_cam, oracle.texture.raster's z-buffer, a mask keeping
    90 % of the pixels, random f32 colours, the candidates. Computed once, never written to."""
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.handoff import GLCAM_IN_CVCAM
    from oracle import texture as TX
    mesh = sphere_mesh()
    rng = np.random.default_rng(0)
    frames = []
    for eye in EYES:
        cam_in_ob = np.ascontiguousarray(SY.look_at(np.asarray(eye, np.float64)) @ GLCAM_IN_CVCAM)
        ob_in_cam = np.ascontiguousarray(np.linalg.inv(cam_in_ob))
        zbuf = TX.raster(mesh.vertices, mesh.faces, ob_in_cam, K, H, W, 0.1, ZFAR)
        mask = (rng.uniform(size=(H, W)) > 0.1).astype(np.uint8)
        colors = rng.uniform(0, 1, (H * W, 3)).astype(np.float32)
        idx, pts = candidates(zbuf, H, W, mask, MIN_DEPTH, cam_in_ob, K)
        fr = dict(cam_in_ob=cam_in_ob, ob_in_cam=ob_in_cam, zbuf=zbuf, mask=mask, colors=colors, idx=idx, pts=pts)
        for a in fr.values():
            a.setflags(write=False)
        frames.append(fr)
    V = mesh.vertices.astype(np.float32)
    V.setflags(write=False)
    return dict(mesh=mesh, V=V, frames=frames)


@functools.lru_cache(maxsize=None)
def fixture_reference(radius):
    """Both restatements over the fixture's three frames at `radius`: per frame (nearest, dist) of
    each, and the final sums, counts and uint8 colours. Computed once per radius."""
    fx = fixture()
    n = len(fx["V"])
    out = {"brute": [], "kdtree": []}
    bs, bc = np.zeros((n, 3)), np.zeros(n, np.int32)
    ks, kc = np.zeros((n, 3)), np.zeros(n, np.int32)
    for fr in fx["frames"]:
        out["brute"].append(brute_frame(fx["V"], fr["idx"], fr["pts"], fr["colors"], radius, bs, bc))
        out["kdtree"].append(kdtree_frame(fx["V"], fr["idx"], fr["pts"], fr["colors"], radius, ks, kc))
    out.update(brute_sum=bs, brute_count=bc, kdtree_sum=ks, kdtree_count=kc,
               brute_rgb=finish(bs, bc), kdtree_rgb=finish(ks, kc))
    for v in (bs, bc, ks, kc, out["brute_rgb"], out["kdtree_rgb"]):
        v.setflags(write=False)
    return out
