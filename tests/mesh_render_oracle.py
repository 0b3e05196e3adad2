"""ORACLE — test infrastructure only. The shade step of nof_render_mesh (csrc/mesh_render.hip,
k_mesh_shade) restated in f64 Python floats, operation by operation in the order the kernel's
header comment states, on top of the z-buffer of oracle.texture.raster (which test_gpu_texture.py
holds k_raster to bit for bit). Also the scene and the figures the mesh render tests share.

Per hit pixel (px, py) of face f:
  1. projection and coverage as oracle.texture.raster: e0, e1, e2, zi; depth = f32(zi) (the key's
     high half), face = f
  2. w_k = (e_k / z_k) * zi
  3. n = (w0 n_0 + w1 n_1) + w2 n_2 with vertex normals, else (p1 - p0) x (p2 - p0)
  4. m_r = (R_r0 n_x + R_r1 n_y) + R_r2 n_z; l = sqrt((m_x m_x + m_y m_y) + m_z m_z); l > 0: m / l
  5. d = ((px - cx) / fx, (py - cy) / fy, 1) / sqrt((d_x d_x + d_y d_y) + 1); c = (m . d); c > 0: m = -m
  6. colour: vertex (w0 c_0 + w1 c_1) + w2 c_2; texture: texel(); flat: the base colour
  7. shade: colour * |c|
  8. rint (half to even), clamped to 0 .. 255
"""
import functools
import math

import numpy as np

from oracle import texture as TX

EMPTY = np.iinfo(np.uint64).max
FLAT_RGB = (200, 200, 200)


def project(V, F, f, T, K, znear):
    """oracle.texture.raster's projection of face f: (u, v, z, area), or None where the face is dropped."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    u, v, z = [0.0] * 3, [0.0] * 3, [0.0] * 3
    for k in range(3):
        x, y, w = (float(a) for a in V[F[f, k]])
        X = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * w) + T[0, 3]
        Y = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * w) + T[1, 3]
        Z = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * w) + T[2, 3]
        if not Z > znear:
            return None
        z[k], u[k], v[k] = Z, fx * X / Z + cx, fy * Y / Z + cy
    area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])
    if area == 0.0:
        return None
    return u, v, z, area


def box_pixels(V, F, T, K, H, W, znear):
    """Per face the pixels of its clamped bounding box (0 for a dropped or off-screen face): what
    k_mesh_setup compares with small_max_pixels."""
    V = np.asarray(V, np.float32).astype(np.float64)
    T, K = np.asarray(T, np.float64), np.asarray(K, np.float64)
    out = np.zeros(len(F), np.int64)
    for f in range(len(F)):
        p = project(V, F, f, T, K, znear)
        if p is None:
            continue
        u, v = p[0], p[1]
        u0, u1 = max(0, math.ceil(min(u))), min(W - 1, math.floor(max(u)))
        v0, v1 = max(0, math.ceil(min(v))), min(H - 1, math.floor(max(v)))
        out[f] = max(0, u1 - u0 + 1) * max(0, v1 - v0 + 1)
    return out


def texel(su, sv, TH, TW):
    """(row, column) of uv (su, sv): nearest texel, rows flipped as bake_texture stores its image."""
    col = int(min(max(float(np.rint(su * (TW - 1))), 0.0), TW - 1))
    row = TH - 1 - int(min(max(float(np.rint(sv * (TH - 1))), 0.0), TH - 1))
    return row, col


def shade(keys, V, F, T, K, H, W, znear, mode="flat", shade=False, colors=None, normals=None, uv=None, texture=None,
          base=FLAT_RGB):
    """keys: oracle.texture.raster's z-buffer of the same arguments -> (depth f32 [H,W], face i32 [H,W],
    rgb u8 [H,W,3], normal f32 [H,W,3])."""
    V = np.asarray(V, np.float32).astype(np.float64)
    F = np.asarray(F, np.int64)
    T, K = np.asarray(T, np.float64), np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    depth, face = np.zeros(H * W, np.float32), np.full(H * W, -1, np.int32)
    rgb, normal = np.zeros((H * W, 3), np.uint8), np.zeros((H * W, 3), np.float32)
    if normals is not None:
        normals = np.asarray(normals, np.float32).astype(np.float64)
    if uv is not None:
        uv = np.asarray(uv, np.float32).astype(np.float64)

    def mix(w, a, b, c):
        return (w[0] * a + w[1] * b) + w[2] * c
    for i in np.nonzero(keys != EMPTY)[0]:
        key = int(keys[i])
        f = key & 0xffffffff
        py, px = divmod(int(i), W)
        u, v, z, area = project(V, F, f, T, K, znear)
        X, Y = float(px), float(py)
        e = [((u[2] - u[1]) * (Y - v[1]) - (v[2] - v[1]) * (X - u[1])) / area,
             ((u[0] - u[2]) * (Y - v[2]) - (v[0] - v[2]) * (X - u[2])) / area,
             ((u[1] - u[0]) * (Y - v[0]) - (v[1] - v[0]) * (X - u[0])) / area]
        zi = 1.0 / ((e[0] / z[0] + e[1] / z[1]) + e[2] / z[2])
        depth[i] = np.uint32(key >> 32).view(np.float32)
        assert depth[i] == np.float32(zi)
        face[i] = f
        w = [(e[k] / z[k]) * zi for k in range(3)]
        i0, i1, i2 = (int(a) for a in F[f])
        if normals is not None:
            n = [mix(w, float(normals[i0, k]), float(normals[i1, k]), float(normals[i2, k])) for k in range(3)]
        else:
            a = [float(V[i1, k]) - float(V[i0, k]) for k in range(3)]
            b = [float(V[i2, k]) - float(V[i0, k]) for k in range(3)]
            n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        m = [(float(T[r, 0]) * n[0] + float(T[r, 1]) * n[1]) + float(T[r, 2]) * n[2] for r in range(3)]
        ln = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        if ln > 0.0:
            m = [m[0] / ln, m[1] / ln, m[2] / ln]
        d = [(X - cx) / fx, (Y - cy) / fy, 1.0]
        dl = math.sqrt((d[0] * d[0] + d[1] * d[1]) + 1.0)
        d = [d[0] / dl, d[1] / dl, d[2] / dl]
        cs = (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]
        if cs > 0.0:
            m = [-m[0], -m[1], -m[2]]
        normal[i] = np.array(m, np.float64).astype(np.float32)
        if mode == "vertex":
            col = [mix(w, float(colors[i0, k]), float(colors[i1, k]), float(colors[i2, k])) for k in range(3)]
        elif mode == "texture":
            su = mix(w, float(uv[i0, 0]), float(uv[i1, 0]), float(uv[i2, 0]))
            sv = mix(w, float(uv[i0, 1]), float(uv[i1, 1]), float(uv[i2, 1]))
            r, c = texel(su, sv, texture.shape[0], texture.shape[1])
            col = [float(texture[r, c, k]) for k in range(3)]
        else:
            col = [float(base[k]) for k in range(3)]
        if shade:
            col = [ck * abs(cs) for ck in col]
        rgb[i] = [int(min(max(float(np.rint(ck)), 0.0), 255.0)) for ck in col]
    return depth.reshape(H, W), face.reshape(H, W), rgb.reshape(H, W, 3), normal.reshape(H, W, 3)


def render(mesh, T, K, H, W, znear, zfar, mode="flat", shade_on=False, normals=True, keys=None):
    """The whole oracle for a Mesh: raster (unless `keys` is given) + shade."""
    if keys is None:
        keys = TX.raster(mesh.vertices, mesh.faces, T, K, H, W, znear, zfar)
    return shade(keys, mesh.vertices, mesh.faces, T, K, H, W, znear, mode=mode, shade=shade_on,
                 colors=mesh.vertex_colors, normals=mesh.vertex_normals if normals else None, uv=mesh.uv,
                 texture=mesh.texture)


# ------------------------------------------------------------------ the shared scene
H, W = 48, 64
K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
ZNEAR, ZFAR = 0.1, 3.0


def icosphere(subdivisions=2, radius=0.25):
    """(vertices [V,3] f64, faces [20 * 4^subdivisions, 3]) of a subdivided icosahedron, outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, np.int64)


def _pose(rotvec, t):
    a = np.asarray(rotvec, np.float64)
    ang = np.linalg.norm(a)
    T = np.eye(4)
    if ang > 0:
        k = a / ang
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def scene():
    """The mesh, poses and per-pose oracle z-buffers the mesh render tests share (read-only).

    Mesh (object frame, drawn about 1 m in front of the camera): an icosphere of 320 faces (radius
    0.25) with vertex colours and normals; behind it (0.5 further) a two-face quad of half extent 2,
    far larger than the 64x48 screen at focal length 60; one zero-area face (a repeated corner); one
    face with a corner 0.97 towards the camera (z about 0.03 <= znear at the head-on pose); and at the highest
    index a copy of the sphere face the head-on camera sees at the image centre.
    Poses: head-on; shifted so that part of the sphere leaves the image; shifted 50 to the side
    (everything off-screen)."""
    from bundlesdf_amd.mesh import Mesh
    rng = np.random.default_rng(14)
    sv, sf = icosphere(2, 0.25)
    n_s = len(sv)
    quad = np.array([[-2.0, -2.0, 0.5], [2.0, -2.0, 0.5], [2.0, 2.0, 0.5], [-2.0, 2.0, 0.5]])
    near = np.array([[0.05, 0.05, -0.97], [-0.05, 0.05, -0.5], [0.0, -0.05, -0.5]])
    V = np.concatenate([sv, quad, near]).astype(np.float32).astype(np.float64)
    q, nr = n_s, n_s + 4
    faces = [sf, [[q, q + 1, q + 2], [q, q + 2, q + 3]], [[0, 0, 1]], [[nr, nr + 1, nr + 2]]]
    F = np.concatenate([np.asarray(a, np.int64).reshape(-1, 3) for a in faces])
    poses = np.stack([_pose([0.02, -0.03, 0.01], [0.01, -0.02, 1.0]), _pose([0.3, 0.2, -0.1], [0.35, 0.1, 1.0]),
                      _pose([0.0, 0.1, 0.0], [50.0, 0.0, 1.0])])
    # the duplicate: the sphere face at the image centre of the head-on pose
    z0 = TX.raster(V, F, poses[0], K, H, W, ZNEAR, ZFAR)
    seen = int(z0[(H // 2) * W + W // 2]) & 0xffffffff
    assert seen < len(sf)
    F = np.concatenate([F, F[seen:seen + 1]])
    mesh = Mesh(V, F)
    nrm = rng.normal(size=(len(V), 3))
    nrm[:n_s] = sv
    mesh.vertex_normals = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    mesh.vertex_colors = rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    mesh.uv = rng.uniform(0, 1, (len(V), 2)).astype(np.float32)
    mesh.texture = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    keys = [TX.raster(V, F, T, K, H, W, ZNEAR, ZFAR) for T in poses]
    ids = {"sphere": np.arange(len(sf)), "quad": np.array([len(sf), len(sf) + 1]), "zero_area": len(sf) + 2,
           "near": len(sf) + 3, "duplicate": len(F) - 1, "original": seen}
    for a in (mesh.vertices, mesh.faces, mesh.vertex_normals, mesh.vertex_colors, mesh.uv, mesh.texture, poses, *keys):
        a.setflags(write=False)
    return {"mesh": mesh, "poses": poses, "keys": keys, "ids": ids}


@functools.lru_cache(maxsize=None)
def reference(pose, mode, shade_on, normals=True):
    """(depth, face, rgb, normal) of scene() at pose index `pose`, computed once per argument set."""
    s = scene()
    out = render(s["mesh"], s["poses"][pose], K, H, W, ZNEAR, ZFAR, mode=mode, shade_on=shade_on, normals=normals,
                 keys=s["keys"][pose])
    for a in out:
        a.setflags(write=False)
    return out
