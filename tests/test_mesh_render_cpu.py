"""CPU: the mesh render's host side. The oracle of tests/mesh_render_oracle.py against closed forms,
the C ABI's exports and refusals (validated before any HIP call, so they run without a GPU),
Mesh.export -> Mesh.load round trips, and evaluate.mesh_frame_agreement on hand-made frames."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mesh_render_oracle as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle against closed forms
def _mesh(V, F):
    from bundlesdf_amd.mesh import Mesh
    return Mesh(np.asarray(V, np.float64), np.asarray(F, np.int64))


def test_fronto_parallel_quad_renders_its_depth_exactly():
    z = 0.75                                     # exactly representable, as are the corners
    m = _mesh([[-0.25, -0.125, z], [0.25, -0.125, z], [0.25, 0.125, z], [-0.25, 0.125, z]], [[0, 1, 2], [0, 2, 3]])
    depth, face, rgb, normal = MR.render(m, np.eye(4), MR.K, MR.H, MR.W, 0.1, 2.0)
    hit = face >= 0
    # the quad spans u = 31.5 +- 20, v = 23.5 +- 10: pixel centres 12..51 x 14..33
    want = np.zeros((MR.H, MR.W), bool)
    want[14:34, 12:52] = True
    assert np.array_equal(hit, want)
    assert (depth[hit] == np.float32(z)).all() and (depth[~hit] == 0).all()
    assert (rgb[hit] == 200).all() and (rgb[~hit] == 0).all()
    # the face normal is +-z; it is flipped towards the camera
    assert np.array_equal(normal[hit], np.tile(np.array([0, 0, -1], np.float32), (hit.sum(), 1)))
    assert (normal[~hit] == 0).all()


def test_rgb_triangle_gives_the_analytic_colour():
    # fx = 64, cx = 32, Z = 1: corners project to pixels (8, 8), (40, 8), (8, 40) exactly
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1]])
    px = np.array([[8, 8], [40, 8], [8, 40]], np.float64)
    V = np.concatenate([(px - [32.0, 24.0]) / 64.0, np.ones((3, 1))], 1)
    m = _mesh(V, [[0, 1, 2]])
    m.vertex_colors = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    depth, face, rgb, _ = MR.render(m, np.eye(4), K, 48, 64, 0.1, 2.0, mode="vertex")
    for x, y in [(8, 8), (40, 8), (8, 40), (16, 16), (24, 8), (9, 8), (20, 25), (24, 24)]:
        b1, b2 = (x - 8) / 32.0, (y - 8) / 32.0          # barycentrics of corners 1 and 2: exact in f64
        want = np.rint(np.array([1.0 - b1 - b2, b1, b2]) * 255.0)   # half to even: 127.5 -> 128
        assert face[y, x] == 0 and depth[y, x] == 1.0
        assert np.array_equal(rgb[y, x], want.astype(np.uint8)), (x, y)
    assert np.array_equal(rgb[8, 24], [128, 128, 0])
    assert face[8, 41] == -1 and face[25, 24] == -1      # just outside the right edge and the hypotenuse
    # the headlight: on the optical axis' pixel row the factor is |n . d| = 1 / |d|
    _, _, lit, _ = MR.render(m, np.eye(4), K, 48, 64, 0.1, 2.0, mode="vertex", shade_on=True)
    d = np.array([(16 - 32.0) / 64.0, (16 - 24.0) / 64.0, 1.0])
    want = np.rint(np.array([0.5, 0.25, 0.25]) * 255.0 * (1.0 / np.linalg.norm(d)))
    assert np.abs(lit[16, 16].astype(int) - want).max() <= 1 and (lit[16, 16] < rgb[16, 16]).all()


def test_texture_rows_and_columns_of_the_corner_uvs():
    TH, TW = 5, 7
    assert MR.texel(0.0, 0.0, TH, TW) == (TH - 1, 0)
    assert MR.texel(1.0, 0.0, TH, TW) == (TH - 1, TW - 1)
    assert MR.texel(0.0, 1.0, TH, TW) == (0, 0)
    assert MR.texel(1.0, 1.0, TH, TW) == (0, TW - 1)
    assert MR.texel(0.25, 0.5, TH, TW) == (2, 2)         # rint(1.5) = 2 (half to even), row 4 - 2
    # through the render: a triangle whose three corners share one uv shows that texel everywhere
    rng = np.random.default_rng(0)
    tex = rng.integers(0, 256, (TH, TW, 3)).astype(np.uint8)
    for uv, (r, c) in (((0, 0), (TH - 1, 0)), ((1, 0), (TH - 1, TW - 1)), ((0, 1), (0, 0)), ((1, 1), (0, TW - 1))):
        m = _mesh([[-0.2, -0.2, 1.0], [0.2, -0.2, 1.0], [0.0, 0.2, 1.0]], [[0, 1, 2]])
        m.uv, m.texture = np.tile(np.array(uv, np.float64), (3, 1)), tex
        _, face, rgb, _ = MR.render(m, np.eye(4), MR.K, MR.H, MR.W, 0.1, 2.0, mode="texture")
        assert (face >= 0).sum() > 100 and (rgb[face >= 0] == tex[r, c]).all()


def test_shared_scene_is_not_vacuous():
    s = MR.scene()
    ids = s["ids"]
    assert len(ids["sphere"]) == 320
    face0 = MR.reference(0, "flat", False)[1]
    assert (face0 >= 0).sum() > 300
    assert ids["duplicate"] not in face0 and ids["original"] in face0
    assert MR.box_pixels(s["mesh"].vertices, s["mesh"].faces, s["poses"][0], MR.K, MR.H, MR.W, MR.ZNEAR)[
        [ids["zero_area"], ids["near"]]].tolist() == [0, 0]
    assert (MR.reference(2, "flat", False)[1] == -1).all()


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def libnof():
    from bundlesdf_amd import build
    build.build()
    from bundlesdf_amd import _lib
    return _lib.lib()


def test_symbols_exported_and_bound(libnof):
    from bundlesdf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nof.h")).read()
    for name in ("nof_render_mesh", "nof_render_mesh_workspace_bytes"):
        assert name + "(" in header and name in _lib.declared_symbols() and hasattr(libnof, name)
    assert libnof.nof_render_mesh_workspace_bytes(2, 10, 4, 8) >= (2 * 4 * 8 + 2 * 10) * 8


def _valid_desc(buf, K):
    """A descriptor nof_render_mesh would accept. Its device pointers name a host buffer: the tests
    below break one field each and the call returns before anything is dereferenced."""
    from bundlesdf_amd import _lib
    d = _lib.MeshRenderDesc()
    p = buf.ctypes.data
    for name in ("vertices", "faces", "colors", "normals", "uv", "texture", "ob_in_cam", "workspace", "depth", "face",
                 "rgb", "normal"):
        setattr(d, name, p)
    d.K = K.ctypes.data
    d.n_vertices, d.n_faces, d.tex_h, d.tex_w = 3, 1, 4, 4
    d.B, d.H, d.W, d.znear, d.zfar = 1, 4, 4, 0.1, 2.0
    d.colour_mode, d.small_max_pixels = _lib.MESH_COLOUR_FLAT, 256
    return d


_REFUSALS = [
    ("vertices", dict(vertices=None), b"vertices is NULL"), ("faces", dict(faces=None), b"faces is NULL"),
    ("ob_in_cam", dict(ob_in_cam=None), b"ob_in_cam is NULL"), ("K", dict(K=None), b"K is NULL"),
    ("workspace", dict(workspace=None), b"workspace is NULL"), ("depth", dict(depth=None), b"depth is NULL"),
    ("face", dict(face=None), b"face is NULL"), ("rgb", dict(rgb=None), b"rgb is NULL"),
    ("normal", dict(normal=None), b"normal is NULL"),
    ("B0", dict(B=0), b"B=0"), ("H0", dict(H=0), b"H=0"), ("W0", dict(W=-1), b"W=-1"),
    ("BHW", dict(B=1 << 11, H=1 << 10, W=1 << 10), b"B*H*W=2147483648"),
    ("znear0", dict(znear=0.0), b"znear=0"), ("znear_neg", dict(znear=-1.0), b"znear=-1"),
    ("znear_nan", dict(znear=float("nan")), b"znear"),
    ("zfar", dict(zfar=0.1), b"zfar=0.1"), ("zfar_below", dict(zfar=0.05), b"zfar"),
    ("texture_no_uv", dict(colour_mode=2, uv=None), b"needs uv"),
    ("texture_no_texture", dict(colour_mode=2, texture=None), b"needs texture"),
    ("vertex_no_colors", dict(colour_mode=1, colors=None), b"needs colors"),
    ("mode", dict(colour_mode=7), b"colour_mode=7"),
    ("small_max_pixels", dict(small_max_pixels=-1), b"small_max_pixels=-1"),
    ("n_faces", dict(n_faces=-1), b"n_faces=-1"),
]


@pytest.mark.parametrize("name,change,message", _REFUSALS, ids=[r[0] for r in _REFUSALS])
def test_bad_descriptors_are_refused_before_device_work(libnof, name, change, message):
    buf, K = np.zeros(64, np.float64), np.ascontiguousarray(MR.K)
    d = _valid_desc(buf, K)
    for k, v in change.items():
        setattr(d, k, v)
    assert libnof.nof_render_mesh(ctypes.byref(d), None) == 1        # NOF_EINVAL
    err = libnof.nof_last_error()
    assert err.startswith(b"render_mesh: ") and message in err, err


def test_null_descriptor_is_refused(libnof):
    assert libnof.nof_render_mesh(None, None) == 1
    assert b"desc is NULL" in libnof.nof_last_error()


# ------------------------------------------------------------------ Mesh.load
def _tetra():
    m = _mesh([[0, 0, 0], [1.5, 0, 0], [0, -2.25, 0], [0.125, 0.5, 3.0]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    return m


def _same_geometry(a, b):
    assert np.allclose(a.vertices, b.vertices, atol=5e-7, rtol=0) and np.array_equal(a.faces, b.faces)


def test_load_round_trip_plain(tmp_path):
    from bundlesdf_amd.mesh import Mesh
    m = _tetra()
    m.export(str(tmp_path / "m.obj"))
    r = Mesh.load(str(tmp_path / "m.obj"))
    _same_geometry(m, r)
    assert r.vertex_colors is None and r.vertex_normals is None and r.uv is None and r.texture is None
    assert r.vertices.dtype == np.float64 and r.faces.dtype == np.int64


def test_load_round_trip_vertex_colours(tmp_path):
    from bundlesdf_amd.mesh import Mesh
    m = _tetra()
    m.vertex_colors = np.array([[0, 1, 2], [255, 254, 127], [128, 129, 64], [33, 200, 17]], np.uint8)
    m.export(str(tmp_path / "m.obj"))
    r = Mesh.load(str(tmp_path / "m.obj"))
    _same_geometry(m, r)
    assert r.vertex_colors.dtype == np.uint8 and np.array_equal(r.vertex_colors, m.vertex_colors)


def test_load_round_trip_normals(tmp_path):
    from bundlesdf_amd.mesh import Mesh
    m = _tetra()
    n = np.array([[1, 2, 3], [-1, 0, 0], [0, 0.5, 0.5], [3, -1, 2]], np.float64)
    m.vertex_normals = n / np.linalg.norm(n, axis=1, keepdims=True)
    m.vertex_colors = np.full((4, 3), 9, np.uint8)
    m.export(str(tmp_path / "m.obj"))
    r = Mesh.load(str(tmp_path / "m.obj"))
    _same_geometry(m, r)
    assert np.allclose(r.vertex_normals, m.vertex_normals, atol=5e-7, rtol=0)
    assert np.array_equal(r.vertex_colors, m.vertex_colors)


@pytest.mark.parametrize("normals", [False, True])
def test_load_round_trip_textured(tmp_path, normals):
    from bundlesdf_amd.mesh import Mesh
    m = _tetra()
    m.uv = np.array([[0, 0], [1, 0], [0.25, 0.75], [0.5, 1]], np.float64)
    m.texture = np.random.default_rng(1).integers(0, 256, (6, 5, 3)).astype(np.uint8)
    if normals:
        m.vertex_normals = np.tile(np.array([0.0, 0.0, 1.0]), (4, 1))
    m.export(str(tmp_path / "t.obj"))
    r = Mesh.load(str(tmp_path / "t.obj"))
    _same_geometry(m, r)
    assert np.allclose(r.uv, m.uv, atol=5e-7, rtol=0)
    assert r.texture.dtype == np.uint8 and np.array_equal(r.texture, m.texture)
    assert (r.vertex_normals is not None) == normals


@pytest.mark.parametrize("line,why", [("vp 0.1 0.2", "unsupported"), ("v 1 2", "expected"), ("v 1 2 x", "not a number"),
                                      ("f 1 2 3 4", "three corners"), ("f 1/2 2/2 3/3", "corner"),
                                      ("f 0 1 2", "corner"), ("g group", "unsupported"), ("vt 0.5", "expected")])
def test_load_names_the_malformed_line(tmp_path, line, why):
    from bundlesdf_amd.mesh import Mesh
    p = tmp_path / "bad.obj"
    p.write_text("# a comment\nv 0 0 0\nv 1 0 0\nv 0 1 0\n" + line + "\nf 1 2 3\n")
    with pytest.raises(ValueError) as e:
        Mesh.load(str(p))
    msg = str(e.value)
    assert f"{p}:5:" in msg and why in msg and line in msg


def test_load_refuses_a_face_past_the_vertices(tmp_path):
    from bundlesdf_amd.mesh import Mesh
    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="vertex 4 of 3"):
        Mesh.load(str(p))


def test_read_png_undoes_every_row_filter(tmp_path):
    """write_png only writes filter 0; a file with the other four row filters decodes to the same image."""
    import struct
    import zlib
    from bundlesdf_amd.mesh import read_png
    img = np.random.default_rng(2).integers(0, 256, (5, 4, 3)).astype(np.uint8)
    flat = img.reshape(5, 12).astype(int)
    rows = []
    for r, ft in enumerate([0, 1, 2, 3, 4]):
        up = flat[r - 1] if r else np.zeros(12, int)
        enc = []
        for x in range(12):
            a = flat[r, x - 3] if x >= 3 else 0
            b, c = up[x], (up[x - 3] if x >= 3 else 0)
            p = a + b - c
            paeth = min((abs(p - a), 0, a), (abs(p - b), 1, b), (abs(p - c), 2, c))[2]
            pred = [0, a, b, (a + b) // 2, paeth][ft]
            enc.append((flat[r, x] - pred) & 255)
        rows.append(bytes([ft]) + bytes(enc))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    path = tmp_path / "f.png"
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 5, 8, 2, 0, 0, 0))
                     + chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b""))
    assert np.array_equal(read_png(str(path)), img)


# ------------------------------------------------------------------ mesh_frame_agreement
def test_mesh_frame_agreement_by_hand():
    from bundlesdf_amd.evaluate import mesh_frame_agreement
    # frame 0, 2x4. rendered valid: 5 pixels (one masked pixel has depth 0, one lies beyond max_depth);
    # observed valid: 5 pixels; both: 4 pixels with |diff| 0.5, 0.25, 0, 1.0; union 6
    rd0 = np.array([[1.0, 2.0, 3.0, 0.0], [1.5, 4.0, 9.0, 0.0]])
    rm0 = np.array([[1, 1, 1, 1], [1, 1, 1, 0]])
    od0 = np.array([[1.5, 2.25, 3.0, 1.0], [0.0, 5.0, 2.0, 99.0]])
    om0 = np.array([[1, 1, 1, 1], [1, 1, 0, 1]])
    # frame 1: the valid sets do not meet
    rd1 = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    rm1 = rd1 > 0
    od1 = np.array([[0.0, 0.0, 2.0, 2.0], [99.0, 0.0, 0.0, 0.0]])
    om1 = np.ones((2, 4))
    # frame 2: nothing valid anywhere
    z = np.zeros((2, 4))
    r = mesh_frame_agreement(torch.tensor(np.stack([rd0, rd1, z]), dtype=torch.float32),
                             torch.tensor(np.stack([rm0, rm1, z])) != 0,
                             np.stack([od0, od1, z]), np.stack([om0, om1, z]), max_depth=5.0)
    assert r["count"].tolist() == [4, 0, 0]
    assert r["iou"].tolist() == [4 / 6, 0.0, 0.0]
    assert r["depth_mean"].tolist() == [(0.5 + 0.25 + 0.0 + 1.0) / 4, 0.0, 0.0]
    assert r["depth_median"].tolist() == [0.25, 0.0, 0.0]      # the lower middle of 0, 0.25, 0.5, 1
    assert all(torch.isfinite(v.double()).all() for v in r.values())
    # a single [H,W] frame, odd count: the middle value
    od = od0.copy()
    od[1, 1] = 0.0
    one = mesh_frame_agreement(rd0, rm0, od, om0, 5.0)
    assert one["count"].tolist() == [3] and one["depth_median"].tolist() == [0.25] and one["iou"].tolist() == [3 / 6]
