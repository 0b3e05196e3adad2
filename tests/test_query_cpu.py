"""CPU: the field point query's host side — the query oracle checked against finite differences,
nof_query_field's argument validation (before any device work), Mesh vertex attributes through
copy / weld / mask / transform / export, and the gating of NerfRunner._hook_mesh."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import query_oracle as QO


@pytest.fixture(scope="module")
def libnof():
    from bundlesdf_amd import build
    build.build()
    from bundlesdf_amd import _lib
    return _lib.lib()


def test_oracle_normal_is_the_finite_difference_of_its_sdf():
    """Two dense levels (base_res 4, finest 8), a random NeRFSmall, fp32. Inside one cell of every level
    and one ReLU region the SDF is trilinear, so along an axis it is linear and the central difference
    quotient over +-h is exact up to the fp32 rounding of the two SDF values: eps_fp32 |sdf| / h (half an
    ulp of each value over 2 h is half of that; the other half is left for the sums before the last
    rounding). That premise needs an SDF that is not the small remainder of larger cancelling terms, so
    the output bias is 1: with it |sdf| ~ 1 is the largest partial sum. (With a zero bias |sdf| ~ 0.3
    sits under 64 terms of absolute sum ~ 1 and the quotient misses the bound by 1.8x - 2.3x.)
    Points whose +-h neighbours leave a cell of either level or flip a layer-1 ReLU are set aside:
    4.0 % of the 2000 points with seed 0 and h = 2^-12 (cap 10 %; 16.2 % at h = 2^-10)."""
    from bundlesdf_amd.grid import level_layout
    from bundlesdf_amd.nerf_helpers import NeRFSmall
    from oracle import kernels as K
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    L, base, finest, h = 2, 4, 8, 2.0 ** -12
    pls, offsets = level_layout(3, L, 2, base, 12, finest)
    S_log = float(np.log2(pls))
    emb = torch.from_numpy(rng.uniform(-1, 1, (int(offsets[-1]), 2)).astype(np.float32))
    net = NeRFSmall(2, 64, 15, 3, 64, input_ch=2 * L, input_ch_views=9)
    W = {k: v.detach().clone() for k, v in net.state_dict().items()}
    W["sigma_net.2.bias"][0] = 1.0   # |sdf| ~ 1 dominates the terms it is summed from: no cancellation
    n = 2000
    pts = rng.uniform(-0.99, 0.99, (n, 3)).astype(np.float32)
    ref = QO.field_query(pts, emb, offsets, S_log, base, W)
    scales, _ = K.level_params(L, S_log, base)

    def cells(p):
        x01 = (p + np.float32(1)) / np.float32(2)
        return np.stack([np.floor(x01 * np.float32(s) + np.float32(0.5)) for s in scales], -1)

    keep = np.ones(n, bool)
    fd = np.zeros((n, 3))
    mag = np.zeros((n, 3))
    sign0, cell0 = ref["pre1"].numpy() > 0, cells(pts)
    for d in range(3):
        side = []
        for s in (-1, 1):
            p = pts.copy()
            p[:, d] += np.float32(s * h)
            o = QO.field_query(p, emb, offsets, S_log, base, W)
            keep &= ((o["pre1"].numpy() > 0) == sign0).all(1) & (cells(p) == cell0).all((1, 2))
            side.append((p[:, d].astype(np.float64), o["sdf"].numpy().astype(np.float64)))
        fd[:, d] = (side[1][1] - side[0][1]) / (side[1][0] - side[0][0])
        mag[:, d] = np.maximum(np.abs(side[0][1]), np.abs(side[1][1]))
    share = 1 - keep.mean()
    err = np.abs(fd - ref["normal"].numpy().astype(np.float64))[keep]
    tol = (np.finfo(np.float32).eps * mag / h)[keep]
    print(f"set aside {share:.3f}; max err {err.max():.3e}; max err / tol {np.max(err / tol):.3f}")
    assert share <= 0.10, share
    assert (err <= tol).all(), float(np.max(err / tol))


def _call(libnof, **kw):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = dict(table=p, table_dtype=0, level_table=p, L=16, frags=p, bias=p, mlp_dtype=0, mlp_in=32, points=p, n=4,
             ff=None, n_frames=0, n_ff=0, frame_id=0, sdf=p, grad=p, rgb=p)
    a.update(kw)
    rc = libnof.nof_query_field(a["table"], a["table_dtype"], a["level_table"], a["L"], a["frags"], a["bias"],
                                a["mlp_dtype"], a["mlp_in"], a["points"], a["n"], a["ff"], a["n_frames"], a["n_ff"],
                                a["frame_id"], a["sdf"], a["grad"], a["rgb"], None)
    return rc, libnof.nof_last_error(), p


def test_query_field_refuses_bad_arguments_before_device_work(libnof):
    """Every refusal is NOF_EINVAL (1) with its message and comes before the first HIP call: the
    pointers are host memory and there is no device here."""
    rc, msg, p = _call(libnof, sdf=None, grad=None, rgb=None)
    assert rc == 1 and b"no output" in msg
    rc, msg, _ = _call(libnof, points=None)
    assert rc == 1 and b"points is NULL" in msg
    rc, msg, _ = _call(libnof, n=-1)
    assert rc == 1 and b"negative" in msg
    rc, msg, _ = _call(libnof, table_dtype=1, mlp_dtype=0)
    assert rc == 1 and b"dtypes must match" in msg
    rc, msg, _ = _call(libnof, L=17, mlp_in=34)
    assert rc == 1 and b"L<=16" in msg
    rc, msg, _ = _call(libnof, L=16, mlp_in=64)   # C = 4
    assert rc == 1 and b"C=2" in msg
    for fid in (-1, 3):
        rc, msg, _ = _call(libnof, ff=p, n_frames=3, n_ff=2, frame_id=fid)
        assert rc == 1 and b"frame_id" in msg
    rc, msg, _ = _call(libnof, table=None)
    assert rc == 1 and b"table" in msg
    # n == 0: success, nothing launched (null points are fine then)
    assert _call(libnof, n=0, points=None)[0] == 0
    assert _call(libnof, n=0, ff=p, n_frames=3, n_ff=2, frame_id=2)[0] == 0


def _mesh():
    from bundlesdf_amd.mesh import Mesh
    return Mesh([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25], [1, 1, -0.125]], [[0, 1, 2], [1, 3, 2]])


def _attr_mesh():
    m = _mesh()
    nrm = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], np.float64)
    m.vertex_normals = nrm.copy()
    m.vertex_colors = np.array([[255, 0, 0], [0, 128, 7], [1, 2, 3], [250, 251, 252]], np.uint8)
    return m


def test_mesh_attributes_default_to_none_and_follow_their_vertices():
    from bundlesdf_amd.mesh import Mesh
    assert _mesh().vertex_normals is None and _mesh().vertex_colors is None
    m = _attr_mesh()
    c = m.copy()
    assert np.array_equal(c.vertex_normals, m.vertex_normals) and np.array_equal(c.vertex_colors, m.vertex_colors)
    c.vertex_normals[0, 0] = 9
    c.vertex_colors[0, 0] = 9
    assert m.vertex_normals[0, 0] == 0 and m.vertex_colors[0, 0] == 255          # deep copies
    # update_vertices: rows follow the kept vertices
    k = m.copy().update_vertices([False, True, True, True])
    assert np.array_equal(k.vertex_colors, m.vertex_colors[1:]) and np.array_equal(k.vertex_normals, m.vertex_normals[1:])
    assert k.faces.tolist() == [[0, 2, 1]]
    # merge_vertices: np.unique sorts the positions; each new vertex keeps the row of its old one
    d = Mesh(np.concatenate([m.vertices[::-1], m.vertices[:1]]), [[0, 1, 2], [2, 3, 4]])
    d.vertex_colors = np.concatenate([m.vertex_colors[::-1], m.vertex_colors[:1]])
    d.vertex_normals = np.concatenate([m.vertex_normals[::-1], m.vertex_normals[:1]])
    d.merge_vertices()
    assert len(d.vertices) == 4
    for v, col, nr in zip(d.vertices, d.vertex_colors, d.vertex_normals):
        i = int(np.flatnonzero((m.vertices == v).all(1))[0])
        assert np.array_equal(col, m.vertex_colors[i]) and np.array_equal(nr, m.vertex_normals[i])
    # apply_transform: normals rotate, they do not translate
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [5, 6, 7]
    t = m.copy().apply_transform(T)
    np.testing.assert_allclose(t.vertex_normals, m.vertex_normals @ T[:3, :3].T, atol=0)
    np.testing.assert_allclose(t.vertices, m.vertices @ T[:3, :3].T + T[:3, 3], atol=0)
    assert np.array_equal(t.vertex_colors, m.vertex_colors)


def _parse_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property") and "list" not in ln]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[ty]) for ty, name in props])
    v = np.frombuffer(body[:nv * dt.itemsize], dt)
    faces = np.frombuffer(body[nv * dt.itemsize:], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    return v, faces["i"]


def _parse_obj(path):
    v, vn, f = [], [], []
    for ln in open(path).read().split("\n"):
        t = ln.split()
        if not t:
            continue
        if t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t[0] == "vn":
            vn.append([float(x) for x in t[1:]])
        elif t[0] == "f":
            f.append(t[1:])
    return np.array(v), np.array(vn), f


def test_mesh_export_with_attributes_parses_back(tmp_path):
    m = _attr_mesh()
    m.export(str(tmp_path / "a.ply"))
    v, faces = _parse_ply(str(tmp_path / "a.ply"))
    assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), m.vertices.astype(np.float32))
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), m.vertex_normals.astype(np.float32))
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), m.vertex_colors)
    assert np.array_equal(faces, m.faces)
    m.export(str(tmp_path / "a.obj"))
    v, vn, f = _parse_obj(str(tmp_path / "a.obj"))
    assert v.shape == (4, 6) and vn.shape == (4, 3)
    np.testing.assert_allclose(v[:, :3], m.vertices, atol=5e-7)
    np.testing.assert_allclose(v[:, 3:], m.vertex_colors / 255.0, atol=5e-7)
    assert np.array_equal(np.round(v[:, 3:] * 255).astype(np.uint8), m.vertex_colors)
    np.testing.assert_allclose(vn, m.vertex_normals, atol=5e-7)
    assert f == [["1//1", "2//2", "3//3"], ["2//2", "4//4", "3//3"]]
    # textured: a/a/a
    m.uv = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float64)
    m.texture = np.zeros((2, 2, 3), np.uint8)
    m.export(str(tmp_path / "t.obj"))
    assert _parse_obj(str(tmp_path / "t.obj"))[2] == [["1/1/1", "2/2/2", "3/3/3"], ["2/2/2", "4/4/4", "3/3/3"]]
    # one attribute alone
    n_only = _attr_mesh()
    n_only.vertex_colors = None
    n_only.export(str(tmp_path / "n.ply"))
    assert _parse_ply(str(tmp_path / "n.ply"))[0].dtype.names == ("x", "y", "z", "nx", "ny", "nz")
    c_only = _attr_mesh()
    c_only.vertex_normals = None
    c_only.export(str(tmp_path / "c.obj"))
    v, vn, f = _parse_obj(str(tmp_path / "c.obj"))
    assert v.shape == (4, 6) and vn.shape == (0,) and f[0] == ["1", "2", "3"]


# what the commit before vertex attributes wrote for _mesh()
_PARENT_OBJ = (b'v 0.000000 0.000000 0.000000\nv 1.000000 0.000000 0.500000\nv 0.000000 1.000000 0.250000\n'
               b'v 1.000000 1.000000 -0.125000\nf 1 2 3\nf 2 4 3\n')
_PARENT_PLY = (b'ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n'
               b'property float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n'
               b'\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00?'
               b'\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x80>\x00\x00\x80?\x00\x00\x80?\x00\x00\x00\xbe'
               b'\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00\x03\x01\x00\x00\x00\x03\x00\x00\x00\x02\x00\x00\x00')


def test_mesh_export_without_attributes_is_byte_identical(tmp_path):
    m = _mesh()
    m.export(str(tmp_path / "p.obj"))
    m.export(str(tmp_path / "p.ply"))
    assert open(tmp_path / "p.obj", "rb").read() == _PARENT_OBJ
    assert open(tmp_path / "p.ply", "rb").read() == _PARENT_PLY


def _hook_runner(cfg, tmp_path):
    from bundlesdf_amd.nerf_runner import NerfRunner

    class Trainer:
        calls = 0

        def query_field(self, points, sdf=True, normals=False, colour=False, frame_id=0, **kw):
            if not cfg.get("mesh_vertex_attributes"):
                raise AssertionError("query_field called with mesh_vertex_attributes unset")
            self.calls += 1
            n = len(points)
            out = {}
            if normals:
                out["normals"] = torch.tensor([[0.0, 0.0, 2.0]]).repeat(n, 1)
            if colour:
                out["colour"] = torch.full((n, 3), 0.5)
            return out

    nr = object.__new__(NerfRunner)
    nr.cfg = dict(cfg, save_dir=str(tmp_path), mesh_resolution=0.01, translation=np.zeros(3), sc_factor=1.0,
                  optimize_poses=0)
    nr.global_step, nr._run, nr.trainer, nr.models = 7, None, Trainer(), {}
    nr.poses = np.eye(4)[None]
    nr.extract_mesh = lambda **kw: _mesh()
    return nr


def test_hook_mesh_queries_the_field_only_when_asked(tmp_path):
    nr = _hook_runner({}, tmp_path / "off")
    nr._hook_mesh()
    path = tmp_path / "off" / "step_0000007_mesh_normalized_space.obj"
    assert open(path, "rb").read() == _PARENT_OBJ and nr.trainer.calls == 0
    assert nr.mesh.vertex_normals is None and nr.mesh.vertex_colors is None
    nr = _hook_runner({"mesh_vertex_attributes": True}, tmp_path / "on")
    nr._hook_mesh()
    for name in ("normalized_space", "real_world"):
        v, vn, f = _parse_obj(str(tmp_path / "on" / f"step_0000007_mesh_{name}.obj"))
        assert v.shape == (4, 6) and np.allclose(vn, [0, 0, 1]) and f[0] == ["1//1", "2//2", "3//3"]
        assert np.allclose(v[:, 3:], 127 / 255.0, atol=5e-7)          # (0.5 * 255) truncated
    assert nr.trainer.calls == 2 and nr.mesh.vertex_colors.dtype == np.uint8
