"""Mesh extraction: NerfRunner.extract_mesh
(nerf_runner.py:1349-1408) = SDF on a dense grid (nof_query_sdf, the fused
encode + sigma-net kernel) + marching cubes + rescale.

The reference calls skimage.measure.marching_cubes (Lewiner) and wraps the
result in a trimesh.Trimesh; neither package is available here, so this module
implements marching cubes on the device with torch tensor ops and returns a
small Mesh (vertices, faces, export to .ply/.obj). PARITY UNPINNED against
skimage: the case table below is generated (not the Lewiner table); both
produce a closed, consistently oriented surface through the same edge
crossings (linear interpolation of the SDF along grid edges), so vertex
positions agree while the triangulation of ambiguous cells may differ.

Case table construction: for each of the 256 sign configurations, every cube
face contributes the contour segments of its marching-squares case, oriented
(viewed from outside the cube, counter-clockwise boundary walk) from the
crossing where the walk leaves the inside to the crossing where it enters it;
ambiguous faces separate the inside corners. Each crossing lies on two faces
that walk its edge in opposite directions, so the segments chain into closed
loops, which are fan-triangulated. The face rule depends only on the face's
own corner signs, so neighbouring cubes agree and the surface is watertight.
"""
import numpy as np
import torch

from ._args import as_tensor, default_device

# corner c of a cube = offset (c & 1, c >> 1 & 1, c >> 2 & 1) along (i, j, k)
_CORNERS = np.array([[(c >> d) & 1 for d in range(3)] for c in range(8)])
# edge e = (corner with bit `axis` clear, axis): 4 per axis
_EDGES = [(c, ax) for ax in range(3) for c in range(8) if not (c >> ax) & 1]
_EDGE_ID = {(c, c | (1 << ax)): e for e, (c, ax) in enumerate(_EDGES)}
_EDGE_ID.update({(c | (1 << ax), c): e for e, (c, ax) in enumerate(_EDGES)})


def _faces():
    """6 faces as 4 corners in counter-clockwise order seen from outside."""
    out = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, 1):
            base = side << ax
            ring = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            # (u, v, ax) is right-handed: this ring is CCW seen from +ax; reverse for the -ax face
            out.append(ring if side == 1 else ring[::-1])
    return out


def _build_tables():
    faces = _faces()
    tris = []
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        seg = {}
        for ring in faces:
            cross = []   # (edge id, 'out' if the walk leaves the inside here, else 'in')
            for k in range(4):
                a, b = ring[k], ring[(k + 1) % 4]
                if inside[a] != inside[b]:
                    cross.append((_EDGE_ID[(a, b)], "out" if inside[a] else "in"))
            if not cross:
                continue
            # pair every 'out' crossing with the 'in' crossing before it along the walk:
            # the inside corners of an ambiguous face stay separated
            n = len(cross)
            for k in range(n):
                e, kind = cross[k]
                if kind == "out":
                    prev = cross[(k - 1) % n]
                    assert prev[1] == "in"
                    seg[e] = prev[0]      # segment from the 'out' crossing to that 'in' crossing
        loops, seen = [], set()
        for start in seg:
            if start in seen:
                continue
            loop, e = [], start
            while e not in seen:
                seen.add(e)
                loop.append(e)
                e = seg[e]
            loops.append(loop)
        t = []
        for loop in loops:
            for k in range(1, len(loop) - 1):
                t.append((loop[0], loop[k], loop[k + 1]))
        tris.append(t)
    width = max(len(t) for t in tris)
    table = np.full((256, width, 3), -1, np.int64)
    count = np.zeros(256, np.int64)
    for case, t in enumerate(tris):
        count[case] = len(t)
        if t:
            table[case, :len(t)] = np.array(t)
    return table, count


TRI_TABLE, TRI_COUNT = _build_tables()
EDGE_CORNER = np.array([c for c, _ in _EDGES])
EDGE_AXIS = np.array([ax for _, ax in _EDGES])


class Mesh:
    """Minimal stand-in for trimesh.Trimesh(vertices, faces, process=False)."""

    def __init__(self, vertices, faces):
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces, np.int64)
        self.uv = None          # [V,2] texture coordinates (texture.unwrap)
        self.texture = None     # [H,W,3] uint8 image (texture.bake_texture), row 0 = top
        self.vertex_normals = None   # [V,3] float, unit length (NerfRunner.mesh_vertex_normals_from_network)
        self.vertex_colors = None    # [V,3] uint8 (NerfRunner.mesh_vertex_color_from_network / _from_train_images)
        self.vertex_color_counts = None   # [V] int32: frames that coloured the vertex (_from_train_images)

    @property
    def face_normals(self):
        v = self.vertices[self.faces]
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)

    def apply_transform(self, T):
        T = np.asarray(T, np.float64)
        self.vertices = self.vertices @ T[:3, :3].T + T[:3, 3]
        if self.vertex_normals is not None:   # directions: the rotation part only
            self.vertex_normals = np.asarray(self.vertex_normals, np.float64) @ T[:3, :3].T
        return self

    @property
    def edges(self):
        return self.faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)

    def copy(self):
        m = Mesh(self.vertices.copy(), self.faces.copy())
        m.uv = None if self.uv is None else self.uv.copy()
        m.texture = None if self.texture is None else self.texture.copy()
        m.vertex_normals = None if self.vertex_normals is None else self.vertex_normals.copy()
        m.vertex_colors = None if self.vertex_colors is None else self.vertex_colors.copy()
        m.vertex_color_counts = None if self.vertex_color_counts is None else self.vertex_color_counts.copy()
        return m

    def _take_vertex_rows(self, rows):
        """Per-vertex attributes follow their vertices (rows: index array or mask of the old vertices)."""
        if self.vertex_normals is not None:
            self.vertex_normals = np.asarray(self.vertex_normals)[rows]
        if self.vertex_colors is not None:
            self.vertex_colors = np.asarray(self.vertex_colors)[rows]
        if self.vertex_color_counts is not None:
            self.vertex_color_counts = np.asarray(self.vertex_color_counts)[rows]

    def merge_vertices(self):
        """Weld vertices at identical positions (marching_cubes output already shares them)."""
        v, first, inv = np.unique(self.vertices, axis=0, return_index=True, return_inverse=True)
        self.vertices, self.faces = v, inv.reshape(-1)[self.faces]
        self._take_vertex_rows(first)   # a welded vertex keeps the attributes of its first occurrence
        return self

    def remove_duplicate_faces(self):
        """Drop faces with the same vertex set as an earlier face (first kept)."""
        key = np.sort(self.faces, axis=1)
        _, first = np.unique(key, axis=0, return_index=True)
        self.faces = self.faces[np.sort(first)]
        return self

    def update_vertices(self, mask):
        """Keep the vertices in `mask` and the faces whose corners are all kept."""
        mask = np.asarray(mask, bool)
        remap = np.cumsum(mask) - 1
        keep = mask[self.faces].all(1)
        self.faces = remap[self.faces[keep]]
        self.vertices = self.vertices[mask]
        self._take_vertex_rows(mask)
        return self

    def compute_vertex_normals(self, backend="hip"):
        """Set and return vertex_normals [V,3] f64 from the geometry: per vertex the unnormalised
        (v1 - v0) x (v2 - v0) of its faces (area weights) added in ascending face index, divided by
        the sum's length; a zero sum gives (0, 0, 0). backend "hip": nof_mesh_vertex_normals, a gather
        over the vertex -> face CSR; "scipy": the same sums in numpy on the host."""
        _check_backend("compute_vertex_normals", backend)
        V = len(self.vertices)
        dev = default_device() if backend == "hip" else torch.device("cpu")
        faces = _checked_faces("compute_vertex_normals", self.faces, V, dev)
        row_start, face_ids = vertex_faces(faces, V, device=dev)
        if backend == "hip":
            from . import _lib
            v = as_tensor(self.vertices, np.float64).to(dev)
            f32 = faces.to(torch.int32).contiguous()
            out = torch.empty_like(v)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().nof_mesh_vertex_normals(_lib.ptr(v), _lib.ptr(f32), _lib.ptr(row_start),
                                                              _lib.ptr(face_ids), V, _lib.ptr(out), _lib.stream_of(v)),
                           "mesh_vertex_normals")
            self.vertex_normals = out.cpu().numpy()
            return self.vertex_normals
        v, f = self.vertices, faces.numpy()
        t = v[f]
        fn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).reshape(-1, 3)
        rs, ids = row_start.numpy().astype(np.int64), face_ids.numpy()
        s = np.zeros((V, 3))
        deg = np.diff(rs)
        for r in range(int(deg.max()) if V else 0):     # the r-th face of every row that has one: ascending order
            rows = np.flatnonzero(deg > r)
            s[rows] = s[rows] + fn[ids[rs[rows] + r]]
        n = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = n > 0
        self.vertex_normals = np.where(ok[:, None], s / np.where(ok, n, 1.0)[:, None], 0.0)
        return self.vertex_normals

    def export(self, path):
        if path.endswith(".obj"):
            import os
            textured = self.uv is not None and self.texture is not None
            base = os.path.splitext(path)[0]
            with open(path, "w") as f:
                if textured:
                    f.write(f"mtllib {os.path.basename(base)}.mtl\nusemtl material0\n")
                if self.vertex_colors is not None:   # the common "v x y z r g b" extension, colours in [0, 1]
                    for v, c in zip(self.vertices, np.asarray(self.vertex_colors, np.float64) / 255.0):
                        f.write(f"v {v[0]:.6f} {v[1]:.6f} {v[2]:.6f} {c[0]:.6f} {c[1]:.6f} {c[2]:.6f}\n")
                else:
                    for v in self.vertices:
                        f.write(f"v {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")
                normals = self.vertex_normals is not None
                if normals:
                    for v in self.vertex_normals:
                        f.write(f"vn {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")
                if textured:
                    for t in self.uv:
                        f.write(f"vt {t[0]:.6f} {t[1]:.6f}\n")
                    for t in self.faces + 1:
                        if normals:
                            f.write(f"f {t[0]}/{t[0]}/{t[0]} {t[1]}/{t[1]}/{t[1]} {t[2]}/{t[2]}/{t[2]}\n")
                        else:
                            f.write(f"f {t[0]}/{t[0]} {t[1]}/{t[1]} {t[2]}/{t[2]}\n")
                elif normals:
                    for t in self.faces + 1:
                        f.write(f"f {t[0]}//{t[0]} {t[1]}//{t[1]} {t[2]}//{t[2]}\n")
                else:
                    for t in self.faces + 1:
                        f.write(f"f {t[0]} {t[1]} {t[2]}\n")
            if textured:
                with open(base + ".mtl", "w") as f:
                    f.write(f"newmtl material0\nKa 1 1 1\nKd 1 1 1\nmap_Kd {os.path.basename(base)}.png\n")
                write_png(base + ".png", self.texture)
        elif path.endswith(".ply"):
            with open(path, "wb") as f:
                props, fields = "", [("p", "<f4", 3)]
                if self.vertex_normals is not None:
                    props += "property float nx\nproperty float ny\nproperty float nz\n"
                    fields.append(("n", "<f4", 3))
                if self.vertex_colors is not None:
                    props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                    fields.append(("c", "u1", 3))
                f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(self.vertices)}\n"
                         "property float x\nproperty float y\nproperty float z\n" + props +
                         f"element face {len(self.faces)}\nproperty list uchar int vertex_indices\n"
                         "end_header\n").encode())
                vrec = np.zeros(len(self.vertices), dtype=fields)
                vrec["p"] = self.vertices
                if self.vertex_normals is not None:
                    vrec["n"] = self.vertex_normals
                if self.vertex_colors is not None:
                    vrec["c"] = self.vertex_colors
                f.write(vrec.tobytes())
                rec = np.zeros(len(self.faces), dtype=[("n", "u1"), ("i", "<i4", 3)])
                rec["n"] = 3
                rec["i"] = self.faces
                f.write(rec.tobytes())
        else:
            raise ValueError("Mesh.export: .obj or .ply")


    @staticmethod
    def load(path):
        """Read a .obj that Mesh.export wrote: `v x y z [r g b]` (colours in [0, 1] -> uint8), `vn`, `vt`,
        faces `f a b c` with corners `a`, `a/a`, `a//a` or `a/a/a` (one index for position, uv and normal: the
        attributes are per vertex), and `mtllib` -> the .mtl beside the file -> `map_Kd` -> the .png
        beside it as the texture. `usemtl`, blank lines and `#` comments are skipped; anything else raises
        ValueError naming the file and line."""
        import os

        def bad(no, line, why):
            return ValueError(f"Mesh.load: {path}:{no}: {why}: {line.strip()!r}")

        def floats(no, line, tok, counts):
            try:
                vals = [float(x) for x in tok]
            except ValueError:
                raise bad(no, line, "not a number") from None
            if len(vals) not in counts or not np.isfinite(vals).all():
                raise bad(no, line, f"expected {' or '.join(str(c) for c in counts)} finite numbers")
            return vals

        if not path.endswith(".obj"):
            raise ValueError("Mesh.load: .obj")
        v, vc, vn, vt, faces, mtl = [], [], [], [], [], None
        with open(path) as fh:
            for no, line in enumerate(fh, 1):
                tok = line.split()
                if not tok or tok[0].startswith("#") or tok[0] == "usemtl":
                    continue
                if tok[0] == "v":
                    vals = floats(no, line, tok[1:], (3, 6))
                    v.append(vals[:3])
                    if len(vals) == 6:
                        vc.append(vals[3:])
                    if len(vc) not in (0, len(v)):
                        raise bad(no, line, "some vertices carry a colour and some do not")
                elif tok[0] == "vn":
                    vn.append(floats(no, line, tok[1:], (3,)))
                elif tok[0] == "vt":
                    vt.append(floats(no, line, tok[1:], (2,)))
                elif tok[0] == "f":
                    if len(tok) != 4:
                        raise bad(no, line, "a face must have three corners")
                    corner = []
                    for t in tok[1:]:
                        parts = t.split("/")
                        idx = [p for p in parts if p != ""]
                        if len(parts) > 3 or not idx or not all(p.isdigit() for p in idx) or len(set(idx)) != 1 \
                                or parts[0] == "" or int(idx[0]) < 1:
                            raise bad(no, line, "a corner must be a, a/a, a//a or a/a/a with a >= 1")
                        corner.append(int(idx[0]) - 1)
                    faces.append(corner)
                elif tok[0] == "mtllib" and len(tok) == 2:
                    mtl = tok[1]
                else:
                    raise bad(no, line, "unsupported line")
        n = len(v)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        if len(f) and int(f.max()) >= n:
            raise ValueError(f"Mesh.load: {path}: a face names vertex {int(f.max()) + 1} of {n}")
        for name, rows in (("vn", vn), ("vt", vt)):
            if rows and len(rows) != n:
                raise ValueError(f"Mesh.load: {path}: {len(rows)} {name} lines for {n} vertices")
        mesh = Mesh(np.asarray(v, np.float64).reshape(-1, 3), f)
        if vc:
            mesh.vertex_colors = np.clip(np.rint(np.asarray(vc) * 255.0), 0, 255).astype(np.uint8)
        if vn:
            mesh.vertex_normals = np.asarray(vn, np.float64)
        if vt:
            mesh.uv = np.asarray(vt, np.float64)
        if mtl is not None:
            folder = os.path.dirname(path)
            image = None
            with open(os.path.join(folder, mtl)) as fh:
                for no, line in enumerate(fh, 1):
                    tok = line.split()
                    if tok and tok[0] == "map_Kd":
                        if len(tok) != 2:
                            raise ValueError(f"Mesh.load: {os.path.join(folder, mtl)}:{no}: map_Kd takes one file name: "
                                             f"{line.strip()!r}")
                        image = tok[1]
            if image is not None:
                mesh.texture = read_png(os.path.join(folder, image))
        return mesh


def read_png(path):
    """The uint8 [H,W,3] image of an 8-bit RGB, non-interlaced PNG (what write_png writes; every
    row filter is undone). Anything else raises ValueError."""
    import struct
    import zlib
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"read_png: {path} is not a PNG file")
    pos, head, idat = 8, None, b""
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"read_png: {path}: only 8-bit RGB without interlacing is read")
    W, H = head[:2]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    if raw.size != H * (1 + 3 * W):
        raise ValueError(f"read_png: {path}: {raw.size} bytes of image data for {W}x{H}")
    raw = raw.reshape(H, 1 + 3 * W)
    if not raw[:, 0].any():                       # filter 0 on every row
        return raw[:, 1:].reshape(H, W, 3).copy()
    out = np.zeros((H, 3 * W), np.int64)
    for r in range(H):
        ft, row = int(raw[r, 0]), raw[r, 1:].astype(np.int64)
        up = out[r - 1] if r else np.zeros(3 * W, np.int64)
        if ft == 0:
            out[r] = row
        elif ft == 2:
            out[r] = (row + up) & 255
        elif ft in (1, 3, 4):
            for x in range(3 * W):
                a = out[r, x - 3] if x >= 3 else 0
                b, c = up[x], (up[x - 3] if x >= 3 else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                out[r, x] = (row[x] + pred) & 255
        else:
            raise ValueError(f"read_png: {path}: row {r} has filter type {ft}")
    return out.astype(np.uint8).reshape(H, W, 3)


def write_png(path, img):
    """8-bit RGB PNG (zlib, no external imaging library)."""
    import struct
    import zlib
    img = np.ascontiguousarray(np.asarray(img, np.uint8))
    H, W = img.shape[:2]
    raw = b"".join(b"\x00" + img[r].tobytes() for r in range(H))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def device_tables(device):
    """The [256,16] uint8 case table nof_marching_cubes_* read, on `device`: per case TRI_COUNT, then the
    5 x 3 entries of TRI_TABLE, each table edge e as EDGE_CORNER[e] | EDGE_AXIS[e] << 3 (unused slots 0)."""
    key = str(device)
    if key not in _DEVICE_TABLES:
        # the kernels take corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1): _CORNERS' construction
        assert all(tuple(_CORNERS[c]) == (c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8))
        assert TRI_TABLE.shape == (256, 5, 3) and int(TRI_COUNT.max()) <= 5
        code = EDGE_CORNER | (EDGE_AXIS << 3)
        t = np.zeros((256, 16), np.uint8)
        t[:, 0] = TRI_COUNT
        t[:, 1:] = np.where(TRI_TABLE >= 0, code[np.maximum(TRI_TABLE, 0)], 0).reshape(256, 15)
        _DEVICE_TABLES[key] = torch.from_numpy(t).to(device)
    return _DEVICE_TABLES[key]


_DEVICE_TABLES = {}


def marching_cubes_device(volume, level=0.0):
    """marching_cubes on the device with the HIP kernels of csrc/mesh.hip (nof_marching_cubes_count /
    _emit): device tensors (vertices float32 [V,3] in index coordinates, faces int32 [F,3]), equal to
    marching_cubes(volume, level) bit for bit and in the same order. `volume` [N0,N1,N2]: a device tensor is
    used where it is (float32 contiguous: no copy), anything else is copied to the current device. One
    host read: the totals (V, F) with the volume's value range. At most 4 bytes of scratch per grid
    point (plus 32 per 256 points)."""
    from . import _lib
    vol = torch.as_tensor(volume)
    if not vol.is_cuda:
        vol = vol.to(default_device())
    vol = vol.float().contiguous()
    if vol.dim() != 3:
        raise ValueError(f"marching_cubes_device: volume must be [N0,N1,N2], got {tuple(vol.shape)}")
    dev = vol.device
    n0, n1, n2 = (int(n) for n in vol.shape)
    if max(n0, n1, n2) >= 1 << 31:
        raise ValueError(f"marching_cubes_device: volume {n0} x {n1} x {n2} is too large")
    L = _lib.lib()
    nb = _lib.ctypes.c_int64(0)
    _lib.check(L.nof_marching_cubes_blocks(n0, n1, n2, _lib.ctypes.byref(nb)), "marching_cubes_blocks")
    nb = nb.value
    with torch.cuda.device(dev):
        tables = device_tables(dev)
        cells = torch.empty(n0 * n1 * n2, dtype=torch.int32, device=dev)
        counts = torch.empty((nb, 2), dtype=torch.int32, device=dev)
        rng = torch.empty((nb, 2), dtype=torch.float32, device=dev)
        st = _lib.stream_of(vol)
        _lib.check(L.nof_marching_cubes_count(_lib.ptr(vol), n0, n1, n2, level, _lib.ptr(tables), _lib.ptr(cells),
                                              _lib.ptr(counts), _lib.ptr(rng), st), "marching_cubes_count")
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        base = (incl - counts).contiguous()
        stats = torch.cat([incl[-1].double(), rng[:, 0].min().double()[None], rng[:, 1].max().double()[None]]).cpu()
        V, F, lo, hi = int(stats[0]), int(stats[1]), float(stats[2]), float(stats[3])
        if not (lo <= level <= hi):
            raise ValueError("Surface level must be within volume data range.")   # as skimage
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        if V:
            _lib.check(L.nof_marching_cubes_emit(_lib.ptr(vol), n0, n1, n2, level, _lib.ptr(tables), _lib.ptr(cells),
                                                 _lib.ptr(base), V, F, _lib.ptr(verts), _lib.ptr(faces), st),
                       "marching_cubes_emit")
    return verts, faces


def component_labels(faces, n_vertices, device=None):
    """Connected components of a triangle list on the device (nof_mesh_components): an int32 device tensor
    [n_vertices], labels[v] = the smallest vertex index of v's component (a vertex in no face labels itself).
    Ranking the labels gives scipy's connected_components numbering, which numbers components by their
    first vertex. The kernel does one hook-and-compress sweep; this loop repeats it until a sweep changes
    nothing, reading one flag per sweep."""
    from . import _lib
    f = torch.as_tensor(faces)
    f = f.to(device=default_device(f, device), dtype=torch.int32).reshape(-1, 3).contiguous()
    n = int(n_vertices)
    if len(f) and (int(f.min()) < 0 or int(f.max()) >= n):
        raise ValueError(f"component_labels: face corners must be in [0, {n})")
    L = _lib.lib()
    with torch.cuda.device(f.device):
        labels = torch.arange(n, dtype=torch.int32, device=f.device)
        changed = torch.zeros(1, dtype=torch.int32, device=f.device)
        if n == 0 or len(f) == 0:
            return labels
        for _ in range(n + 1):
            _lib.check(L.nof_mesh_components(_lib.ptr(f), len(f), n, _lib.ptr(labels), _lib.ptr(changed),
                                             _lib.stream_of(f)), "mesh_components")
            if int(changed.item()) == 0:
                return labels
    raise RuntimeError(f"component_labels: no fixed point after {n + 1} sweeps")


def marching_cubes(volume, level=0.0, backend="torch"):
    """(vertices [V,3] in index coordinates, faces [F,3]) of the `level` set of
    a [N0,N1,N2] volume (torch tensor on any device, or numpy). Faces are
    oriented with normals towards increasing values (outside of an SDF).
    backend "torch": the tensor ops below, on the volume's device; "hip":
    marching_cubes_device, the same arrays from the HIP kernels."""
    if backend == "hip":
        verts, faces = marching_cubes_device(volume, level)
        return verts.double().cpu().numpy(), faces.long().cpu().numpy()
    if backend != "torch":
        raise ValueError(f"marching_cubes: backend must be 'torch' or 'hip', got {backend!r}")
    vol = torch.as_tensor(volume)
    dev = vol.device
    vol = vol.float()
    N0, N1, N2 = vol.shape
    if not (float(vol.min()) <= level <= float(vol.max())):
        raise ValueError("Surface level must be within volume data range.")   # as skimage
    inside = (vol < level)
    case = torch.zeros((N0 - 1, N1 - 1, N2 - 1), dtype=torch.int64, device=dev)
    for c in range(8):
        dx, dy, dz = _CORNERS[c]
        case |= inside[dx:N0 - 1 + dx, dy:N1 - 1 + dy, dz:N2 - 1 + dz].long() << c
    count = torch.as_tensor(TRI_COUNT, device=dev)[case]
    cubes = torch.nonzero(count > 0)
    if cubes.numel() == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    ccase = case[cubes[:, 0], cubes[:, 1], cubes[:, 2]]
    tri = torch.as_tensor(TRI_TABLE, device=dev)[ccase]                    # [C, W, 3]
    valid = tri[..., 0] >= 0
    cube_of = cubes[:, None, None, :].expand(-1, tri.shape[1], 3, 3)[valid]  # [T, 3, 3]
    edges = tri[valid]                                                      # [T, 3]
    corner = torch.as_tensor(_CORNERS, device=dev)[torch.as_tensor(EDGE_CORNER, device=dev)[edges]]
    axis = torch.as_tensor(EDGE_AXIS, device=dev)[edges]
    p0 = cube_of + corner                                                   # [T, 3, 3] grid point
    key = ((p0[..., 0] * N1 + p0[..., 1]) * N2 + p0[..., 2]) * 3 + axis
    ukey, inv = torch.unique(key.reshape(-1), return_inverse=True)
    ax = ukey % 3
    g = ukey // 3
    q0 = torch.stack([g // (N1 * N2), (g // N2) % N1, g % N2], -1)
    q1 = q0.clone()
    q1[torch.arange(len(ax), device=dev), ax] += 1
    v0 = vol[q0[:, 0], q0[:, 1], q0[:, 2]]
    v1 = vol[q1[:, 0], q1[:, 1], q1[:, 2]]
    t = ((level - v0) / (v1 - v0)).clamp(0, 1)
    verts = q0.float() + t[:, None] * (q1 - q0).float()
    faces = inv.reshape(-1, 3)
    # generated loops run with the inside on the left seen from outside the surface;
    # flip to make the normals point towards increasing values
    faces = faces[:, [0, 2, 1]]
    return verts.double().cpu().numpy(), faces.cpu().numpy()


def grid_axes(bounds, voxel_size):
    """extract_mesh's query axes (nerf_runner.py:1354-1360): numpy float64 arange,
    stored as float32 like the reference's query tensor."""
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    return [np.arange(b[0, d] + 0.5 * voxel_size, b[1, d], voxel_size) for d in range(3)]


def trimesh_split(mesh, min_edge=1000, backend="scipy"):
    """Connected components with at least `min_edge` vertices, as separate meshes
    (Utils.py:287-298, trimesh.graph.connected_components over mesh.edges).
    backend "scipy": on the host; "hip": component_labels on the device, the
    same parts in the same order (components by their lowest vertex)."""
    if backend == "hip":
        n = len(mesh.vertices)
        label = component_labels(mesh.faces, n)
        roots = torch.nonzero(torch.bincount(label, minlength=n) >= min_edge).view(-1).cpu().numpy()
        label = label.cpu().numpy()
        return [mesh.copy().update_vertices(label == c) for c in roots]
    if backend != "scipy":
        raise ValueError(f"trimesh_split: backend must be 'scipy' or 'hip', got {backend!r}")
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(mesh.vertices)
    e = mesh.edges
    _, label = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    out = []
    for c in np.flatnonzero(np.bincount(label) >= min_edge):
        out.append(mesh.copy().update_vertices(label == c))
    return out


def largest_component(mesh, min_edge=100, backend="scipy"):
    """bundlesdf.py:748-759: merge vertices, split, keep the component with the
    most vertices (None when every component is below `min_edge`). backend as
    trimesh_split's."""
    if backend not in ("scipy", "hip"):
        raise ValueError(f"largest_component: backend must be 'scipy' or 'hip', got {backend!r}")
    mesh.merge_vertices()
    parts = trimesh_split(mesh, min_edge=min_edge, backend=backend)
    return max(parts, key=lambda m: len(m.vertices)) if parts else None


def mesh_to_real_world(mesh, pose_offset, translation, sc_factor):
    """Utils.py:508-514: normalised space -> object frame in metres."""
    mesh.vertices = mesh.vertices / sc_factor - np.asarray(translation, np.float64).reshape(1, 3)
    mesh.apply_transform(pose_offset)
    return mesh


def trimesh_clean(mesh):
    """Utils.py:278-284 (trimesh_clean) with what Mesh has: weld, drop faces that repeat a vertex index,
    drop duplicate faces, drop vertices no face uses. In place; returns the mesh."""
    mesh.merge_vertices()
    f = mesh.faces
    mesh.faces = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    mesh.remove_duplicate_faces()
    used = np.zeros(len(mesh.vertices), bool)
    used[mesh.faces.reshape(-1)] = True
    return mesh.update_vertices(used)


_VOLUME_ERROR = "volume_constraint needs a closed, outward-oriented mesh"


def _check_backend(what, backend):
    if backend not in ("scipy", "hip"):
        raise ValueError(f"{what}: backend must be 'scipy' or 'hip', got {backend!r}")


def _checked_faces(what, faces, n_vertices, device):
    """faces as an int64 [F,3] tensor on `device`; ValueError for a corner outside [0, n_vertices)."""
    f = as_tensor(faces, np.int64).to(device=device, dtype=torch.int64).reshape(-1, 3)
    n = int(n_vertices)
    if n < 0 or n * 3 >= 1 << 31 or len(f) * 3 >= 1 << 31:
        raise ValueError(f"{what}: {n} vertices, {len(f)} faces: both times 3 must be below 2^31")
    if len(f) and (int(f.min()) < 0 or int(f.max()) >= n):
        raise ValueError(f"{what}: face corners must be in [0, {n})")
    return f


def _csr(rows, vals, n_rows, n_vals):
    """CSR (row_start [n_rows+1] int32, cols int32) of the distinct (row, val) pairs, vals ascending
    within a row: one sort of the keys row * n_vals + val and unique_consecutive, on the pairs' device."""
    key = torch.unique_consecutive(torch.sort(rows * max(int(n_vals), 1) + vals).values)
    r = torch.div(key, max(int(n_vals), 1), rounding_mode="floor")
    row_start = torch.zeros(int(n_rows) + 1, dtype=torch.int64, device=key.device)
    row_start[1:] = torch.cumsum(torch.bincount(r, minlength=int(n_rows)), 0)
    return row_start.to(torch.int32), (key - r * max(int(n_vals), 1)).to(torch.int32)


def vertex_adjacency(faces, n_vertices, device=None):
    """(row_start [V+1], cols [E]) int32 tensors on `device` (default: the faces' device when they are a
    device tensor, else the current HIP device): row v holds the distinct vertices that share a face
    edge with v, ascending. An edge shared by several faces counts once; the self-edge of a degenerate
    face (a, a, b) is dropped; a corner outside [0, n_vertices) raises ValueError."""
    f = _checked_faces("vertex_adjacency", faces, n_vertices, default_device(faces, device))
    a = torch.cat([f[:, [0, 1, 2]].reshape(-1), f[:, [1, 2, 0]].reshape(-1)])   # every face edge, both directions
    b = torch.cat([f[:, [1, 2, 0]].reshape(-1), f[:, [0, 1, 2]].reshape(-1)])
    keep = a != b
    return _csr(a[keep], b[keep], n_vertices, n_vertices)


def vertex_faces(faces, n_vertices, device=None):
    """The vertex -> face CSR (row_start [V+1], face_ids) int32 on `device`, by vertex_adjacency's routine
    keyed (vertex, face): the faces of v, each once, in ascending face index."""
    f = _checked_faces("vertex_faces", faces, n_vertices, default_device(faces, device))
    ids = torch.arange(len(f), dtype=torch.int64, device=f.device)[:, None].expand(-1, 3).reshape(-1)
    return _csr(f.reshape(-1), ids, n_vertices, len(f))


def _volume_host(vertices, faces):
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    return float(np.sum(np.sum(t[:, 0] * np.cross(t[:, 1], t[:, 2]).reshape(-1, 3), axis=1)) / 6.0)


def mesh_volume(mesh_or_vertices, faces=None, backend="hip"):
    """Signed volume sum_f v0 . (v1 x v2) / 6 of a triangle mesh (a Mesh, or vertices with faces), as a
    float: positive for a closed mesh whose faces are oriented outwards. backend "hip":
    nof_mesh_volume (f64, per-block partial sums added in block order: the same bits on every run);
    "scipy": numpy on the host."""
    _check_backend("mesh_volume", backend)
    if faces is None:
        mesh_or_vertices, faces = mesh_or_vertices.vertices, mesh_or_vertices.faces
    vertices = np.array(mesh_or_vertices, np.float64).reshape(-1, 3)
    if backend == "scipy":
        f = _checked_faces("mesh_volume", faces, len(vertices), torch.device("cpu")).numpy()
        return _volume_host(vertices, f)
    from . import _lib
    dev = default_device()
    f = _checked_faces("mesh_volume", faces, len(vertices), dev).to(torch.int32).contiguous()
    v = torch.from_numpy(vertices).to(dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(L.nof_mesh_volume_workspace_bytes(len(f))), dtype=torch.uint8, device=dev)
        _lib.check(L.nof_mesh_volume(_lib.ptr(v), _lib.ptr(f), len(f), _lib.ptr(out), _lib.ptr(ws), _lib.stream_of(v)),
                   "mesh_volume")
    return float(out.item())


def _smooth_hip(vertices, faces, factors, volume_constraint):
    """The filter loop on the device, all of it enqueued on one stream: per factor one
    nof_mesh_laplacian_step, with the constraint followed by nof_mesh_volume and nof_mesh_scale_to_volume
    towards the initial volume. One host read at the end: the vertices with the initial volume and the flag."""
    from . import _lib
    dev = default_device()
    V = len(vertices)
    f = _checked_faces("filter", faces, V, dev)
    row_start, cols = vertex_adjacency(f, V, device=dev)
    f32 = f.to(torch.int32).contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        a = as_tensor(vertices, np.float64).to(dev)
        b = torch.empty_like(a)
        vol0, vol = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.nof_mesh_volume_workspace_bytes(len(f32))), dtype=torch.uint8, device=dev)
        st = _lib.stream_of(a)
        if volume_constraint:
            _lib.check(L.nof_mesh_volume(_lib.ptr(a), _lib.ptr(f32), len(f32), _lib.ptr(vol0), _lib.ptr(ws), st),
                       "mesh_volume")
        for factor in factors:
            _lib.check(L.nof_mesh_laplacian_step(_lib.ptr(a), _lib.ptr(row_start), _lib.ptr(cols), V, float(factor),
                                                 _lib.ptr(b), st), "mesh_laplacian_step")
            a, b = b, a
            if volume_constraint:
                _lib.check(L.nof_mesh_volume(_lib.ptr(a), _lib.ptr(f32), len(f32), _lib.ptr(vol), _lib.ptr(ws), st),
                           "mesh_volume")
                _lib.check(L.nof_mesh_scale_to_volume(_lib.ptr(a), V, _lib.ptr(vol0), _lib.ptr(vol), _lib.ptr(flag),
                                                      st), "mesh_scale_to_volume")
        out = torch.cat([a.reshape(-1), vol0, flag.double()]).cpu().numpy()
    if volume_constraint and (out[-1] != 0 or not out[-2] > 0):
        raise ValueError(_VOLUME_ERROR)
    return out[:-2].reshape(V, 3)


def _smooth_host(vertices, faces, factors, volume_constraint):
    """The same definition on the host: a scipy.sparse CSR operator with 1 / degree in every stored entry
    of the same adjacency (a row product adds its entries in stored order), volume by numpy."""
    from scipy.sparse import csr_matrix
    V = len(vertices)
    f = _checked_faces("filter", faces, V, torch.device("cpu"))
    row_start, cols = (t.numpy() for t in vertex_adjacency(f, V, device="cpu"))
    f = f.numpy()
    deg = np.diff(row_start)
    w = np.repeat(1.0 / np.maximum(deg, 1), deg)
    op = csr_matrix((w, cols, row_start), shape=(V, V))
    isolated = (deg == 0)[:, None]
    v = np.array(vertices, np.float64)
    vol0 = _volume_host(v, f) if volume_constraint else 0.0
    if volume_constraint and not vol0 > 0:
        raise ValueError(_VOLUME_ERROR)
    for factor in factors:
        v = np.where(isolated, v, v + float(factor) * (op @ v - v))
        if volume_constraint:
            r = vol0 / _volume_host(v, f)
            if not (r > 0 and np.isfinite(r)):
                raise ValueError(_VOLUME_ERROR)
            v = v * np.cbrt(r)
    return v


def _smooth(what, mesh, factors, volume_constraint, backend):
    _check_backend(what, backend)
    if not all(np.isfinite(x) for x in factors):
        raise ValueError(f"{what}: lamb / nu must be finite")
    if not factors or len(mesh.vertices) == 0:
        return mesh
    run = _smooth_hip if backend == "hip" else _smooth_host
    mesh.vertices = run(mesh.vertices, mesh.faces, factors, volume_constraint)   # raises before assigning
    mesh.vertex_normals = None      # they described the old surface
    return mesh


def filter_laplacian(mesh, lamb=0.5, iterations=10, volume_constraint=True, backend="hip"):
    """trimesh.smoothing.filter_laplacian(mesh, lamb, iterations, implicit_time_integration=False,
    volume_constraint) with the default (uniform-weight) operator. Per iteration every vertex moves by
    lamb of the way to the mean of its neighbours (vertex_adjacency), all vertices at once:
    v + lamb (m - v), m = ((w v[j0] + w v[j1]) + ...), w = 1 / degree; a vertex without neighbours stays
    (trimesh pulls it towards the origin). With volume_constraint each iteration is followed by a
    rescale about the origin by cbrt(initial volume / volume); a mesh whose initial volume is not
    positive, or whose volume stops being so, raises ValueError and is left untouched. In place:
    vertices change, vertex_normals become None, faces and the other attributes stay. iterations == 0
    is the identity. backend "hip": the device loop of _smooth_hip (nof_mesh_laplacian_step, nof_mesh_volume,
    nof_mesh_scale_to_volume; one host read); "scipy": the same definition on the host."""
    return _smooth("filter_laplacian", mesh, [float(lamb)] * int(iterations), volume_constraint, backend)


def filter_taubin(mesh, lamb=0.5, nu=0.5, iterations=10, backend="hip"):
    """Taubin's filter with trimesh.smoothing.filter_taubin's signature and defaults: filter_laplacian's
    step with factor lamb in iteration k = 0, 2, 4, ... and factor -nu in k = 1, 3, 5, ... (the shrinking
    step and the inflating step alternate), no volume constraint. This is the definition here; parity
    with trimesh is not pinned by a test. In place, as filter_laplacian."""
    factors = [float(lamb) if k % 2 == 0 else -float(nu) for k in range(int(iterations))]
    return _smooth("filter_taubin", mesh, factors, False, backend)


def postprocess_mesh(mesh, translation, sc_factor, out_dir=None, min_edge=1000, lamb=0.5, iterations=3, backend="hip"):
    """run_custom.py:158-188 for a normalised-space Mesh -> {"real_scale", "biggest_component", "smoothed"}.

    On a copy: vertices / sc_factor - translation (the inverse of the normalisation); trimesh_split(min_edge,
    backend) and the component with the most vertices (ValueError when there is none); trimesh_clean;
    filter_laplacian(lamb, iterations, volume_constraint=True, backend) on a copy of that, then
    compute_vertex_normals(backend). With out_dir the three meshes are also written there under the
    reference's names: mesh_real_scale.obj, mesh_biggest_component.obj, mesh_biggest_component_smoothed.obj."""
    _check_backend("postprocess_mesh", backend)
    real = mesh.copy()
    real.vertices = real.vertices / sc_factor - np.asarray(translation, np.float64).reshape(1, 3)
    parts = trimesh_split(real, min_edge=min_edge, backend=backend)
    if not parts:
        raise ValueError(f"postprocess_mesh: no component with at least {min_edge} vertices")
    biggest = trimesh_clean(max(parts, key=lambda m: len(m.vertices)))
    smoothed = filter_laplacian(biggest.copy(), lamb=lamb, iterations=iterations, volume_constraint=True,
                                backend=backend)
    smoothed.compute_vertex_normals(backend=backend)
    out = {"real_scale": real, "biggest_component": biggest, "smoothed": smoothed}
    if out_dir is not None:
        import os
        os.makedirs(out_dir, exist_ok=True)
        for key, name in (("real_scale", "mesh_real_scale.obj"), ("biggest_component", "mesh_biggest_component.obj"),
                          ("smoothed", "mesh_biggest_component_smoothed.obj")):
            out[key].export(os.path.join(out_dir, name))
    return out
