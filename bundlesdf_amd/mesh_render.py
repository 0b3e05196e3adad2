"""Mesh render on the device: depth, face id, colour and normal images of a Mesh at any number of
poses in one call (nof_render_mesh, csrc/mesh_render.hip), the counterpart of the reference's
pyrender pass (offscreen_renderer.py: ModelRendererOffscreen).

Poses are ob-in-OpenCV-camera matrices (x right, y down, z forward), pixel centres sit at integer
(u, v), and the z-buffer is nof_raster_faces' bit for bit: faces with a vertex at z <= znear are
dropped (no near-plane clipping), edges are inclusive, either winding is drawn, ties in depth go to
the lower face index. The reference lights with full ambient, so colours are unlit unless
shade=True asks for a headlight.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._args import default_device

# Faces whose clamped screen bounding box holds at most this many pixels are rasterised by their own
# lane; larger ones by a wave each. Chosen from scripts/render_mesh.py's table on one MI355X
# (profiles/r14/render_mesh.json, 64 poses at 640x480): the dense mesh takes the same time from 64
# up (0.57-0.58 ms; 0.84 ms at 16, 2.8 ms at 0) and the screen-filling box from 0 to 1024 (2.2 ms;
# 3.7 ms at 4096, 99.5 ms with every face on one lane). 256 lies inside both plateaus. The images
# do not depend on it.
SMALL_MAX_PIXELS = 256

FLAT_RGB = (200, 200, 200)
_MODES = {"flat": _lib.MESH_COLOUR_FLAT, "vertex": _lib.MESH_COLOUR_VERTEX, "texture": _lib.MESH_COLOUR_TEXTURE}


class MeshRenderer:
    """A mesh uploaded once: vertices (float32), faces, and what it carries of vertex_colors,
    vertex_normals, uv and texture. K [3,3], H, W: the camera; znear, zfar in the mesh's units."""

    def __init__(self, mesh, K, H, W, znear=0.1, zfar=2.0, device=None):
        from .mesh import _checked_faces
        dev = default_device(device=device)
        self.device = dev
        self.H, self.W, self.znear, self.zfar = int(H), int(W), float(znear), float(zfar)
        self.K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        v = np.asarray(mesh.vertices, np.float32).reshape(-1, 3)
        n = len(v)
        self.V = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        self.F = _checked_faces("MeshRenderer", mesh.faces, n, dev).contiguous()

        def per_vertex(a, dtype, cols, name):
            if a is None:
                return None
            a = np.asarray(a)
            if a.shape != (n, cols):
                raise ValueError(f"MeshRenderer: {name} must be [{n},{cols}], got {a.shape}")
            return torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).to(dev)

        self.colors = per_vertex(mesh.vertex_colors, np.uint8, 3, "vertex_colors")
        self.normals = per_vertex(mesh.vertex_normals, np.float32, 3, "vertex_normals")
        self.uv = self.texture = None
        if mesh.uv is not None and mesh.texture is not None:
            self.uv = per_vertex(mesh.uv, np.float32, 2, "uv")
            tex = np.asarray(mesh.texture)
            if tex.ndim != 3 or tex.shape[2] != 3 or tex.shape[0] < 1 or tex.shape[1] < 1:
                raise ValueError(f"MeshRenderer: texture must be [TH,TW,3], got {tex.shape}")
            self.texture = torch.from_numpy(np.ascontiguousarray(tex.astype(np.uint8))).to(dev)

    def _mode(self, colour):
        if colour == "auto":
            colour = "texture" if self.texture is not None else "vertex" if self.colors is not None else "flat"
        if colour not in _MODES:
            raise ValueError(f"MeshRenderer.render: colour must be 'auto', 'texture', 'vertex' or 'flat', got {colour!r}")
        if colour == "texture" and self.texture is None:
            raise ValueError("MeshRenderer.render: colour 'texture' needs a mesh with uv and texture")
        if colour == "vertex" and self.colors is None:
            raise ValueError("MeshRenderer.render: colour 'vertex' needs a mesh with vertex_colors")
        return _MODES[colour]

    def render(self, ob_in_cams, colour="auto", shade=False, small_max_pixels=None, flat_rgb=FLAT_RGB):
        """ob_in_cams [4,4] or [B,4,4] (numpy or tensor) -> {"depth" float32 [B,H,W] (0 on a miss), "face"
        int32 [B,H,W] (-1 on a miss), "mask" bool [B,H,W], "rgb" uint8 [B,H,W,3], "normal" float32
        [B,H,W,3] (unit, camera frame, towards the camera)}: device tensors, without the leading B
        for a single [4,4] pose. Nothing is read back; the call is enqueued on the current stream."""
        mode = self._mode(colour)
        dev = self.device
        T = torch.as_tensor(ob_in_cams)
        single = T.dim() == 2
        T = T.to(device=dev, dtype=torch.float64).reshape(-1, 4, 4).contiguous()
        if single and len(T) != 1:
            raise ValueError("MeshRenderer.render: ob_in_cams must be [4,4] or [B,4,4]")
        B, H, W = len(T), self.H, self.W
        smp = SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
        L = _lib.lib()
        d = _lib.MeshRenderDesc()
        d.vertices, d.faces, d.n_vertices, d.n_faces = _lib.ptr(self.V), _lib.ptr(self.F), len(self.V), len(self.F)
        d.colors, d.normals, d.uv, d.texture = (_lib.ptr(self.colors), _lib.ptr(self.normals), _lib.ptr(self.uv),
                                                _lib.ptr(self.texture))
        if self.texture is not None:
            d.tex_h, d.tex_w = int(self.texture.shape[0]), int(self.texture.shape[1])
        d.ob_in_cam, d.K = _lib.ptr(T), self.K.ctypes.data_as(_lib._p)
        d.B, d.H, d.W, d.znear, d.zfar = B, H, W, self.znear, self.zfar
        d.colour_mode, d.shade, d.small_max_pixels = mode, int(bool(shade)), smp
        d.base_rgb = (ctypes.c_uint8 * 4)(int(flat_rgb[0]), int(flat_rgb[1]), int(flat_rgb[2]), 0)
        with torch.cuda.device(dev):
            ws = torch.empty(max(int(L.nof_render_mesh_workspace_bytes(B, len(self.F), H, W)), 1), dtype=torch.uint8,
                             device=dev)
            out = {"depth": torch.empty((B, H, W), dtype=torch.float32, device=dev),
                   "face": torch.empty((B, H, W), dtype=torch.int32, device=dev),
                   "rgb": torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev),
                   "normal": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)}
            d.workspace = _lib.ptr(ws)
            d.depth, d.face, d.rgb, d.normal = (_lib.ptr(out[k]) for k in ("depth", "face", "rgb", "normal"))
            _lib.check(L.nof_render_mesh(ctypes.byref(d), _lib.stream_of(self.V)), "render_mesh")
        out["mask"] = out["face"] >= 0
        return {k: v[0] for k, v in out.items()} if single else out


def render_mesh(mesh, ob_in_cams, K, H, W, znear=0.1, zfar=2.0, device=None, **kw):
    """MeshRenderer(mesh, K, H, W, znear, zfar, device).render(ob_in_cams, **kw) in one call."""
    return MeshRenderer(mesh, K, H, W, znear=znear, zfar=zfar, device=device).render(ob_in_cams, **kw)
