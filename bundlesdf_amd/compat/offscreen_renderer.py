"""`from offscreen_renderer import ModelRendererOffscreen` shim (nerf_runner.py:1435): ModelRendererOffscreen on bundlesdf_amd.mesh_render in
place of pyrender (offscreen_renderer.py). Meshes are bundlesdf_amd.mesh.Mesh objects (model_paths
are read with Mesh.load); colours are unlit, as the reference's full ambient light leaves them."""
import numpy as np
import torch

from bundlesdf_amd.mesh import Mesh
from bundlesdf_amd.mesh_render import MeshRenderer

__all__ = ["ModelRendererOffscreen"]


class ModelRendererOffscreen:
    def __init__(self, model_paths, cam_K, H, W, zfar=2, device=None):
        self.K = np.asarray(cam_K, np.float64)
        self.H, self.W, self.zfar, self.device = int(H), int(W), float(zfar), device
        self.mesh_nodes = []
        for path in model_paths:
            self.add_mesh(Mesh.load(path))

    def clear_meshes(self):
        self.mesh_nodes = []

    def add_mesh(self, mesh):
        self.mesh_nodes.append(MeshRenderer(mesh, self.K, self.H, self.W, znear=0.1, zfar=self.zfar, device=self.device))

    def render(self, ob_in_cvcams):
        """One ob-in-OpenCV-camera pose per mesh, in the order the meshes were added -> (color uint8
        [H,W,3], depth float32 [H,W]); every mesh is drawn at its own pose and each pixel shows the
        nearest one (the first added on a tie), depth 0 and colour 0 where nothing is hit."""
        if len(ob_in_cvcams) != len(self.mesh_nodes):
            raise ValueError(f"ModelRendererOffscreen.render: {len(ob_in_cvcams)} poses for {len(self.mesh_nodes)} meshes")
        color = depth = None
        for node, pose in zip(self.mesh_nodes, ob_in_cvcams):
            r = node.render(np.asarray(pose, np.float64).reshape(4, 4))
            if depth is None:
                color, depth = r["rgb"], r["depth"]
                continue
            nearer = r["mask"] & ((depth == 0) | (r["depth"] < depth))
            depth = torch.where(nearer, r["depth"], depth)
            color = torch.where(nearer[..., None], r["rgb"], color)
        if depth is None:
            return np.zeros((self.H, self.W, 3), np.uint8), np.zeros((self.H, self.W), np.float32)
        return color.cpu().numpy(), depth.cpu().numpy()

    def renderBatch(self, ob_in_cvcams):
        """A list of render() arguments -> (colors [N,H,W,3], depths [N,H,W])."""
        out = [self.render(poses) for poses in ob_in_cvcams]
        return np.array([c for c, _ in out]), np.array([d for _, d in out])
