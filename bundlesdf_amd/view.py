"""Free-camera rays: the host-side statement of step 1 of the surface render (nof_render_view).

The convention is the ray pool's: GL camera frame, direction columns 0-2 of a pool row are
((u - cx) / fx, -((v - cy) / fy), -1) with the intrinsics rounded to float32 (ray_pool.hip
camera_dir), c2w is a camera-to-world matrix in normalised space (NerfRunner.poses), and the trace
takes the unit direction rotated to the world (k_trace). Every operation is a float32 torch
operation rounded on its own, in the kernel's order, so the values are the kernel's bit for bit.
"""
import numpy as np
import torch


def pixel_indices(H, W, pixels=None):
    """Row-major pixel indices (v * W + u) as an int64 tensor: every pixel of the image, or `pixels`
    given as indices [n] or (u, v) pairs [n,2]."""
    if pixels is None:
        return torch.arange(int(H) * int(W), dtype=torch.int64)
    p = torch.as_tensor(np.asarray(pixels.cpu() if torch.is_tensor(pixels) else pixels)).to(torch.int64)
    if p.ndim == 2 and p.shape[1] == 2:
        if ((p[:, 0] < 0) | (p[:, 0] >= W) | (p[:, 1] < 0) | (p[:, 1] >= H)).any():
            raise ValueError(f"view: a (u, v) pixel lies outside the {W}x{H} image")
        p = p[:, 1] * int(W) + p[:, 0]
    p = p.reshape(-1)
    if p.numel() and (int(p.min()) < 0 or int(p.max()) >= int(H) * int(W)):
        raise ValueError(f"view: a pixel index lies outside the {W}x{H} image")
    return p


def view_rays(c2w, K, H, W, pixels=None):
    """The rays of a camera: {"pixels" [n] int64, "dir_cam" [n,3] (as the pool stores it), "origin" [3],
    "dir" [n,3] (unit, world), "vz" [n] = |v^_z| (depth = t * vz)}, float32 CPU tensors."""
    f = np.float32
    T = np.asarray(c2w, np.float64).astype(f).reshape(4, 4)
    k32 = np.asarray(K, np.float64).astype(f)
    fx, fy, cx, cy = k32[0, 0], k32[1, 1], k32[0, 2], k32[1, 2]
    pix = pixel_indices(H, W, pixels)
    p = pix.numpy()
    u, v = (p % int(W)).astype(f), (p // int(W)).astype(f)
    dc = np.stack([(u - cx) / fx, -((v - cy) / fy), np.full_like(u, -1.0)], -1)
    nrm = np.sqrt((dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1]) + dc[:, 2] * dc[:, 2])
    vd = dc / nrm[:, None]
    d = np.stack([(T[i, 0] * vd[:, 0] + T[i, 1] * vd[:, 1]) + T[i, 2] * vd[:, 2] for i in range(3)], -1)
    assert dc.dtype == d.dtype == np.float32
    return {"pixels": pix, "dir_cam": torch.from_numpy(dc), "origin": torch.from_numpy(T[:3, 3].copy()),
            "dir": torch.from_numpy(d), "vz": torch.from_numpy(np.abs(vd[:, 2]))}
