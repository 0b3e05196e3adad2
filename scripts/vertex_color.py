"""Time one frame of NerfRunner.mesh_vertex_color_from_train_images both ways, in one process, on the
synthetic scene after --steps training steps and extract_mesh at the default voxel size (640x480 frames):

  device  nof_raster_faces + nof_vertex_color_accumulate (one lane per vertex) with the frame's mask
          and image already in HBM, by HIP events: warm-up, then --reps timed passes over the sequence's
          frames, the median per frame;
  cpu     the reference's lines on the same z-buffer: back-project the valid pixels (numpy),
          cKDTree(points).query(vertices, workers=16), wall clock, the median per frame.

Also the mean search-window area (pixels per vertex, from the kernel's bound restated in numpy) and the
share of vertices coloured. Writes profiles/r10/vertex_color.json. No threshold is asserted.
Usage: python scripts/vertex_color.py [--frames 8] [--steps 300] [--reps 10] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_area(V, ob_in_cam, K, H, W, radius, min_depth):
    """Pixels in every vertex's search window (0 where it is empty): k_vertex_color's bound."""
    X = V.astype(np.float64) @ ob_in_cam[:3, :3].T + ob_in_cam[:3, 3]
    z0, z1 = np.maximum(X[:, 2] - radius, min_depth), X[:, 2] + radius

    def span(f, c, x, n):
        v = np.stack([f * a / z + c for a in (x - radius, x + radius) for z in (z0, z1)])
        lo, hi = np.maximum(np.floor(v.min(0)) - 1, 0), np.minimum(np.ceil(v.max(0)) + 1, n - 1)
        return np.where(lo <= hi, hi - lo + 1, 0)
    with np.errstate(all="ignore"):
        return np.where(z0 <= z1, span(K[0, 0], K[0, 2], X[:, 0], W) * span(K[1, 1], K[1, 2], X[:, 1], H), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "vertex_color.json"))
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    from bundlesdf_amd import _lib
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    from bundlesdf_amd.texture import _cvcam_in_obs
    seq = SY.make_sequence(a.frames, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=a.steps, N_rand=2048,
                         num_levels=16, amp=True)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = nr.extract_mesh()
    dev, L = nr.device, _lib.lib()
    sc, H, W = cfg["sc_factor"], nr.H, nr.W
    min_depth, zfar, radius = 0.1 * sc, cfg["far"] * sc, 0.002 * sc
    K = np.ascontiguousarray(nr.K, np.float64)
    Vh = np.asarray(mesh.vertices, np.float32)
    V = torch.as_tensor(Vh, device=dev)
    Fc = torch.as_tensor(np.asarray(mesh.faces, np.int64), device=dev)
    nV = len(V)
    cams = [np.ascontiguousarray(c, np.float64) for c in _cvcam_in_obs(nr)]
    invs = [np.ascontiguousarray(np.linalg.inv(c)) for c in cams]
    masks = [torch.as_tensor(np.asarray(m).reshape(H, W).astype(bool).astype(np.uint8), device=dev) for m in nr.masks]
    imgs = [torch.as_tensor(np.asarray(im, np.float32).reshape(H * W, 3), device=dev) for im in nr.images]
    zbuf = torch.empty(H * W, dtype=torch.int64, device=dev)
    csum = torch.zeros((nV, 3), dtype=torch.float64, device=dev)
    cnt = torch.zeros(nV, dtype=torch.int32, device=dev)
    st = _lib.stream_of(V)

    def frame(i):
        _lib.check(L.nof_raster_faces(_lib.ptr(V), _lib.ptr(Fc), len(Fc), invs[i].ctypes.data_as(_lib._p),
                                      K.ctypes.data_as(_lib._p), H, W, 0.1, zfar, _lib.ptr(zbuf), st), "raster_faces")
        _lib.check(L.nof_vertex_color_accumulate(_lib.ptr(zbuf), H, W, _lib.ptr(masks[i]), min_depth, _lib.ptr(imgs[i]),
                                                 cams[i].ctypes.data_as(_lib._p), invs[i].ctypes.data_as(_lib._p),
                                                 K.ctypes.data_as(_lib._p), _lib.ptr(V), nV, radius, _lib.ptr(csum),
                                                 _lib.ptr(cnt), None, None, st), "vertex_color_accumulate")

    for i in range(a.frames):      # warm-up, and the counts of one pass
        frame(i)
    torch.cuda.synchronize()
    coloured = float((cnt > 0).float().mean())
    dev_ms = []
    for _ in range(a.reps):
        for i in range(a.frames):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            frame(i)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
    cpu_ms, areas, cands = [], [], []
    for i in range(a.frames):
        _lib.check(L.nof_raster_faces(_lib.ptr(V), _lib.ptr(Fc), len(Fc), invs[i].ctypes.data_as(_lib._p),
                                      K.ctypes.data_as(_lib._p), H, W, 0.1, zfar, _lib.ptr(zbuf), st), "raster_faces")
        zb = zbuf.cpu().numpy().view(np.uint64)
        m = masks[i].cpu().numpy().reshape(-1)
        t0 = time.perf_counter()
        z = (zb >> np.uint64(32)).astype(np.uint32).view(np.float32)
        with np.errstate(invalid="ignore"):
            idx = np.nonzero((zb != np.iinfo(np.uint64).max) & (m != 0) & (z >= np.float32(min_depth)))[0]
        zd = z[idx].astype(np.float64)
        py, px = np.divmod(idx, W)
        pc = np.stack([((px - K[0, 2]) * zd / K[0, 0]).astype(np.float32), ((py - K[1, 2]) * zd / K[1, 1]).astype(np.float32),
                       zd], -1).astype(np.float64)
        pts = pc @ cams[i][:3, :3].T + cams[i][:3, 3]
        if len(pts):
            cKDTree(pts).query(Vh.astype(np.float64), workers=16)
        cpu_ms.append((time.perf_counter() - t0) * 1e3)
        cands.append(len(idx))
        areas.append(float(window_area(Vh, invs[i], K, H, W, radius, min_depth).mean()))
    out = {"vertices": nV, "faces": int(len(Fc)), "frames": a.frames, "H": H, "W": W, "steps": a.steps, "reps": a.reps,
           "mapping": "one lane per vertex", "device": torch.cuda.get_device_name(0),
           "device_ms_per_frame": round(float(np.median(dev_ms)), 4),
           "device_ms_per_frame_min_max": [round(float(np.min(dev_ms)), 4), round(float(np.max(dev_ms)), 4)],
           "cpu_ms_per_frame": round(float(np.median(cpu_ms)), 3),
           "cpu_ms_per_frame_min_max": [round(float(np.min(cpu_ms)), 3), round(float(np.max(cpu_ms)), 3)],
           "cpu_workers": 16, "candidates_per_frame_mean": float(np.mean(cands)),
           "window_area_mean_px": round(float(np.mean(areas)), 2), "coloured_share": round(coloured, 4)}
    out["cpu_over_device"] = round(out["cpu_ms_per_frame"] / out["device_ms_per_frame"], 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
