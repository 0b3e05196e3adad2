"""Turntable of the synthetic scene's mesh through the mesh render (bundlesdf_amd.mesh_render), and its
timing against the route the library offered before it: a loop of nof_raster_faces, one call per pose
(a z-buffer only: no image comes out of that route).

    python scripts/render_mesh.py --frames 8 --size 640x480

Trains the synthetic runner for --steps steps, extracts its mesh, gives it the network's vertex colours
and normals, writes --frames views around it to PNG (colour, normal as (n + 1) / 2, depth), then times
--poses poses at --size two ways (medians of --reps after warm-up, HIP events, host calls included):
one batched MeshRenderer.render call, and the nof_raster_faces loop. Once on the dense mesh and once on
a 12-face box that fills the screen, each for several small_max_pixels (the table the module's default
is chosen from). Figures go to --json; they are recorded, not asserted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = [0, 16, 64, 256, 1024, 4096, 1 << 30]


def rot_y(a):
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return R


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def box_mesh(h):
    from bundlesdf_amd.mesh import Mesh
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return Mesh(v, np.array(f, np.int64))


def time_mesh(mesh, poses, K, H, W, zfar, reps):
    """{"faces", "raster_loop_ms", "batched_ms": {threshold: ms}, "large_faces": {threshold: count}}."""
    from bundlesdf_amd import _lib
    from bundlesdf_amd.mesh_render import MeshRenderer
    r = MeshRenderer(mesh, K, H, W, znear=0.1, zfar=zfar)
    L = _lib.lib()
    Kd = np.ascontiguousarray(np.asarray(K, np.float64))
    host = [np.ascontiguousarray(T) for T in poses]
    zb = torch.empty(H * W, dtype=torch.int64, device=r.device)
    st = _lib.stream_of(zb)

    def loop():
        for T in host:
            _lib.check(L.nof_raster_faces(_lib.ptr(r.V), _lib.ptr(r.F), len(r.F), T.ctypes.data_as(_lib._p),
                                          Kd.ctypes.data_as(_lib._p), H, W, 0.1, float(zfar), _lib.ptr(zb), st),
                       "raster_faces")
    dev_poses = torch.as_tensor(poses, device=r.device)
    out = {"faces": int(len(r.F)), "poses": len(poses), "raster_loop_ms": median_ms(loop, reps), "batched_ms": {},
           "hit_share": float(r.render(dev_poses, colour="flat")["mask"].float().mean())}
    print(f"{out['faces']} faces: raster loop {out['raster_loop_ms']:.3f} ms", file=sys.stderr, flush=True)
    for t in THRESHOLDS:
        out["batched_ms"][str(t)] = median_ms(lambda: r.render(dev_poses, colour="flat", small_max_pixels=t), reps)
        print(f"  small_max_pixels {t}: {out['batched_ms'][str(t)]:.3f} ms", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--size", default="640x480", help="WxH of the rendered views")
    ap.add_argument("--steps", type=int, default=300, help="training steps before the mesh is extracted")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "turntable"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r14", "render_mesh.json"))
    args = ap.parse_args()
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.handoff import GLCAM_IN_CVCAM
    from bundlesdf_amd.mesh import write_png
    from bundlesdf_amd.mesh_render import SMALL_MAX_PIXELS, MeshRenderer
    from bundlesdf_amd.nerf_runner import NerfRunner
    W, H = (int(x) for x in args.size.lower().split("x"))
    seq = SY.make_sequence(3, seed=1)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=args.steps, N_rand=2048,
                         num_levels=16, amp=True)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = nr.extract_mesh()
    nr.mesh_vertex_color_from_network(mesh)
    nr.mesh_vertex_normals_from_network(mesh)
    K = np.asarray(nr.K, np.float64).copy()
    K[0] *= W / nr.W
    K[1] *= H / nr.H
    zfar = cfg["far"] * cfg["sc_factor"]
    cam_in_ob = np.asarray(nr.poses[1], np.float64) @ np.linalg.inv(GLCAM_IN_CVCAM)     # OpenCV camera in object

    def around(n):
        return np.stack([np.linalg.inv(rot_y(2 * np.pi * i / n) @ cam_in_ob) for i in range(n)])
    os.makedirs(args.out, exist_ok=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    r = MeshRenderer(mesh, K, H, W, znear=0.1, zfar=zfar)
    views = {k: v.cpu().numpy() for k, v in r.render(around(args.frames), colour="vertex", shade=True).items()}
    for i in range(args.frames):
        hit = views["mask"][i]
        far = views["depth"][i][hit].max() if hit.any() else 1.0
        depth = np.where(hit, 255 * (1 - 0.8 * views["depth"][i] / far), 0)
        write_png(os.path.join(args.out, f"mesh_{i:03d}_colour.png"), views["rgb"][i])
        write_png(os.path.join(args.out, f"mesh_{i:03d}_normal.png"),
                  (np.where(hit[..., None], (views["normal"][i] + 1) / 2, 0) * 255).astype(np.uint8))
        write_png(os.path.join(args.out, f"mesh_{i:03d}_depth.png"), np.repeat(depth[..., None], 3, -1).astype(np.uint8))
    # the box: half extent 0.3 with its centre 0.8 in front of the camera, turning about its own y axis
    box_poses = []
    for i in range(args.poses):
        T = rot_y(2 * np.pi * i / args.poses)
        T[:3, 3] = [0.0, 0.0, 0.8]
        box_poses.append(T)
    fig = {"size": [W, H], "train_steps": args.steps, "reps": args.reps, "default_small_max_pixels": SMALL_MAX_PIXELS,
           "thresholds": THRESHOLDS, "device": torch.cuda.get_device_name(0),
           "turntable_hit_share": [float(views["mask"][i].mean()) for i in range(args.frames)],
           "dense": time_mesh(mesh, around(args.poses), K, H, W, zfar, args.reps),
           "box": time_mesh(box_mesh(0.3), np.stack(box_poses), K, H, W, zfar, args.reps)}
    with open(args.json, "w") as f:
        json.dump(fig, f, indent=1)
    print(json.dumps(fig))


if __name__ == "__main__":
    main()
