"""Time the two searches of the run evaluation both ways, in one process, on the synthetic scene's mesh
after --steps training steps:

  ADD-S     evaluate.adi_err over --pose-frames perturbed poses of the mesh's vertices (one grid, one
            nof_nearest_points launch for all frames) against the reference's route, a scipy cKDTree
            per frame over the predicted-pose cloud queried with workers=16. The cKDTree route is timed
            on the first --baseline-frames frames only and reported per frame, as is the device route;
  chamfer   evaluate.chamfer_distance_between_clouds_mutual of two surface samples of --chamfer-points
            points each against two cKDTrees (workers=16).

Both routes start from host numpy arrays and end with the result on the host; a host clock spans each
call, warm-up passes first, then the median and the min / max of --reps passes, each pass repeating the
call until it spans at least 0.2 s (times are per call). The two routes' results are compared. Writes profiles/r12/evaluate.json. No threshold is asserted.
Usage: python scripts/evaluate.py [--frames 8] [--steps 300] [--reps 7] [--voxel 0.003] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKERS = 16
MIN_WINDOW_S = 0.2


def timed(fn, reps, warm=2):
    for _ in range(warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        once = time.perf_counter() - t0
    inner = max(1, int(np.ceil(MIN_WINDOW_S / max(once, 1e-6))))    # calls per timed pass: a pass spans >= 0.2 s
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return out, {"ms": round(float(np.median(ms)), 3), "ms_min_max": [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)],
                 "reps": reps, "calls_per_rep": inner}


def small_rigid(rng, rot_sd, trans_sd):
    r = rng.normal(0, rot_sd, 3)
    th = np.linalg.norm(r)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = rng.normal(0, trans_sd, 3)
    return T


def adds_ckdtree(pred, gt, model):
    from scipy.spatial import cKDTree
    out = np.empty(len(pred))
    for f in range(len(pred)):
        p = model @ pred[f, :3, :3].T + pred[f, :3, 3]
        g = model @ gt[f, :3, :3].T + gt[f, :3, 3]
        out[f] = cKDTree(p).query(g, k=1, workers=WORKERS)[0].mean()
    return out


def chamfer_ckdtree(a, b):
    from scipy.spatial import cKDTree
    d1 = cKDTree(a).query(b, workers=WORKERS)[0]
    d2 = cKDTree(b).query(a, workers=WORKERS)[0]
    return 0.5 * (d1.mean() + d2.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=0.003)
    ap.add_argument("--pose-frames", type=int, default=1000)
    ap.add_argument("--baseline-frames", type=int, default=50)
    ap.add_argument("--chamfer-points", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "evaluate.json"))
    a = ap.parse_args()
    from bundlesdf_amd import evaluate as E
    from bundlesdf_amd import mesh as M
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(a.frames, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=a.steps, N_rand=2048,
                         num_levels=16, amp=True)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = nr.extract_mesh(voxel_size=a.voxel, mesher="hip")
    mesh = M.largest_component(M.mesh_to_real_world(mesh, np.eye(4), cfg["translation"], cfg["sc_factor"]),
                               backend="hip")      # normalised space -> metres
    model = np.ascontiguousarray(mesh.vertices)

    rng = np.random.default_rng(0)
    F = a.pose_frames
    gt = np.stack([small_rigid(rng, 1.0, 0.3) for _ in range(F)])
    pred = np.stack([g @ small_rigid(rng, 0.05, 0.01) for g in gt])
    Fb = min(a.baseline_frames, F)
    adds_dev, t_dev = timed(lambda: E.adi_err(pred, gt, model), a.reps)
    adds_ref, t_ref = timed(lambda: adds_ckdtree(pred[:Fb], gt[:Fb], model), max(3, a.reps // 2), warm=1)
    pts1 = E.sample_surface(mesh, a.chamfer_points, seed=1)[0].cpu().numpy()
    pts2 = E.sample_surface(mesh, a.chamfer_points, seed=2)[0].cpu().numpy() + rng.normal(0, 5e-4, (a.chamfer_points, 3))
    cd_dev, t_cd_dev = timed(lambda: E.chamfer_distance_between_clouds_mutual(pts1, pts2), a.reps)
    cd_ref, t_cd_ref = timed(lambda: chamfer_ckdtree(pts1, pts2), a.reps)

    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "frames": a.frames, "voxel_size": a.voxel,
           "model_points": int(len(model)), "pose_frames": F, "baseline_frames": Fb, "ckdtree_workers": WORKERS,
           "adds_device": t_dev, "adds_device_ms_per_frame": round(t_dev["ms"] / F, 4),
           "adds_ckdtree": t_ref, "adds_ckdtree_ms_per_frame": round(t_ref["ms"] / Fb, 4),
           "adds_max_abs_difference_m": float(np.abs(adds_dev[:Fb] - adds_ref).max()),
           "adds_mean_cm": float(adds_dev.mean() * 100), "adds_auc_percent": float(E.compute_auc(adds_dev) * 100),
           "chamfer_points": a.chamfer_points, "chamfer_device": t_cd_dev, "chamfer_ckdtree": t_cd_ref,
           "chamfer_cm": float(cd_dev * 100), "chamfer_relative_difference": float(abs(cd_dev - cd_ref) / cd_ref)}
    out["adds_ckdtree_over_device_per_frame"] = round(out["adds_ckdtree_ms_per_frame"] / out["adds_device_ms_per_frame"], 2)
    out["chamfer_ckdtree_over_device"] = round(t_cd_ref["ms"] / t_cd_dev["ms"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
