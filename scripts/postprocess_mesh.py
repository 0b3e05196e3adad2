"""Time mesh post-processing both ways, in one process, on the synthetic scene's extracted mesh (obtained as
scripts/extract_mesh.py obtains it: --steps training steps, extract_mesh's dense SDF volume at the default
voxel size through NerfRunner.extract_mesh with the device mesher), in normalised space:

  postprocess_mesh   mesh.postprocess_mesh(mesh, translation, sc_factor, backend="hip") against backend="scipy":
                     real scale, trimesh_split, the biggest component, trimesh_clean, three constrained
                     Laplacian iterations, vertex normals — from the host Mesh to the three host meshes;
  filter_laplacian   mesh.filter_laplacian(iterations=3, volume_constraint=True) alone on the biggest
                     component, "hip" against "scipy", from the host Mesh to its new host vertices (the
                     adjacency build, the upload and the final read included);
  vertex normals     Mesh.compute_vertex_normals, "hip" against "scipy".

A host clock around each call, which starts from host arrays and ends on the host after a device
synchronise; warm-up, then the median of --reps passes, each pass repeating the call until --window seconds
have gone by. The two backends are also compared. Writes profiles/r13/postprocess_mesh.json. No threshold is
asserted.
Usage: python scripts/postprocess_mesh.py [--frames 8] [--steps 300] [--reps 7] [--window 0.2] [--voxel 0.003] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, window, warm=2):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            out = fn()
            torch.cuda.synchronize()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= window:
                break
        ms.append(dt / n * 1e3)
    return out, {"ms": round(float(np.median(ms)), 3), "ms_min_max": [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--voxel", type=float, default=0.003)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "postprocess_mesh.json"))
    a = ap.parse_args()
    from bundlesdf_amd import mesh as M
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(a.frames, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=a.steps, N_rand=2048,
                         num_levels=16, amp=True)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    mesh = nr.extract_mesh(voxel_size=a.voxel, mesher="hip")     # normalised space
    tr, sc = np.asarray(seq["translation"], np.float64), float(seq["sc_factor"])

    post_h, t_post_h = timed(lambda: M.postprocess_mesh(mesh, tr, sc, backend="hip"), a.reps, a.window)
    post_s, t_post_s = timed(lambda: M.postprocess_mesh(mesh, tr, sc, backend="scipy"), a.reps, a.window)
    big = post_h["biggest_component"]
    sm_h, t_lap_h = timed(lambda: M.filter_laplacian(big.copy(), iterations=3, backend="hip"), a.reps, a.window)
    sm_s, t_lap_s = timed(lambda: M.filter_laplacian(big.copy(), iterations=3, backend="scipy"), a.reps, a.window)
    n_h, t_nrm_h = timed(lambda: big.copy().compute_vertex_normals(backend="hip"), a.reps, a.window)
    n_s, t_nrm_s = timed(lambda: big.copy().compute_vertex_normals(backend="scipy"), a.reps, a.window)
    diag = float(np.linalg.norm(big.vertices.max(0) - big.vertices.min(0)))
    vol0, vol1 = M.mesh_volume(big, backend="hip"), M.mesh_volume(sm_h, backend="hip")
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "frames": a.frames, "reps": a.reps,
           "window_s": a.window, "voxel_size": a.voxel,
           "vertices": int(len(mesh.vertices)), "faces": int(len(mesh.faces)),
           "biggest_component_vertices": int(len(big.vertices)), "biggest_component_faces": int(len(big.faces)),
           "same_faces": bool(all(np.array_equal(post_h[k].faces, post_s[k].faces) for k in post_h)),
           "postprocess_max_vertex_diff_over_diagonal":
               float(np.abs(post_h["smoothed"].vertices - post_s["smoothed"].vertices).max() / diag),
           "filter_max_vertex_diff_over_diagonal": float(np.abs(sm_h.vertices - sm_s.vertices).max() / diag),
           "normals_max_diff": float(np.abs(n_h - n_s).max()),
           "volume_before": vol0, "volume_after_relative_change": abs(vol1 - vol0) / abs(vol0),
           "postprocess_mesh_hip": t_post_h, "postprocess_mesh_scipy": t_post_s,
           "filter_laplacian_hip": t_lap_h, "filter_laplacian_scipy": t_lap_s,
           "vertex_normals_hip": t_nrm_h, "vertex_normals_scipy": t_nrm_s}
    out["postprocess_mesh_scipy_over_hip"] = round(t_post_s["ms"] / t_post_h["ms"], 2)
    out["filter_laplacian_scipy_over_hip"] = round(t_lap_s["ms"] / t_lap_h["ms"], 2)
    out["vertex_normals_scipy_over_hip"] = round(t_nrm_s["ms"] / t_nrm_h["ms"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
