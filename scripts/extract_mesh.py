"""Time the two halves of mesh extraction both ways, in one process, on the synthetic scene after --steps
training steps, on extract_mesh's dense SDF volume at the default voxel size:

  marching cubes  mesh.marching_cubes(volume, 0, backend="torch") (tensor ops on the device volume) against
                  backend="hip" (nof_marching_cubes_count / _emit), both from the device volume to the
                  numpy arrays extract_mesh wraps; and marching_cubes_device alone (device tensors out);
  components      mesh.trimesh_split(mesh, backend="scipy") (host, connected_components) against
                  backend="hip" (nof_mesh_components), both from the host Mesh to the list of parts.

HIP events around each call, warm-up, then the median of --reps passes (the method of
scripts/vertex_color.py); every call ends on the host, so the events span its host work too. The two
backends are also compared for equality. Writes profiles/r11/extract_mesh.json. No threshold is asserted.
Usage: python scripts/extract_mesh.py [--frames 8] [--steps 300] [--reps 10] [--voxel 0.003] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, {"ms": round(float(np.median(ms)), 3), "ms_min_max": [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--voxel", type=float, default=0.003)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "extract_mesh.json"))
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
    tx, ty, tz = M.grid_axes(cfg["bounding_box"], a.voxel * cfg["sc_factor"])
    occ = nr._occ_trace_level() if nr.octree_m is not None else None

    def query():
        return nr.trainer.query_sdf(axes=(tx, ty, tz), occ=occ).reshape(len(tx), len(ty), len(tz))
    vol, t_query = timed(query, a.reps)
    (v_t, f_t), t_torch = timed(lambda: M.marching_cubes(vol, 0.0, backend="torch"), a.reps)
    (v_h, f_h), t_hip = timed(lambda: M.marching_cubes(vol, 0.0, backend="hip"), a.reps)
    _, t_dev = timed(lambda: M.marching_cubes_device(vol, 0.0), a.reps)
    same_mesh = bool(np.array_equal(v_t, v_h) and np.array_equal(f_t, f_h))
    mesh = M.Mesh(v_h, f_h)
    parts_s, t_scipy = timed(lambda: M.trimesh_split(mesh, min_edge=1000, backend="scipy"), a.reps)
    parts_h, t_cc = timed(lambda: M.trimesh_split(mesh, min_edge=1000, backend="hip"), a.reps)
    _, t_lab = timed(lambda: M.component_labels(mesh.faces, len(mesh.vertices)), a.reps)
    same_parts = len(parts_s) == len(parts_h) and all(
        np.array_equal(p.vertices, q.vertices) and np.array_equal(p.faces, q.faces) for p, q in zip(parts_s, parts_h))
    lab = M.component_labels(mesh.faces, len(mesh.vertices))
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "frames": a.frames, "reps": a.reps,
           "voxel_size": a.voxel, "volume": [len(tx), len(ty), len(tz)], "grid_points": int(vol.numel()),
           "vertices": int(len(v_h)), "faces": int(len(f_h)), "components": int(len(torch.unique(lab))),
           "parts_min_edge_1000": len(parts_h), "same_mesh": same_mesh, "same_parts": bool(same_parts),
           "query_sdf": t_query, "marching_cubes_torch": t_torch, "marching_cubes_hip": t_hip,
           "marching_cubes_device_only": t_dev, "trimesh_split_scipy": t_scipy, "trimesh_split_hip": t_cc,
           "component_labels_only": t_lab}
    out["marching_cubes_torch_over_hip"] = round(t_torch["ms"] / t_hip["ms"], 2)
    out["trimesh_split_scipy_over_hip"] = round(t_scipy["ms"] / t_cc["ms"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
