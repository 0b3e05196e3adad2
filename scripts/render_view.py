"""Turntable of the synthetic scene through the free-camera surface render (NerfRunner.render_view):
trains the synthetic runner for --steps steps, renders --frames views around the object to PNG (colour,
normal as (n + 1) / 2, depth) and writes timing and march figures to --json.

    python scripts/render_view.py --frames 8 --size 640x480

Figures (render_view.json): the view render against FusedStep.render_rays on the same number of pool
rays in the same process (medians of --reps after warm-up, HIP events), the mean number of 32-sample
tiles marched per ray, the hit share, and — rendering training frame 1 from its own pose — the median
|depth - observed depth| over hit pixels next to the truncation band."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def turntable(c2w, i, n):
    """c2w turned by 2 pi i / n about the y axis through the origin of normalised space."""
    a = 2 * np.pi * i / n
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return R @ np.asarray(c2w, np.float64)


def median_ms(fn, reps, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="640x480", help="WxH of the rendered views")
    ap.add_argument("--steps", type=int, default=300, help="training steps before rendering")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "turntable"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r9", "render_view.json"))
    ap.add_argument("--fp32", action="store_true")
    args = ap.parse_args()
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.mesh import write_png
    from bundlesdf_amd.nerf_runner import NerfRunner
    W, H = (int(x) for x in args.size.lower().split("x"))
    seq = SY.make_sequence(3, seed=1)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=args.steps, N_rand=2048,
                         num_levels=16, amp=not args.fp32)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    K = np.asarray(nr.K, np.float64).copy()
    K[0] *= W / nr.W
    K[1] *= H / nr.H
    os.makedirs(args.out, exist_ok=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    hits = []
    for i in range(args.frames):
        r = nr.render_view(turntable(nr.poses[1], i, args.frames), K=K, H=H, W=W)
        hit = r["hit"]
        hits.append(float(hit.mean()))
        far = r["depth"][hit].max() if hit.any() else 1.0
        depth = np.where(hit, 255 * (1 - 0.8 * r["depth"] / far), 0)
        write_png(os.path.join(args.out, f"view_{i:03d}_colour.png"), (r["rgb"] * 255).astype(np.uint8))
        write_png(os.path.join(args.out, f"view_{i:03d}_normal.png"),
                  (np.where(hit[..., None], (r["normal"] + 1) / 2, 0) * 255).astype(np.uint8))
        write_png(os.path.join(args.out, f"view_{i:03d}_depth.png"),
                  np.repeat(depth[..., None], 3, -1).astype(np.uint8))
    # timing: the first view against render_rays on as many pool rays
    tr = nr.trainer
    c2w = turntable(nr.poses[1], 0, args.frames)
    n_pool = int(tr.pool.shape[0])
    ids = (torch.arange(H * W, device=tr.dev) % n_pool).to(torch.int32)
    step = 0.5 * nr.get_truncation()
    view_ms = median_ms(lambda: tr.render_view(c2w, K, H, W, step=step), args.reps)
    rays_ms = median_ms(lambda: tr.render_rays(ids, global_step=nr.global_step), args.reps)
    st = tr.render_view(c2w, K, H, W, step=step, stats=True)
    # a training frame from its own pose against its observed depth
    own = nr.render_view(nr.poses[1])
    obs = np.asarray(seq["depths"][1][..., 0], np.float32)
    both = own["hit"] & (obs < cfg["far"] * cfg["sc_factor"]) & (seq["masks"][1][..., 0] > 0)
    fig = {
        "size": [W, H], "rays": H * W, "amp": not args.fp32, "train_steps": args.steps, "reps": args.reps,
        "step": step, "max_steps": 512, "n_refine": 8,
        "render_view_ms": view_ms, "render_rays_ms": rays_ms, "ratio": view_ms / rays_ms,
        "render_rays_samples_per_ray": cfg["N_samples"] + cfg["N_samples_around_depth"],
        "tiles_per_ray_mean": float(st["tiles"].float().mean()),
        "tiles_per_traced_ray_mean": float(st["tiles"][st["tiles"] > 0].float().mean()) if (st["tiles"] > 0).any() else 0.0,
        "hit_share": float(st["hit"].float().mean()), "turntable_hit_share": hits,
        "own_pose_hit_pixels": int(both.sum()),
        "own_pose_median_abs_depth_error": float(np.median(np.abs(own["depth"] - obs)[both])) if both.any() else None,
        "truncation_band": nr.get_truncation(),
    }
    with open(args.json, "w") as f:
        json.dump(fig, f, indent=1)
    print(json.dumps(fig))


if __name__ == "__main__":
    main()
