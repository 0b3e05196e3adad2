"""Time FusedStep.render_rays on one frame's rays of the bench pool (amp) against the k_encode + k_colour
buckets of a training step on the same rays, in one process: writes profiles/r7/render_frame.json.
Usage: python scripts/render_frame.py [--pool-frames 64] [--reps 9] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "render_frame.json"))
    a = ap.parse_args()
    from bundlesdf_amd.fused import FusedStep
    dev = torch.device("cuda", 0)
    cfg, pool, frame_start, poses, occ, info, _ = B.build_rank_scene(0, 1, a.pool_frames, dict(amp=True), dev)
    enc, net, pa = B.make_models(cfg, a.pool_frames, dev)
    f = a.pool_frames // 2
    ids = torch.arange(int(frame_start[f]), int(frame_start[f + 1]), dtype=torch.int32, device=dev)
    R = int(ids.numel())
    fs = FusedStep(cfg, pool, torch.from_numpy(poses), occ, enc, net, pa, amp=True, time_kernels=True)
    for _ in range(3):   # warm-up: a few training steps move the field off its initial constant
        fs.step(ids=ids)
    fs.field_kernel_breakdown()
    for _ in range(a.reps):
        fs.step(ids=ids)
    kb, n = fs.field_kernel_breakdown()
    times = {}
    for samples in (False, True):
        for _ in range(3):
            fs.render_rays(ids, samples=samples, chunk=R)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fs.render_rays(ids, samples=samples, chunk=R)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        times[samples] = ms
    out = {"R": R, "S": cfg["N_samples"] + cfg["N_samples_around_depth"], "amp": True, "reps": a.reps,
           "render_rays_ms_median": round(float(np.median(times[False])), 4),
           "render_rays_ms_min": round(float(np.min(times[False])), 4),
           "render_rays_samples_ms_median": round(float(np.median(times[True])), 4),
           "render_includes": "prologue + nof_trace_rays + nof_render_rays (3 kernels) + output allocation",
           "yardstick_k_encode_ms": round(kb["k_encode"], 4), "yardstick_k_colour_ms": round(kb["k_colour"], 4),
           "yardstick_ms": round(kb["k_encode"] + kb["k_colour"], 4), "yardstick_calls": n,
           "device": torch.cuda.get_device_name(0)}
    out["ratio"] = round(out["render_rays_ms_median"] / out["yardstick_ms"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
