"""Time FusedStep.query_sdf and FusedStep.query_field (SDF only, SDF + normals, all three outputs) on the
same random points in [-1, 1]^3 with the bench's field configuration (amp), in one process, by HIP events:
warm-up, then --reps timed calls each, medians. Writes profiles/r8/query_field.json. --parent-ms records
the parent commit's query_sdf median measured by this tool in the same session.
Usage: python scripts/query_field.py [--points 1048576] [--reps 25] [--parent-ms X] [--out PATH]"""
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
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--pool-frames", type=int, default=4)
    ap.add_argument("--parent-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "query_field.json"))
    a = ap.parse_args()
    from bundlesdf_amd.fused import FusedStep
    dev = torch.device("cuda", 0)
    cfg, pool, frame_start, poses, occ, info, _ = B.build_rank_scene(0, 1, a.pool_frames, dict(amp=True), dev)
    enc, net, pa = B.make_models(cfg, a.pool_frames, dev)
    fs = FusedStep(cfg, pool, torch.from_numpy(poses), occ, enc, net, pa, amp=True)
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (a.points, 3)).astype(np.float32)).to(dev)
    modes = {"query_sdf": lambda: fs.query_sdf(points=pts)}
    if hasattr(fs, "query_field"):   # absent on the parent commit: only query_sdf is timed there
        modes["query_field_sdf"] = lambda: fs.query_field(pts)
        modes["query_field_sdf_normals"] = lambda: fs.query_field(pts, normals=True)
        modes["query_field_all"] = lambda: fs.query_field(pts, normals=True, colour=True)
    out = {"points": a.points, "L": cfg["num_levels"], "log2_hashmap_size": cfg["log2_hashmap_size"], "amp": True,
           "reps": a.reps, "includes": "wait_exchange + nof_pack_mlp + output allocation + the query launch",
           "device": torch.cuda.get_device_name(0)}
    for name, fn in modes.items():
        for _ in range(5):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name + "_ms_median"] = round(float(np.median(ms)), 4)
        out[name + "_ms_min"] = round(float(np.min(ms)), 4)
        out[name + "_ms_max"] = round(float(np.max(ms)), 4)
    base = out["query_sdf_ms_median"]
    for name in modes:
        if name != "query_sdf":
            out[name + "_ratio"] = round(out[name + "_ms_median"] / base, 3)
    if a.parent_ms is not None:
        out["parent_query_sdf_ms_median"] = a.parent_ms
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
