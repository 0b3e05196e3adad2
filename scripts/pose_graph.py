"""Time optimize_poses on the size the tracker runs it at and record the figures.

15 frames of 160x120 point / normal maps of the two-sphere scene of tests/pose_graph_oracle.py, radius
5, 7 x 5 iterations, about 20,000 sparse matches over every frame pair. Device: the median of 3 calls
after one warm-up, a host clock around the whole call (host validation, uploads, every launch) ending
in a device synchronise; kernel time alone is not measured. Oracle: tests/pose_graph_oracle.optimise on
16 threads, the median of --oracle-runs runs (3 by default; one run takes minutes). The figures are
recorded in profiles/r16/pose_graph.json, not asserted.

    python scripts/pose_graph.py [--out profiles/r16/pose_graph.json] [--skip-oracle]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bundlesdf_amd import pose_graph as PG  # noqa: E402
from tests import pose_graph_oracle as O  # noqa: E402


def build_case(N=15, H=120, W=160, rows=20000, seed=0):
    rng = np.random.default_rng(seed)
    truth = O._ring_poses(N, rng, spread=0.1)
    K = np.array([[200.0, 0.0, W / 2 - 0.3], [0.0, 200.0, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    maps = [O.render_maps(T, K, H, W) for T in truth]
    fixed = np.zeros(N, bool)
    fixed[0] = True
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    per = rows // len(pairs)
    pf, a, b, ps = [], [], [], [0]
    for (i, j) in pairs:
        X = rng.uniform(-0.08, 0.08, (per, 3)) + (0.0, 0.0, 0.04)
        pf.append((i, j))
        a.append(O.xform(O.inverse(truth[i]), X))
        b.append(O.xform(O.inverse(truth[j]), X))
        ps.append(ps[-1] + per)
    return dict(poses=O._perturb(truth, fixed, rng, 0.004, 0.0005), truth=truth, fixed=fixed, K=K, radius=5,
                points=np.stack([m[0] for m in maps]), normals=np.stack([m[1] for m in maps]),
                pair_frames=np.array(pf, np.int32), pts_a=np.concatenate(a), pts_b=np.concatenate(b),
                pair_start=np.array(ps, np.int32), weight=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "pose_graph.json"))
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--oracle-runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_graph.py times the device path: no HIP device")
    dev = torch.device("cuda", 0)
    case = build_case()
    kw = {k: case[k] for k in ("pair_frames", "pts_a", "pts_b", "pair_start", "points", "normals", "K", "fixed", "radius")}

    def call():
        t = time.perf_counter()
        poses, history = PG.optimize_poses(case["poses"], device=dev, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t, poses, history

    call()
    runs = [call() for _ in range(3)]
    history = runs[-1][2].cpu().numpy()
    res = dict(frames=len(case["poses"]), map=[120, 160], radius=5, n_outer=7, n_inner=5,
               sparse_rows=int(case["pair_start"][-1]), sparse_pairs=len(case["pair_frames"]),
               device=torch.cuda.get_device_name(0),
               device_call_ms_median_of_3=1e3 * float(np.median([r[0] for r in runs])),
               device_call_ms_all=[1e3 * r[0] for r in runs],
               timing="host clock around optimize_poses (validation, uploads, launches) to a device synchronise; "
                      "kernel time alone not measured",
               history_first=history[0].tolist(), history_last=history[-1].tolist(),
               pose_error_start=O.pose_error(case["poses"], case["truth"]),
               pose_error_end=O.pose_error(runs[-1][1].cpu().numpy(), case["truth"]))
    if not args.skip_oracle:
        ts = []
        for _ in range(args.oracle_runs):
            t = time.perf_counter()
            want = O.optimise(case)
            ts.append(time.perf_counter() - t)
        res.update(oracle_threads=int(os.environ["OMP_NUM_THREADS"]), oracle_runs=args.oracle_runs, oracle_s_median=float(np.median(ts)),
                   oracle_s_all=ts, poses_away_from_oracle=float(np.abs(want["poses"] - runs[-1][1].cpu().numpy()).max()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
