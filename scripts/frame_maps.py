"""Time the frame-map front end on the size the tracker runs it at and record the figures.

15 synthetic frames of 640x480: MeshRenderer depth of a bumpy icosphere (5120 faces, about 0.5 m from
the camera) with zero holes and speckle added, through prepare_frames with the reference's settings;
then a lift of 20,000 pixel matches spread over every frame pair, and the covisibility of all 210
ordered pairs. Device: the median of 3 calls after one warm-up, a host clock around the whole call
(host validation, uploads, every launch) ending in a device synchronise; kernel time alone is not
measured. Oracle: tests/frame_maps_oracle.py (numpy float64) on 16 threads, --oracle-runs runs (1 by
default: the figure is a scale, not a race). Also the hand-over to optimize_poses that
tests/test_gpu_frame_maps.py runs, with its drift from the true poses. The figures are recorded in
profiles/r18/frame_maps.json, not asserted.

    python scripts/frame_maps.py [--out profiles/r18/frame_maps.json] [--skip-oracle]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def bumpy_mesh(subdivisions=4, radius=0.08):
    """An icosphere whose radius varies by a few per cent, so that no rotation maps it onto itself."""
    from bundlesdf_amd.mesh import Mesh
    from tests.mesh_render_oracle import icosphere
    v, f = icosphere(subdivisions, 1.0)
    r = radius * (1.0 + 0.12 * np.sin(4.0 * v[:, 0]) * np.cos(3.0 * v[:, 1]) + 0.08 * np.sin(5.0 * v[:, 2] + 1.0))
    return Mesh((v * r[:, None]).astype(np.float32).astype(np.float64), f)


def object_poses(n, seed=0, dist=0.5):
    """ob_in_cam [n,4,4]: the object about `dist` in front of the camera, turned a little more each frame."""
    from tests.mesh_render_oracle import _pose
    rng = np.random.default_rng(seed)
    return np.stack([_pose([0.03 * k, 0.05 * k, -0.02 * k], [0.004 * k, -0.003 * k, dist]) +
                     np.pad(rng.uniform(-0.002, 0.002, (3, 1)), ((0, 1), (3, 0))) for k in range(n)])


def render_depth(mesh, ob_in_cams, K, H, W, dev):
    from bundlesdf_amd.mesh_render import MeshRenderer
    return MeshRenderer(mesh, K, H, W, znear=0.1, zfar=2.0, device=dev).render(ob_in_cams, colour="flat")["depth"]


def hand_over(dev, H=96, W=128, n_outer=3):
    """Render 3 known poses, prepare_frames, optimize_poses (dense term only) from the true poses."""
    from bundlesdf_amd import frames as F
    from bundlesdf_amd.pose_graph import optimize_poses
    K = np.array([[260.0, 0.0, W / 2 - 0.5], [0.0, 260.0, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    ob_in_cam = object_poses(3)
    depth = render_depth(bumpy_mesh(3), ob_in_cam, K, H, W, dev)
    maps = F.prepare_frames(depth, K)
    truth = np.linalg.inv(ob_in_cam)                     # camera in world, the world being the object
    poses, history = optimize_poses(truth, points=maps.points, normals=maps.normals, K=maps.K, n_outer=n_outer)
    torch.cuda.synchronize()
    poses, history = poses.cpu().numpy(), history.cpu().numpy()
    return dict(map=[H, W], n_outer=n_outer, n_valid=maps.n_valid.cpu().numpy().tolist(),
                poses_finite=bool(np.isfinite(poses).all()), dense_correspondences=history[:, 3].tolist(),
                dense_energy=history[:, 1].tolist(), drift_max_abs_pose_entry=float(np.abs(poses - truth).max()),
                drift="largest absolute difference of a pose entry from the true poses after the dense-only "
                      "optimisation started at the true poses; recorded, no bound derived")


def build_case(dev, N=15, H=480, W=640, rows=20000, seed=0):
    rng = np.random.default_rng(seed)
    K = np.array([[1300.0, 0.0, W / 2 - 0.5], [0.0, 1300.0, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    ob_in_cam = object_poses(N)
    depth = render_depth(bumpy_mesh(4), ob_in_cam, K, H, W, dev).cpu().numpy()
    hit = depth > 0
    depth[hit & (rng.uniform(size=depth.shape) < 0.02)] = 0.0                              # holes
    speck = hit & (rng.uniform(size=depth.shape) < 0.005)
    depth[speck] += rng.uniform(0.01, 0.05, int(speck.sum())).astype(np.float32)          # speckle
    mask = hit.astype(np.uint8)
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    per = rows // len(pairs)
    vs, us = np.nonzero(hit.any(0))
    pick = rng.integers(0, len(vs), (2, len(pairs) * per))
    uv_a = np.stack([us[pick[0]], vs[pick[0]]], 1) + rng.uniform(-0.5, 0.5, (len(pairs) * per, 2))
    uv_b = np.stack([us[pick[1]], vs[pick[1]]], 1) + rng.uniform(-0.5, 0.5, (len(pairs) * per, 2))
    return dict(depth=depth, K=K, mask=mask, poses=np.linalg.inv(ob_in_cam), pair_frames=np.array(pairs, np.int32),
                pair_start=(np.arange(len(pairs) + 1) * per).astype(np.int32), uv_a=uv_a, uv_b=uv_b,
                ordered=[(i, j) for i in range(N) for j in range(N) if i != j])


def _median_ms(call, reps=3):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "frame_maps.json"))
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--oracle-runs", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_maps.py times the device path: no HIP device")
    from bundlesdf_amd import frames as F
    from tests import frame_maps_oracle as O
    dev = torch.device("cuda", 0)
    case = build_case(dev)
    maps = F.prepare_frames(case["depth"], case["K"], case["mask"], device=dev)
    lift_kw = dict(poses=case["poses"], max_dist=0.2, max_normal_deg=45.0)
    prep_ms, prep_all = _median_ms(lambda: F.prepare_frames(case["depth"], case["K"], case["mask"], device=dev))
    depth_d, mask_d = torch.from_numpy(case["depth"]).to(dev), torch.from_numpy(case["mask"]).to(dev)
    prep_dev_ms, prep_dev_all = _median_ms(lambda: F.prepare_frames(depth_d, case["K"], mask_d))
    lift_ms, lift_all = _median_ms(lambda: F.lift_matches(maps, case["pair_frames"], case["uv_a"], case["uv_b"],
                                                          case["pair_start"], **lift_kw))
    covis_ms, covis_all = _median_ms(lambda: F.covisibility(maps, case["poses"], case["ordered"]))
    lifted = F.lift_matches(maps, case["pair_frames"], case["uv_a"], case["uv_b"], case["pair_start"], **lift_kw)
    ratio, counts = F.covisibility(maps, case["poses"], case["ordered"])
    torch.cuda.synchronize()
    res = dict(frames=len(case["depth"]), size=[480, 640], device=torch.cuda.get_device_name(0),
               timing="host clock around each call (validation, uploads, launches) to a device synchronise, median of "
                      "3 after a warm-up; kernel time alone not measured",
               prepare_frames_ms_from_host_arrays=prep_ms, prepare_frames_ms_from_host_arrays_all=prep_all,
               prepare_frames_ms_from_device_tensors=prep_dev_ms, prepare_frames_ms_from_device_tensors_all=prep_dev_all,
               lift_rows=int(case["pair_start"][-1]), lift_pairs=len(case["pair_frames"]), lift_ms=lift_ms, lift_ms_all=lift_all,
               lift_valid_rows=int(lifted.valid.sum().item()),
               covis_pairs=len(case["ordered"]), covis_ms=covis_ms, covis_ms_all=covis_all,
               covis_ratio_min_max=[float(ratio.min().item()), float(ratio.max().item())],
               n_valid=maps.n_valid.cpu().numpy().tolist(), hand_over=hand_over(dev))
    if not args.skip_oracle:
        tp, tl, tc = [], [], []
        pts, nrm = maps.points.cpu().numpy(), maps.normals.cpu().numpy()
        for _ in range(args.oracle_runs):
            t = time.perf_counter()
            want = O.prepare(case["depth"], case["K"], case["mask"])
            tp.append(time.perf_counter() - t)
            t = time.perf_counter()
            wl = O.lift(pts, nrm, case["pair_frames"], case["pair_start"], case["uv_a"], case["uv_b"], **lift_kw)
            tl.append(time.perf_counter() - t)
            t = time.perf_counter()
            _, wc = O.covisibility(pts, nrm, case["poses"], case["ordered"])
            tc.append(time.perf_counter() - t)
        res.update(oracle_threads=int(os.environ["OMP_NUM_THREADS"]), oracle_runs=args.oracle_runs,
                   oracle_prepare_s_median=float(np.median(tp)), oracle_lift_s_median=float(np.median(tl)),
                   oracle_covis_s_median=float(np.median(tc)),
                   end_to_end_depth_pixels_differing=int((want["depth"] != maps.depth.cpu().numpy()).sum()),
                   end_to_end_note="the oracle's whole chain on its own stages against the device's: the bilateral "
                                   "passes may differ by one float32 ulp, which later thresholds can amplify; the "
                                   "tests compare stage by stage instead",
                   lift_valid_equal=bool(np.array_equal(wl[4], lifted.valid.cpu().numpy())),
                   covis_counts_equal=bool(np.array_equal(wc, counts.cpu().numpy())))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
