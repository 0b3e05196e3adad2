"""Time bundlesdf_amd.ransac.ransac_pairs at the reference's shape: 20 pairs x 2000 rows x 2000
trials (its max_iter and a typical match count), planted poses, medians of 3 with the host calls
included, against the numpy oracle (tests/ransac_oracle.py) on 16 threads. Writes
profiles/r15/ransac.json; the figures are recorded, not asserted.

    python scripts/ransac.py [--pairs 20] [--rows 2000] [--trials 2000] [--out profiles/r15/ransac.json]
"""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bundlesdf_amd import _lib  # noqa: E402
from bundlesdf_amd import ransac as R  # noqa: E402
from tests import ransac_oracle as O  # noqa: E402


def oracle_run(c, threads):
    """The oracle's whole call, one pair per task."""
    sl = O.pair_slices(c)
    T = c["n_trials"]
    idx, ok = O.draws(len(sl), T, [s.stop - s.start for s in sl], c["seed"])
    max_trans_sq, min_trace, _, _ = O.settings(c)

    def one(p):
        s = sl[p]
        sub = dict(c, pts_a=c["pts_a"][s], pts_b=c["pts_b"][s], normals_a=c["normals_a"][s], normals_b=c["normals_b"][s],
                   pair_start=np.array([0, s.stop - s.start]))
        k = np.flatnonzero(ok[p])                      # the pair keeps the draws of its own index
        poses, live = np.zeros((1, T, 12)), np.zeros((1, T), bool)
        poses[0, k] = O.pose12(*O.fit_svd(sub["pts_a"][idx[p, k]], sub["pts_b"][idx[p, k]]))
        live[0, k] = O.gate(poses[0, k], max_trans_sq[p], min_trace[p])
        return O.finish(sub, poses, live, O.trial_scores(sub, poses, live))["n_inliers"][0]
    with cf.ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(sl))))


def median_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--trials", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "ransac.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.lib()
    rng = np.random.default_rng(15)
    c = O._join([O._pair(rng, a.rows, 0.01) for _ in range(a.pairs)], n_trials=a.trials, seed=1)
    kw = {k: c[k] for k in ("inlier_dist", "normal_angle_deg", "n_trials", "min_inliers", "seed")}
    host = (c["pts_a"], c["pts_b"], c["pair_start"], c["normals_a"], c["normals_b"])
    on_dev = tuple(torch.from_numpy(np.array(x)).to(dev) for x in (c["pts_a"], c["pts_b"])) + (c["pair_start"],) + tuple(
        torch.from_numpy(np.array(x)).to(dev) for x in (c["normals_a"], c["normals_b"]))

    def call(args, **more):
        res = R.ransac_pairs(*args, device=dev, **kw, **more)
        torch.cuda.synchronize()
        return res

    res = call(host)                                             # warm-up: library load, allocator
    planted_ok = bool(np.array_equal(res.inlier.cpu().numpy(), c["planted"]))
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "rows_per_pair": a.rows, "trials": a.trials,
           "row_tests": a.pairs * a.rows * a.trials, "normals": True, "inlier_share": 0.6,
           "workspace_bytes": int(_lib.lib().nof_ransac_workspace_bytes(a.pairs, a.pairs * a.rows, a.trials)),
           "reference_flag_array_bytes": a.pairs * a.rows * a.trials * 4,
           "device_from_numpy_with_refit": median_ms(lambda: call(host)),
           "device_from_tensors_with_refit": median_ms(lambda: call(on_dev)),
           "device_from_tensors_no_refit": median_ms(lambda: call(on_dev, refit=False)),
           "planted_inliers_recovered": planted_ok}
    want = None

    def run_oracle():
        nonlocal want
        want = oracle_run(c, a.threads)
    out["oracle_threads"] = a.threads
    out["oracle_numpy"] = median_ms(run_oracle)
    out["n_inliers_equal_oracle"] = bool(res.n_inliers.cpu().tolist() == [int(x) for x in want])
    out["oracle_over_device"] = round(out["oracle_numpy"]["ms"] / out["device_from_tensors_with_refit"]["ms"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
