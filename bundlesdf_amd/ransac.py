"""Match filtering on the device: multi-pair RANSAC over 3-D correspondences.

Which feature matches between two frames agree with one rigid motion: the step the reference runs
for every new frame against its neighbours and for every key-frame pair before the pose graph
(SiftManager::runRansacMultiPairGPU over BundleTrack/src/cuda/cuda_ransac.cu). Here it is
nof_ransac_pairs (csrc/ransac.hip, include/nof.h group 8): hashed draws, a three-point rigid fit per
trial, integer scores, the lowest trial of the highest score as the winner, flags recomputed from
the winning pose and the 17 sums of a refit over the inliers. Every run gives the same bits.

No CPU fallback: ransac_pairs raises if libnof.so cannot run. The refit's 3x3 solve is
evaluate._kabsch on the host, after one read of the sums.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._args import as_host, as_tensor, default_device
from .evaluate import _kabsch

__all__ = ["ransac_pairs", "inliers_per_pair", "RansacResult", "ROW_TILE", "MAX_PAIRS", "MAX_TRIALS", "MAX_CONF"]

ROW_TILE = 256          # RANSAC_TILE of csrc/ransac.hip: rows a scoring block stages at a time
MAX_PAIRS = 65535
MAX_TRIALS = 65536
MAX_CONF = 32767.0


@dataclass
class RansacResult:
    """Device tensors of one ransac_pairs call (refit_pose is host numpy)."""
    pair_start: torch.Tensor            # [P+1] i32
    inlier: torch.Tensor                # [M] bool
    n_inliers: torch.Tensor             # [P] i32
    score: torch.Tensor                 # [P] f64: the integer score / 65536
    best_trial: torch.Tensor            # [P] i32, -1 = no trial scored
    pose: torch.Tensor                  # [P,4,4] f64, A onto B
    sums: torch.Tensor                  # [P,17] f64
    refit_pose: Optional[np.ndarray] = None      # [P,4,4] f64
    trial_idx: Optional[torch.Tensor] = None     # [P,T,3] i32
    trial_pose: Optional[torch.Tensor] = None    # [P,T,12] f64
    trial_live: Optional[torch.Tensor] = None    # [P,T] u8
    trial_score: Optional[torch.Tensor] = None   # [P,T] i64, fixed point (x 65536)


def _is_list(a):
    return isinstance(a, (list, tuple)) and len(a) > 0 and (torch.is_tensor(a[0]) or np.ndim(a[0]) >= 1)


def _rows(a, name, width):
    """[M,width] (or [M] for width 0) f64 from an array, a tensor or a list of per-pair arrays, left on the
    device it came from: everything is validated before the first device call."""
    if _is_list(a):
        return torch.cat([_rows(x, name, width) for x in a])
    t = as_tensor(a, np.float64).to(torch.float64)
    if width:
        if t.numel() % width:
            raise ValueError(f"ransac_pairs: {name} must be [M,{width}], got {tuple(t.shape)}")
        return t.reshape(-1, width).contiguous()
    return t.reshape(-1).contiguous()


def _per_pair(v, P, name, default):
    if v is None:
        return np.full(P, default, np.float64)
    a = as_host(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.full(P, a[0])
    if a.shape != (P,):
        raise ValueError(f"ransac_pairs: {name} must be a scalar or [{P}], got {a.shape}")
    if np.isnan(a).any() or (a < 0).any():
        raise ValueError(f"ransac_pairs: {name} must not be negative or NaN")
    return a


def ransac_pairs(pts_a, pts_b, pair_start=None, normals_a=None, normals_b=None, conf=None, *, inlier_dist,
                 normal_angle_deg=None, n_trials=2000, max_trans=None, max_rot_deg=None, min_inliers=5, seed=0,
                 refit=True, return_trials=False, device=None):
    """RANSAC over the 3-D matches of P frame pairs in one call -> RansacResult.

    pts_a / pts_b [M,3] (arrays or tensors) with pair_start [P+1] (pair p owns rows pair_start[p] ..
    pair_start[p+1]-1; None = one pair), or lists of per-pair [n_p,3] arrays in place of pair_start.
    normals_a / normals_b: unit normals of both sides or neither; conf [M] match weights in
    [0, 32767], rounded to multiples of 1/65536. The model maps A onto B, b ~ R a + t.

    inlier_dist: a row is an inlier within this distance and, with normals, when the rotated normal
    of A is within normal_angle_deg of B's (None: any angle passes).
    max_trans / max_rot_deg (scalars or [P]; None = no gate) reject a trial whose translation is
    longer or whose rotation is larger. A pair that ends with fewer than min_inliers inliers has its
    flags cleared. With refit, refit_pose is the least-squares rigid fit over the inliers (identity
    for a cleared pair). With return_trials the per-trial draws, poses, live flags and scores come
    back too. include/nof.h (group 8) fixes every operation's order."""
    listed = _is_list(pts_a)
    if listed:
        if pair_start is not None:
            raise ValueError("ransac_pairs: give pair_start or lists of per-pair arrays, not both")
        if not isinstance(pts_b, (list, tuple)) or len(pts_b) != len(pts_a):
            raise ValueError("ransac_pairs: pts_a and pts_b must list the same pairs")
        counts = [int(np.prod(tuple(x.shape))) // 3 for x in pts_a]
        for p, (x, n) in enumerate(zip(pts_b, counts)):
            if int(np.prod(tuple(x.shape))) // 3 != n:
                raise ValueError(f"ransac_pairs: pair {p} has {n} rows in pts_a and another count in pts_b")
        ps = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if (normals_a is None) != (normals_b is None):
        raise ValueError("ransac_pairs: normals must be given for both sides or for neither")
    a, b = _rows(pts_a, "pts_a", 3), _rows(pts_b, "pts_b", 3)
    M = len(a)
    if len(b) != M:
        raise ValueError(f"ransac_pairs: pts_a has {M} rows, pts_b {len(b)}")
    if M >= 2 ** 31:
        raise ValueError(f"ransac_pairs: {M} rows (max 2^31 - 1)")
    if not listed:
        ps = np.array([0, M], np.int64) if pair_start is None else as_host(pair_start, np.int64).reshape(-1)
    P = len(ps) - 1
    if P < 1 or P > MAX_PAIRS:
        raise ValueError(f"ransac_pairs: {P} pairs (1 .. {MAX_PAIRS})")
    if ps[0] != 0 or ps[-1] != M or (np.diff(ps) < 0).any():
        raise ValueError(f"ransac_pairs: pair_start must start at 0, never decrease and end at M={M}")
    n_trials = int(n_trials)
    if n_trials < 1 or n_trials > MAX_TRIALS:
        raise ValueError(f"ransac_pairs: n_trials={n_trials} (1 .. {MAX_TRIALS})")
    if not float(inlier_dist) >= 0:
        raise ValueError(f"ransac_pairs: inlier_dist={inlier_dist} must not be negative")
    na = nb = None
    if normals_a is not None:
        na, nb = _rows(normals_a, "normals_a", 3), _rows(normals_b, "normals_b", 3)
        if len(na) != M or len(nb) != M:
            raise ValueError(f"ransac_pairs: normals must have {M} rows, got {len(na)} and {len(nb)}")
    w = None
    if conf is not None:
        w = _rows(conf, "conf", 0)
        if len(w) != M:
            raise ValueError(f"ransac_pairs: conf must have {M} entries, got {len(w)}")
        if M and not bool(((w >= 0) & (w <= MAX_CONF)).all()):       # also catches NaN
            raise ValueError(f"ransac_pairs: conf must lie in [0, {MAX_CONF:g}]")
    mt = _per_pair(max_trans, P, "max_trans", math.inf)
    mr = _per_pair(max_rot_deg, P, "max_rot_deg", math.inf)
    min_trace = np.where(np.isinf(mr), -np.inf, 1.0 + 2.0 * np.cos(np.deg2rad(np.minimum(mr, 180.0))))
    cos_normal = -math.inf if normal_angle_deg is None else math.cos(math.radians(float(normal_angle_deg)))

    dev = default_device(a, device)
    L = _lib.lib()
    i32, f64 = torch.int32, torch.float64
    with torch.cuda.device(dev):
        a, b, na, nb, w = (None if x is None else x.to(dev).contiguous() for x in (a, b, na, nb, w))
        out = RansacResult(
            pair_start=torch.from_numpy(ps.astype(np.int32)).to(dev),
            inlier=torch.zeros(M, dtype=torch.uint8, device=dev),
            n_inliers=torch.zeros(P, dtype=i32, device=dev),
            score=torch.zeros(P, dtype=torch.int64, device=dev),
            best_trial=torch.full((P,), -1, dtype=i32, device=dev),
            pose=torch.eye(4, dtype=f64, device=dev).repeat(P, 1, 1).contiguous(),
            sums=torch.zeros((P, 17), dtype=f64, device=dev))
        gates = torch.from_numpy(np.stack([mt * mt, min_trace])).to(dev)
        nbytes = int(L.nof_ransac_workspace_bytes(P, M, n_trials))
        ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
        if return_trials:
            out.trial_idx = torch.zeros((P, n_trials, 3), dtype=i32, device=dev)
            out.trial_pose = torch.zeros((P, n_trials, 12), dtype=f64, device=dev)
            out.trial_live = torch.zeros((P, n_trials), dtype=torch.uint8, device=dev)
            out.trial_score = torch.zeros((P, n_trials), dtype=torch.int64, device=dev)
        D = _lib.RansacDesc()
        D.pts_a, D.pts_b, D.normals_a, D.normals_b, D.conf = (_lib.ptr(x) for x in (a, b, na, nb, w))
        D.pair_start, D.max_trans_sq, D.min_trace = _lib.ptr(out.pair_start), _lib.ptr(gates[0]), _lib.ptr(gates[1])
        D.M, D.P, D.n_trials, D.seed, D.min_inliers = M, P, n_trials, int(seed) & 0xFFFFFFFF, int(min_inliers)
        D.inlier_dist_sq, D.cos_normal = float(inlier_dist) * float(inlier_dist), cos_normal
        D.workspace, D.workspace_bytes = _lib.ptr(ws), ws.numel()
        D.best_trial, D.score, D.pose, D.n_inliers = (_lib.ptr(x) for x in (out.best_trial, out.score, out.pose,
                                                                            out.n_inliers))
        D.inlier, D.sums = _lib.ptr(out.inlier), _lib.ptr(out.sums)
        D.trial_idx, D.trial_pose, D.trial_live, D.trial_score = (_lib.ptr(x) for x in (
            out.trial_idx, out.trial_pose, out.trial_live, out.trial_score))
        _lib.check(L.nof_ransac_pairs(ctypes.byref(D), _lib.stream_of(a)), "ransac_pairs")
        out.inlier = out.inlier.bool()
        out.score = out.score.double() / 65536.0
    if refit:
        s = out.sums.cpu().numpy()
        out.refit_pose = np.stack([_kabsch(r) if r[0] >= max(1, int(min_inliers)) else np.eye(4) for r in s])
    return out


def inliers_per_pair(result):
    """The inlier rows of every pair, as indices local to the pair (what runRansacMultiPairGPU hands
    back): a list of P int64 numpy arrays."""
    flags = result.inlier.cpu().numpy()
    ps = result.pair_start.cpu().numpy()
    return [np.flatnonzero(flags[ps[p]:ps[p + 1]]).astype(np.int64) for p in range(len(ps) - 1)]
